"""The feature pass's third mode (RT_AOV_FULL) without a GPU: the twin of its sums (tests/_aov_full_twin.py) on the rooms of
tests/_aov_full_worlds.py — that they reach what the mode is for, on the twin's own counters, before any kernel is compared with it — and the mirrors: the
constant, the Python argument check, the C++ enum and the render tool's choice of mode."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import _aov_full_twin as FT
import _aov_full_worlds as FW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, pkg

F = np.float32
W, H, SPP, SEED = FW.W, FW.H, FW.SPP, FW.SEED


@pytest.fixture(scope="module")
def p():
    return pkg()


@functools.lru_cache(maxsize=None)
def run(**kw):
    """the twin's sums of FW.room(**kw) and its counters; fresh_rng goes to the twin, not to the room"""
    p = pkg()
    fresh = kw.pop("fresh_rng", False)
    scene = FW.room(p, **kw)
    stats = FT.new_stats()
    sums = FT.sums(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(FW.camera(p)), W, H, SPP, SEED, stats=stats, fresh_rng=fresh, **FW.tables(scene))
    sums.setflags(write=False)
    return sums, stats


# ---- the rooms reach what the mode is for ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["stack", "list"])
def test_the_cutout_room_turns_candidates_down_onto_farther_hits_and_onto_misses(walk):
    sums, stats = run(walk=walk)
    assert stats["samples"] == W * H * SPP   # every sample is followed: the twin has no skip
    assert stats["rejected"] >= 100 and stats["then_farther"] >= 100 and stats["then_miss"] >= 100, stats
    assert stats["rejected_quad"] >= 100 and stats["rejected_tri_uv"] >= 100 and stats["rejected_tri_plain"] >= 100, stats   # all three sources of (u, v)
    assert stats["fog_hits"] == 0 and stats["medium_draws"] == 0
    assert 0 < (sums[..., 7] > 0).mean() < 1


@pytest.mark.parametrize("walk", ["stack", "list"])
def test_the_fog_room_ends_first_hits_inside_the_medium_and_lets_others_through(walk):
    sums, stats = run(walk=walk, masks=False, fog=True)
    assert stats["samples"] == W * H * SPP
    assert stats["fog_hits"] >= 100 and stats["through_fog"] >= 100, stats
    assert stats["medium_hits"] >= stats["fog_hits"]   # a medium's hit may still lose to a nearer surface tested later
    fog = np.array(FW.FOG_ALBEDO, F)
    whole = np.zeros(3, F)
    for _ in range(SPP):
        whole = (whole + fog).astype(F)
    deep = (sums[..., 4:7] == whole).all(axis=2)   # pixels whose every sample ended in the fog: its albedo and the constant normal, SPP times over
    assert deep.sum() >= 1 and (sums[deep][:, 0:3] == np.array([SPP, 0, 0], F)).all() and (sums[deep][:, 7] == SPP).all()


def test_the_mixed_room_does_both():
    _, stats = run(fog=True)
    assert stats["rejected"] >= 100 and stats["then_farther"] >= 100 and stats["then_miss"] >= 100 and stats["fog_hits"] >= 100 and stats["through_fog"] >= 100, stats


def test_one_medium_is_met_alike_in_the_lists_order_and_the_trees():
    """A walk tests every primitive once, and the one medium draws one uniform, the sample's next, whenever it is tested: the first hit depends on the order of the
    tests only where a medium's hit and a surface lie within a rounding of each other.  The list and the stack-walked BVH test in different orders and agree on
    every sample of the fog room; tests/test_gpu_aov_full.py holds the queue and the four-wide walk, which no numpy twin restates, to the same sums."""
    assert bits_equal(run(walk="stack", masks=False, fog=True)[0], run(walk="list", masks=False, fog=True)[0])
    assert bits_equal(run(walk="stack", fog=True)[0], run(walk="list", fog=True)[0])


def test_the_first_hits_differ_from_the_solid_cards():
    holed, solid = run()[0], run(opaque=True)[0]
    differ = (holed.view(np.uint32) != solid.view(np.uint32)).any(axis=2)
    assert differ.sum() > 100, differ.sum()
    assert run(opaque=True)[1]["rejected"] == 0 and run(opaque=True)[1]["tested"] > 1000


def test_texture_coordinates_and_vertex_normals_move_what_they_should():
    base = run()[0]
    assert not bits_equal(base, run(uvs=False)[0])   # the card's mask is looked up elsewhere: other holes
    smooth = run(normals=True)[0]
    assert bits_equal(base[..., 3:8], smooth[..., 3:8]) and not bits_equal(base[..., 0:3], smooth[..., 0:3])   # the normal sum alone


def test_an_rng_taken_from_the_wrong_place_changes_the_fog_rooms_sums():
    """a fresh state of the sample's stream instead of the record's — the state the camera's draws left: the medium draws other uniforms"""
    right, wrong = run(masks=False, fog=True)[0], run(masks=False, fog=True, fresh_rng=True)[0]
    differ = (right.view(np.uint32) != wrong.view(np.uint32)).any(axis=2)
    assert differ.sum() > 100, differ.sum()
    assert bits_equal(run()[0], run(fresh_rng=True)[0])   # without a medium nothing draws, and the place does not matter


def test_the_twin_continues_a_sum_in_sample_order(p):
    scene = FW.room(p, fog=True)
    world, cam, tb = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(FW.camera(p)), FW.tables(scene)
    head = FT.sums(world, cam, W, H, 3, SEED, **tb)
    both = FT.sums(world, cam, W, H, SPP - 3, SEED, first_sample=3, start=head, **tb)
    assert bits_equal(both, run(fog=True)[0])


def test_a_tree_with_a_medium_is_beyond_the_streaming_kernels(p):
    foggy = FW.fog_tree(p)
    assert foggy.getWorldPtr().kind == 2 and foggy.getWorldPtr().n_prims == 9


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_constant_the_argument_check_and_the_enum(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    assert re.search(r"^#define RT_AOV_FULL\s+2u", header, re.M)
    assert (p.capi.AOV_PLAIN, p.capi.AOV_TEXTURED, p.capi.AOV_FULL) == (0, 1, 2)
    params = inspect.signature(p.Renderer.enable_aov).parameters
    assert list(params) == ["self", "max_samples", "textured", "full"] and params["full"].default is False and params["textured"].default is False
    with pytest.raises(ValueError, match="textured and full"):   # refused before the handle is looked at
        p.Renderer.enable_aov(object(), 0, textured=True, full=True)
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert re.search(r"enum class AovMode\s*\{\s*Plain,\s*Textured,\s*Full\s*\}", hpp) and "AovMode::Full ? RT_AOV_FULL" in hpp
    L = p.capi.lib()
    assert L.rt_renderer_aov_enable_mode(None, 0, 2) == 1 and "rt_renderer_aov_enable_mode" in L.rt_last_error().decode()


def test_the_render_tools_choice_of_mode(p):
    c = p.capi
    choose = p.api.feature_mode_for
    plain = [c.MAT_LAMBERTIAN, c.MAT_METAL, c.MAT_DIELECTRIC, c.MAT_LAMBERTIAN_CHECKER, c.MAT_DIFFUSE_LIGHT]
    assert choose(plain, False) == "plain" and choose([], False) == "plain"   # exactly where it chose them before
    assert choose(plain + [c.MAT_LAMBERTIAN_NOISE], False) == "textured" and choose([c.MAT_LAMBERTIAN_IMAGE], False) == "textured"
    assert choose(plain, True) == "full" and choose(plain + [c.MAT_ISOTROPIC], False) == "full"
    assert choose([c.MAT_LAMBERTIAN_IMAGE, c.MAT_ISOTROPIC], False) == "full" and choose([c.MAT_LAMBERTIAN_IMAGE], True) == "full"
    assert choose(np.array([c.MAT_ISOTROPIC], np.uint32), False) == "full"
    tool = open(os.path.join(ROOT, "tools", "render.py")).read()
    assert "p.api.feature_mode_for(kinds, scene.cutouts() is not None)" in tool and 'r.enable_aov(textured=mode == "textured", full=mode == "full")' in tool
