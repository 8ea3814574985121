"""Spheres under maps on the GPU against the whole-sample twin, bit for bit on every pixel.

On a sphere the kernels compute (u, v) from the normal before the normal map bends it and share that (u, v) with the image lookup and the roughness map.  §28 to
§30 judged no frame in which that order matters; tests/_surface_worlds.sphere_room is made of such spheres — a globe with an image, a normal map and a mapped coat,
a mapped rough conductor with a normal map, a mapped coat without one, a frosted ball under the roughness map, a cap around a pole, all inside the coated shell —
and tests/test_surfaces_cpu.py shows without a GPU that its twin follows every sample, takes every way out and tells the two orders apart.  Here all sixteen MFAC
keys and, with the microfacet table taken away, all sixteen NMAP keys render it, plain and in mode 48, and eight random worlds of spheres, parallelograms, triangles
and a mesh under random tables run on an LDS-resident and a global-memory form each.  Frames are 24 x 16 at 8 spp and 16 x 12 at 4 spp, depth 6."""
import numpy as np
import pytest

import _rglass_twin as GT
import _surface_worlds as SW
import _tri_worlds as TW
from _common import bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
FORMS = list(SW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, SW.ENV_TREE]


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def setenv(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def sums_of(r, spp):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, GT.resolve(sums, spp))
    return sums


# ---- 1. sphere_room on the 32 keys ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_sums():
    """(family, mode) -> the sums of the first form rendered: what every later form must repeat on every pixel"""
    return {}


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_renders_sphere_room_as_the_twin_does(p, monkeypatch, first_sums, form, mode):
    """All 16 MFAC keys, each reached by its recipe, under a constant background (plain) or the sky map (mode 48): the sums are the twin's on every pixel, and
    one another's within the mode.  Then the microfacet table is taken away, which leaves the renderer on the NMAP key of the same shape — all 16 of them — with
    the room's four mapped spheres, two of them globes: the twin without records."""
    run = SW.run(bool(mode), as_list=form[0] == TW.LIST)
    assert run.followed.all() and run.unrecorded_followed.all()
    setenv(monkeypatch, TW.FORMS[form][1])
    r = p.Renderer.MakeRenderer(SW.W, SW.H, SW.SPP, SW.DEPTH, SW.camera(p), run.scene.getWorldPtr(), seed=SW.SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    for family, want in (("MFAC", run.sums), ("NMAP", run.unrecorded_sums)):
        if family == "NMAP":
            r.microfacets(None)
        assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), (family, r.kernel_form())
        assert r.kernel_microfacet() == (family == "MFAC") and r.kernel_normal_map() == (family == "NMAP") and r.kernel_triangles()
        assert r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
        assert r.microfacets_info() == {"enabled": family == "MFAC", "records": SW.SPHERE_ROOM_RECORDS if family == "MFAC" else 0}
        assert r.normal_maps_info() == {"enabled": True, "mapped": 4}
        sums = sums_of(r, SW.SPP)
        assert bits_equal(sums, want), (family, mismatch_report(sums, want))
        first = first_sums.setdefault((family, mode), sums)
        assert bits_equal(sums, first), (family, mismatch_report(sums, first))
    r.close()
    assert not bits_equal(run.sums, run.unrecorded_sums)


# ---- 2. random worlds ----------------------------------------------------------------------------------------------------------------------------------------------
MEMORY = {"lds": (TW.LDS, 0, 0), "global": (TW.NARROW, 1, 0)}   # name: (environment, big, wide of a BVH form; a list's global-memory form is also wide)


@pytest.mark.parametrize("memory", list(MEMORY))
@pytest.mark.parametrize("seed", SW.SEEDS)
def test_random_surface_worlds_render_as_the_twin_does(p, monkeypatch, seed, memory):
    """Each seed plain and, where its world carries the sky map, in mode 48 as well, on an LDS-resident and on a global-memory form, exact for even seeds and fast
    for odd ones; a world left a list takes the list forms.  The recipe stands in every message."""
    rr = SW.random_run(seed)
    env, big, wide = MEMORY[memory]
    exact = 1 if rr.as_list else int(seed % 2 == 0)
    form = (TW.LIST, 1, 2, big, big) if rr.as_list else (TW.BVH, exact, 2, big, wide)
    variant = TW.FORMS[form][0]
    assert TW.FORMS[form][1] == env
    setenv(monkeypatch, env)
    for mode, run in ((0, rr.plain), (SW.ENV_TREE, rr.mode48)):
        if run is None:
            continue
        recipe = dict(rr.recipe, mode=mode, memory=memory)
        assert run.followed.all(), recipe
        w = run.scene.getWorldPtr()
        r = p.Renderer.MakeRenderer(SW.RW, SW.RH, SW.RSPP, SW.RDEPTH, run.cam, w, seed=SW.SEED, variant=variant)
        if mode:
            r.light_sampling(mode)
        recipe["kernel"] = r.kernel_form()
        assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), recipe
        recorded = run.mfacs is not None
        assert r.kernel_microfacet() == recorded and r.kernel_normal_map() == (not recorded and run.scene.normal_maps() is not None), recipe
        assert r.kernel_microfacet() or r.kernel_normal_map(), recipe
        sums = sums_of(r, SW.RSPP)
        r.close()
        assert bits_equal(sums, run.sums), f"{recipe}: " + mismatch_report(sums, run.sums)
