"""The map and the light tree together without a GPU (mode 48): the whole-sample twin against the older twins, the order of its draws on crafted
tapes, the mixture against the sphere's 4 pi, the estimator against the plain one, the kernel forms against the source, and the host-side plumbing.  The
renderer's own refusals need a device: tests/test_gpu_env_tree.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _env_light_twin as LT
import _env_light_worlds as LW
import _env_tree_twin as VT
import _env_tree_worlds as VW
import _env_twin as ET
import _env_worlds as EW
import _tri_worlds as TW
import _kernel_table as KT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, pkg
from _nee2_twin import world_arrays
from _nee_twin import _Tape, dot, luminance

F = np.float32
BELOW_HALF = np.nextafter(F(0.5), F(0))


# ---- the twin is the older twins where they speak ----------------------------------------------------------------------------------------------------------
def test_the_twin_with_the_mode_off_is_the_environment_twin_bit_for_bit():
    p = pkg()
    scene = EW.sky_room(p)
    env, u0 = scene.environment()
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(EW.camera(p))
    got, f0 = VT.frame_samples(world, cam, EW.W, EW.H, EW.SPP, EW.DEPTH, EW.SEED, ET.sky_environment(env, u0))
    want = EW.sky_room_run()
    assert bits_equal(got, want.samples) and np.array_equal(f0, want.followed)


@pytest.mark.parametrize("name", ["forms", "sun"])
def test_the_twin_without_a_table_is_the_environment_light_twin_bit_for_bit(name):
    p = pkg()
    want = LW.run(name)
    world, cam = as_oracle_world(want.scene.getWorldPtr()), as_oracle_camera(EW.camera(p))
    sky = ET.sky_environment(want.env, want.u0)
    stats = {}
    got, followed = VT.frame_samples(world, cam, LW.W, LW.H, LW.SPP, LW.DEPTH, LW.SEED, sky, light=(want.tables, want.u0), stats=stats)
    assert bits_equal(got, want.samples) and np.array_equal(followed, want.followed)
    assert stats["light_half"] == want.stats["light_half"] > 0 and stats["below_surface"] == want.stats["below_surface"]
    assert stats["map_draws"] == stats["table_draws"] == stats["second_draws"] == stats["image_sampled"] == 0
    off, f0 = VT.frame_samples(world, cam, LW.W, LW.H, LW.SPP, LW.DEPTH, LW.SEED, sky)
    want_off, w0 = LT.frame_samples(world, cam, LW.W, LW.H, LW.SPP, LW.DEPTH, LW.SEED, sky)
    assert bits_equal(off, want_off) and np.array_equal(f0, w0)


def test_an_image_hit_is_followed_and_sampled_in_mode_48_only():
    """the forms' room by the twin: with the mode off and in mode 32's estimator an image hit scatters by the cosine lobe alone (no c draw); in mode 48 it draws c"""
    run = VW.run("forms")
    p = pkg()
    cam = as_oracle_camera(VW.camera(p))
    sky = ET.sky_environment(run.env, run.u0)
    blind, followed = VT.frame_samples(run.world, cam, VW.W, VW.H, 2, VW.DEPTH, VW.SEED, sky)
    assert not followed.all()   # without the images the twin leaves material 7 alone, as the older twins do
    for light in (None, (run.tables, run.u0)):
        stats = {}
        got, all_followed = VT.frame_samples(run.world, cam, VW.W, VW.H, 2, VW.DEPTH, VW.SEED, sky, light=light, tex=run.tex, stats=stats)
        assert all_followed.all() and np.isfinite(got).all() and stats["image_sampled"] == 0
        if light is None:   # the samples that met no image are what they were
            assert bits_equal(got[followed], blind[followed])
    assert run.followed.all() and run.stats["image_sampled"] > 100 and run.stats["image_light_half"] > 30


# ---- the order of the draws --------------------------------------------------------------------------------------------------------------------------------
class ListTape:
    """a tape with crafted uniforms: u (rows, k)"""

    def __init__(self, u):
        self.u, self.cur = np.asarray(u, F), np.zeros(len(u), np.int64)

    def next(self, rows):
        out = self.u[rows, self.cur[rows]]
        self.cur[rows] += 1
        return out


def test_the_first_two_draws_pick_the_map_or_the_table_in_the_order_stated():
    u = [[0.25, 0.5, 0.9], [0.25, BELOW_HALF, 0.9], [0.5, 0.1, 0.9], [BELOW_HALF, 0.75, 0.9], [BELOW_HALF, 2.0 ** -24, 0.9], [1.0, 0.1, 0.9]]
    rows = np.arange(len(u))
    tape = ListTape(u)
    to_light, to_env = VT.pick_half(tape, rows, n_l=3)
    assert to_light.tolist() == [True, True, False, True, True, False]      # c < 0.5f; exactly 0.5 is the cosine half
    assert to_env.tolist() == [False, True, False, False, True, False]      # c2 < 0.5f is the map; exactly 0.5 is the table
    assert tape.cur.tolist() == [2, 2, 1, 2, 2, 1]                          # c2 is drawn only behind a c below 0.5
    for n_l in (1, 4096):
        tape = ListTape(u)
        assert VT.pick_half(tape, rows, n_l)[1].tolist() == to_env.tolist() and tape.cur.tolist() == [2, 2, 1, 2, 2, 1]


def test_an_empty_table_makes_no_second_draw():
    u = [[0.25, 0.5, 0.9], [0.25, BELOW_HALF, 0.9], [0.5, 0.1, 0.9], [BELOW_HALF, 0.75, 0.9]]
    tape = ListTape(u)
    to_light, to_env = VT.pick_half(tape, np.arange(len(u)), n_l=0)
    assert to_light.tolist() == to_env.tolist() == [True, True, False, True] and tape.cur.tolist() == [1, 1, 1, 1]
    run = VW.run("n_l=0")
    assert run.tree.n_l == 0 and run.followed.all()
    assert run.stats["second_draws"] == run.stats["table_draws"] == run.stats["tree_leaves"] == 0
    assert run.stats["map_draws"] == run.stats["light_half"] > 100 and run.stats["image_sampled"] > 100   # the map alone, and image hits are still sampled
    assert VW.run("n_l=1").stats["second_draws"] == VW.run("n_l=1").stats["map_draws"] + VW.run("n_l=1").stats["table_draws"] > 100


# ---- the mixture is a density --------------------------------------------------------------------------------------------------------------------------------
class RandomTape(ListTape):
    """uniforms in (0, 1] on the generator's grid of 2^-24, from numpy's generator: as many as are asked for"""
    on_unit3 = _Tape.on_unit3

    def __init__(self, n, seed):
        self.rng, self.cur = np.random.default_rng(seed), np.zeros(n, np.int64)

    def next(self, rows):
        self.cur[rows] += 1
        return ((self.rng.integers(0, 1 << 24, len(rows)) + 1).astype(np.float64) * 2.0 ** -24).astype(F)


@pytest.mark.parametrize("at", [(5.0, 0.5, 5.0), (9.0, 2.0, 2.0)], ids=["under the lamps", "beside them"])
def test_the_mixture_is_a_density(at):
    """E[1 / pm] over directions drawn from pm is the measure of pm's support: the whole sphere, 4 pi, under a map whose every texel has a positive density.
    The map's dynamic range is 8, so 1 / pm <= 2 / pe is bounded and the estimate's variance finite.  The table is the forms' (a quad, a sphere and a triangle
    light); draws are §26's own — pick_half, the map's rule, §20's choice and point — from one point.  A drawn sphere point lost on the silhouette counts 0."""
    p = pkg()
    env = VW.modest_map()
    tables = p.api.environment_distribution(env)
    assert (tables["density"] > 0).all() and tables["density"].max() / tables["density"].min() < 16
    light = (tables, F(0.3))
    world = VW.run("forms").world
    tree = VW.run("forms").tree
    prims, quads, _ = world_arrays(world)
    n = 400000
    tape = RandomTape(n, seed=48)
    rows = np.arange(n)
    to_light, to_env = VT.pick_half(tape, rows, tree.n_l)
    rows, to_env = rows[to_light], to_env[to_light]
    hit_p = np.broadcast_to(np.array(at, F), (len(rows), 3)).copy()
    dd = np.zeros((len(rows), 3), F)
    drawn = np.full(len(rows), -1, np.int64)
    e, t = np.nonzero(to_env)[0], np.nonzero(~to_env)[0]
    dd[e] = LT.draw(tables, light[1], np.stack([tape.next(rows[e]) for _ in range(4)], axis=1))[0]
    drawn[t], dd[t] = VT.table_point(tape, rows[t], tree, prims, quads, hit_p[t])
    with np.errstate(all="ignore"):
        len2 = dot(dd, dd)
        pm, lost = VT.light_density(tree, light, prims, quads, hit_p, dd, len2, np.sqrt(len2), ~to_env, drawn)
    assert (pm > 0).all() and np.isfinite(pm).all()
    est = np.where(lost, 0.0, 1.0 / pm.astype(np.float64))
    se = est.std(ddof=1) / np.sqrt(len(est))
    share = (~to_env).mean()
    print(f"{len(est)} light-half draws, {share:.4f} of them to the table, {int(lost.sum())} lost on a silhouette: mean(1 / pm) = {est.mean():.5f} +- {se:.5f}, "
          f"4 pi = {4 * np.pi:.5f}, ratio {est.mean() / (4 * np.pi):.5f}")
    assert abs(share - 0.5) < 5 * 0.5 / np.sqrt(len(est))
    assert abs(est.mean() - 4.0 * np.pi) <= 5.0 * se


# ---- the expectation is unchanged ----------------------------------------------------------------------------------------------------------------------------
def test_the_estimator_is_unbiased_against_the_plain_one():
    """DESIGN §16's check by tests/test_env_light_cpu.py's recipe and sizes: frame-mean luminance M with its standard error from the per-pixel sample variances,
    whole frame and the four quadrants: |M_on - M_plain| <= 4 sqrt(SE_on^2 + SE_plain^2), mode 48 at 256 spp against 4096 plain spp, both by the twin on a 12 x 8
    frame of a room with a window onto the sky, a quad light, a sphere lamp and an image-textured parallelogram over most of its floor."""
    p = pkg()
    w, h, depth = 12, 8, 6
    scene = VW.window_room(p)
    env, u0 = scene.environment()
    tables = p.api.environment_distribution(env)
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(VW.camera(p, "room", w, h))
    sky = ET.sky_environment(env, u0)
    tex, tree = VW.tex_of(scene), VT.table_of(world)
    assert tree.n_l == 2
    stats = {}
    on, followed = VT.frame_samples(world, cam, w, h, 256, depth, EW.SEED, sky, light=(tables, u0), tree=tree, tex=tex, stats=stats)
    assert followed.all() and np.isfinite(on).all()
    plain, followed = VT.frame_samples(world, cam, w, h, 4096, depth, EW.SEED, sky, tex=tex)
    assert followed.all()
    print("the mode-on run exercised:", {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in stats.items()})
    assert stats["map_draws"] > 0 and stats["table_draws"] > 0 and stats["image_sampled"] > 0 and stats["below_surface"] > 0

    def mean_and_se(samples, rows, cols):
        y = luminance(samples[rows, cols].astype(np.float64))          # (h, w, spp)
        n = y.shape[2]
        return y.mean(), np.sqrt((y.var(axis=2, ddof=1) / n).sum()) / (y.shape[0] * y.shape[1])

    regions = {"frame": (slice(0, h), slice(0, w))}
    for qy in (0, 1):
        for qx in (0, 1):
            regions[f"quadrant {qy}{qx}"] = (slice(qy * h // 2, (qy + 1) * h // 2), slice(qx * w // 2, (qx + 1) * w // 2))
    for name, (rows, cols) in regions.items():
        m_on, se_on = mean_and_se(on, rows, cols)
        m_pl, se_pl = mean_and_se(plain, rows, cols)
        print(f"{name}: on {m_on:.5f} +- {se_on:.5f}   plain {m_pl:.5f} +- {se_pl:.5f}   |diff| / bound = {abs(m_on - m_pl) / (4 * np.hypot(se_on, se_pl)):.3f}")
        assert m_pl > 0.01
        assert abs(m_on - m_pl) <= 4.0 * np.hypot(se_on, se_pl), name


def test_the_gpu_worlds_exercise_what_they_are_there_for():
    forms = VW.run("forms")
    assert forms.followed.all() and forms.tree.n_l == 3
    st = forms.stats
    assert st["map_draws"] > 100 and st["table_draws"] > 100 and (st["table_kinds"] > 20).all() and st["image_sampled"] > 100 and st["below_surface"] > 10
    assert st["second_draws"] == st["map_draws"] + st["table_draws"] and st["checker_light_half"] > 10 and st["tree_leaves"] > st["table_draws"]
    assert VW.run("forms", as_list=True).followed.all()
    for n_l in (0, 1, 2, 65):
        run = VW.run(f"n_l={n_l}")
        assert run.followed.all() and run.tree.n_l == n_l and (run.stats["table_draws"] > 100) == (n_l > 0)
    sil = VW.run("silhouette")
    assert sil.followed.all() and sil.tree.n_l == 1 and sil.stats["sphere_uncredited"] > 0
    sun = VW.run("sun")
    assert sun.followed.all() and sun.stats["map_draws"] > 100 and not bits_equal(sun.samples, forms.samples)
    lamp = VW.run("triangle_lamp")
    assert lamp.followed.all() and lamp.tex is None and lamp.stats["table_kinds"].tolist() == [0, 0, lamp.stats["table_draws"]]


# ---- forms ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_form_list_is_the_set_of_instantiations_and_the_older_counts_stand():
    """every form of stream_kernel_for()'s ENV_TREE family has a recipe in the list the GPU tests run, and nothing else has"""
    shipped = KT.family("ENV_TREE")
    assert len(shipped) == KT.count("ENV_TREE") == 8   # (the reader raises on a line of the table it cannot read)
    assert shipped == set(VW.FORMS) == set(LW.FORMS), shipped ^ set(VW.FORMS)
    assert all(f[2] == 2 for f in shipped) and all(VW.FORMS[f] == TW.FORMS[f] for f in VW.FORMS)
    for family, count in (("NEE", 16), ("TRI", 16), ("TRI_NEE", 16), ("LIGHT_TREE", 16), ("ENV_LIGHT", 8)):
        assert KT.count(family) == count, family   # nothing existing moved


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_mode_is_declared_and_mirrored():
    p = pkg()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    assert "#define RT_LIGHT_SAMPLING_ENV_TREE 48" in header
    assert "EnvTree = RT_LIGHT_SAMPLING_ENV_TREE" in open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert p.api.light_sampling_mode("env+tree") == 48 and p.api.light_sampling_mode(48) == 48 == VW.ENV_TREE == VT.MODE == 16 | 32
    assert p.api.LIGHT_SAMPLING_MODES == {"off": 0, "quads": 1, "all": 2, "mesh": 4, "tree": 16, "env": 32}   # the names of the single modes stand
    with pytest.raises(ValueError, match="'env\\+tree'"):
        p.api.light_sampling_mode("sky+tree")
    assert '"env+tree"' in open(os.path.join(ROOT, "tools", "render.py")).read()
    assert "--env-tree" in open(os.path.join(ROOT, "tools", "fuzz_campaign.py")).read()


def test_null_handles_are_refused_before_any_device_is_touched():
    L = pkg().lib()
    assert L.rt_renderer_light_sampling_enable(None, 48) != 0 and b"rt_renderer_light_sampling_enable" in L.rt_last_error()
    assert L.rt_multi_renderer_light_sampling_enable(None, 48) != 0
    out = C.c_uint32(7)
    assert L.rt_renderer_kernel_env_light(None, C.byref(out)) != 0 and L.rt_renderer_kernel_light_tree(None, C.byref(out)) != 0
