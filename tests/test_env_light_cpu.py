"""Environment light sampling without a GPU: the distribution against float64 mathematics, the rule against its numpy twin bit for bit, the
draw against the density it claims, the whole-sample twin against the older twin and against the plain estimator, the kernel forms against the source, and the
host-side plumbing.  The renderer's own refusals need a device: tests/test_gpu_env_light.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _env_light_twin as LT
import _env_light_worlds as LW
import _env_twin as ET
import _env_worlds as EW
import _tri_worlds as TW
import _kernel_table as KT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg
from _nee_twin import luminance

F = np.float32
SIZE_IDS = [f"{w}x{h}" for w, h in EW.SIZES]
MAPS = [(f"{w}x{h}", (w, h)) for w, h in EW.SIZES] + [("black rows", None)]
SYMBOLS = ["rt_environment_distribution", "rt_environment_sample_batch", "rt_probe_environment_sample", "rt_renderer_kernel_env_light"]


def map_of(size):
    return LW.black_rows_map() if size is None else EW.random_map(*size)


def solid_angles(tables):
    """omega_j of every row, float64, from the stored rowy"""
    rowy = tables["rowy"].astype(np.float64)
    return (2.0 * np.pi / tables["colc"].shape[1]) * (rowy[:-1] - rowy[1:])


# ---- tables against mathematics no kernel shares ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [s for _, s in MAPS], ids=[n for n, _ in MAPS])
def test_tables_against_float64_mathematics(size):
    p = pkg()
    env = map_of(size)
    h, w, _ = env.shape
    t = p.api.environment_distribution(env)
    assert t["rowc"].shape == (h,) and t["rowy"].shape == (h + 1,) and t["colc"].shape == (h, w) and t["density"].shape == (h, w)
    want_rowy = np.cos(np.pi * np.arange(h + 1, dtype=np.float64) / h).astype(F)
    want_rowy[0], want_rowy[h] = 1, -1
    assert bits_equal(t["rowy"], want_rowy)
    assert (np.diff(t["rowy"]) < 0).all()
    assert (np.diff(t["colc"], axis=1) >= 0).all() and (np.diff(t["rowc"]) >= 0).all() and (t["colc"][:, 0] >= 0).all() and t["rowc"][0] >= 0
    # the running sums, restated in float64 (numpy's cumsum adds in order)
    e = env.astype(np.float64)
    hj = t["rowy"].astype(np.float64)[:-1] - t["rowy"].astype(np.float64)[1:]
    wgt = ((0.2126 * e[..., 0] + 0.7152 * e[..., 1]) + 0.0722 * e[..., 2]) * hj[:, None]
    assert bits_equal(t["colc"], np.cumsum(wgt, axis=1).astype(F))
    assert bits_equal(t["rowc"], np.cumsum(np.cumsum(wgt, axis=1)[:, -1]).astype(F))
    omega = solid_angles(t)
    total = float((t["density"].astype(np.float64) * omega[:, None]).sum())
    print(f"{w}x{h}: |sum density omega - 1| = {abs(total - 1):.3e}")
    assert abs(total - 1.0) <= 1e-6
    black = (env == 0).all(axis=2)
    assert (t["density"][black] == 0).all() and (t["density"] >= 0).all() and np.isfinite(t["density"]).all()
    if size is None:
        assert black[5:].all() and (t["density"][5:] == 0).all() and t["rowc"][4] == t["rowc"][7] and (t["colc"][5:] == 0).all()


def test_an_all_black_map_is_refused():
    p = pkg()
    with pytest.raises(p.capi.RtError, match="all black"):
        p.api.environment_distribution(np.zeros((4, 8, 3), F))
    with pytest.raises(p.capi.RtError, match="all black"):
        p.api.environment_sample_batch(np.zeros((1, 1, 3), F), 0.0, np.full((1, 4), 0.5, F))
    with pytest.raises(p.capi.RtError, match="negative"):
        p.api.environment_distribution(np.full((2, 2, 3), -1.0, F))
    with pytest.raises(p.capi.RtError, match=r"\(0, 1\]"):
        p.api.environment_sample_batch(np.ones((2, 2, 3), F), 0.0, np.array([[0.5, 0.5, 0.0, 0.5]], F))
    with pytest.raises(p.capi.RtError, match="u0"):
        p.api.environment_sample_batch(np.ones((2, 2, 3), F), 1.0, np.full((1, 4), 0.5, F))
    d, texel, dens = p.api.environment_sample_batch(np.ones((2, 2, 3), F), 0.0, np.zeros((0, 4), F))
    assert len(d) == len(texel) == len(dens) == 0


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------------------
def rule_inputs(tables):
    return np.concatenate([LW.random_uniforms(100000, seed=5), LW.crafted_uniforms(tables)])


@pytest.mark.parametrize("u0", EW.ROTATIONS, ids=EW.ROTATION_IDS)
@pytest.mark.parametrize("size", [s for _, s in MAPS], ids=[n for n, _ in MAPS])
def test_the_twin_restates_the_rule_bit_for_bit(size, u0):
    p = pkg()
    env = map_of(size)
    h, w, _ = env.shape
    t = p.api.environment_distribution(env)
    u = rule_inputs(t)
    d, texel, dens = p.api.environment_sample_batch(env, u0, u)
    want_d, want_texel = LT.draw(t, u0, u)
    assert np.array_equal(texel, want_texel), f"{int((texel != want_texel).sum())} drawn texels differ"
    assert bits_equal(d, want_d), mismatch_report(d, want_d)
    assert bits_equal(dens, LT.density_of(t, u0, d))
    assert texel.max() < w * h and (t["density"].reshape(-1)[texel] > 0).all()   # a draw never lands on a texel the density calls impossible
    if size is None:
        assert (texel // w < 5).all()   # never in a black row
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- the draw follows the density ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 8), (64, 32)], ids=["16x8", "64x32"])
def test_the_draw_follows_the_density(size):
    p = pkg()
    w, h = size
    env = EW.random_map(w, h)
    t = p.api.environment_distribution(env)
    omega = solid_angles(t)
    prob = (t["density"].astype(np.float64) * omega[:, None]).reshape(-1)
    n = 1000000
    g = env[..., 1].astype(np.float64).reshape(-1)
    want_mean = float((g.reshape(h, w) * omega[:, None]).sum())
    for u0 in (EW.ROTATIONS[0], EW.ROTATIONS[1]):
        u = LW.random_uniforms(n, seed=9 + int(float(u0) * 100))
        d, texel, dens = p.api.environment_sample_batch(env, u0, u)
        counts = np.bincount(texel, minlength=w * h).astype(np.float64)
        bound = 5.0 * np.sqrt(n * prob * (1.0 - prob)) + 1.0
        worst = np.abs(counts - n * prob) / bound
        looked_up = ET.texel_of(w, h, u0, d)
        share = float((looked_up != texel).mean())
        est = g[looked_up] / dens.astype(np.float64)
        se = est.std(ddof=1) / np.sqrt(n)
        print(f"{w}x{h} u0={float(u0)}: worst count deviation / bound = {worst.max():.3f}; lookup != drawn texel in {share:.2e} of the draws; "
              f"mean(g / density) = {est.mean():.6f} +- {se:.6f}, sum g omega = {want_mean:.6f}")
        assert (np.abs(counts - n * prob) <= bound).all(), int(np.argmax(worst))
        assert share <= 1e-4
        assert (dens > 0).all() and abs(est.mean() - want_mean) <= 4.0 * se


# ---- the whole-sample twin ------------------------------------------------------------------------------------------------------------------------------------
def test_the_twin_with_the_mode_off_is_the_environment_twin_bit_for_bit():
    p = pkg()
    scene = EW.sky_room(p)
    env, u0 = scene.environment()
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(EW.camera(p))
    sky = ET.sky_environment(env, u0)
    got, f0 = LT.frame_samples(world, cam, EW.W, EW.H, EW.SPP, EW.DEPTH, EW.SEED, sky)
    want = EW.sky_room_run()
    assert bits_equal(got, want.samples) and np.array_equal(f0, want.followed)
    stats = {}
    counted, f1 = LT.frame_samples(world, cam, EW.W, EW.H, EW.SPP, EW.DEPTH, EW.SEED, sky, stats=stats)   # counting changes no bit
    assert bits_equal(counted, got) and np.array_equal(f0, f1) and stats["light_half"] == 0


def test_the_estimator_is_unbiased_against_the_plain_one():
    """DESIGN §16's check: frame-mean luminance M with its standard error from the per-pixel sample variances, whole frame and the four quadrants:
    |M_on - M_plain| <= 4 sqrt(SE_on^2 + SE_plain^2), the mode on at 256 spp against 4096 plain spp, both by the twin on a 12 x 8 frame of the forms' world."""
    p = pkg()
    w, h, depth = 12, 8, 6
    scene = LW.sky_mesh_room(p)
    env, u0 = scene.environment()
    tables = p.api.environment_distribution(env)
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(EW.camera(p, w, h))
    sky = ET.sky_environment(env, u0)
    stats = {}
    on, followed = LT.frame_samples(world, cam, w, h, 256, depth, EW.SEED, sky, light=(tables, u0), stats=stats)
    assert followed.all() and np.isfinite(on).all()
    plain, followed = ET.frame_samples(world, cam, w, h, 4096, depth, EW.SEED, sky)
    assert followed.all()
    print("the mode-on run exercised:", {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in stats.items()})
    assert stats["light_half"] > 0 and stats["light_half_hit"] > 0 and stats["below_surface"] > 0 and stats["checker_light_half"] > 0

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
    """the forms' world reaches both halves, hits geometry from the map's half and ends paths below the surface; under the sun map the light half goes to the sun"""
    run = LW.run("forms")
    assert run.followed.all()
    assert run.stats["light_half"] > 100 and run.stats["light_half_hit"] > 10 and run.stats["below_surface"] > 10 and run.stats["checker_light_half"] > 10
    sun = LW.run("sun")
    assert sun.followed.all() and sun.stats["light_half"] > 100
    prob = sun.tables["density"].astype(np.float64) * solid_angles(sun.tables)[:, None]
    assert prob[3, 20] > 0.9   # one texel at 1e4 in a sky of 0.05: nearly every draw of the map's half


# ---- forms ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_form_list_is_the_set_of_environment_sampling_instantiations():
    """every form of stream_kernel_for()'s ENV_LIGHT family has a recipe in the list the GPU tests run, and nothing else has"""
    shipped = KT.family("ENV_LIGHT")
    assert len(shipped) == KT.count("ENV_LIGHT") == 8   # (the reader raises on a line of the table it cannot read)
    assert shipped == set(LW.FORMS), shipped ^ set(LW.FORMS)
    assert all(f[2] == 2 for f in shipped) and all(LW.FORMS[f] == TW.FORMS[f] for f in LW.FORMS)
    for family in ("NEE", "TRI", "TRI_NEE", "LIGHT_TREE"):
        assert KT.count(family) == 16   # nothing existing moved


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_bound_and_mirrored():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in p.capi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    assert "#define RT_LIGHT_SAMPLING_ENV 32" in header
    assert "Env = RT_LIGHT_SAMPLING_ENV" in open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert p.api.LIGHT_SAMPLING_MODES["env"] == 32 and p.api.light_sampling_mode("env") == 32 and p.api.light_sampling_mode(32) == 32
    assert {k: v for k, v in p.api.LIGHT_SAMPLING_MODES.items() if k != "env"} == {"off": 0, "quads": 1, "all": 2, "mesh": 4, "tree": 16}
    with pytest.raises(ValueError, match="'env'"):
        p.api.light_sampling_mode("sky")
    assert callable(p.Renderer.kernel_env_light) and callable(p.api.probe_environment_sample)
    assert '"env"' in open(os.path.join(ROOT, "tools", "render.py")).read()


def test_null_handles_are_refused_before_any_device_is_touched():
    p = pkg()
    L = p.lib()
    out = C.c_uint32(7)
    assert L.rt_renderer_kernel_env_light(None, C.byref(out)) != 0 and b"rt_renderer_kernel_env_light" in L.rt_last_error()
    assert L.rt_renderer_light_sampling_enable(None, 32) != 0
    assert L.rt_multi_renderer_light_sampling_enable(None, 32) != 0


def test_c_and_cpp_checks():
    d = os.path.join(ROOT, "tests", "cpp_env_light")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", d])
    assert subprocess.check_output([os.path.join(d, "env_light_abi_check")], text=True).strip() == "env light ABI ok"
    assert os.access(os.path.join(d, "env_light_app"), os.X_OK)   # the program written against rt06.hpp compiles and links; tests/test_gpu_env_light.py runs it
