"""Light sampling without a GPU: the numpy twin of a whole sample is pinned to the oracle, the estimator it states is
shown unbiased against the oracle's plain path tracer, and the host surface — symbols, the light table, the worlds it refuses — is checked.
The matrix of kernel forms the GPU tests run (tests/_nee_worlds.py) is held against the instantiations csrc/rt_device.hip lists, and every test
world against what it is there to exercise, by the twin's own counts: a world that stops reaching an edge fails here, before any GPU is needed.

The twin (tests/_nee_twin.py) is what the GPU tests of tests/test_gpu_light_sampling.py compare the kernels with, so the first test here
pins it to orc_radiance_batch with sampling off before anything is compared against it."""
import ctypes as C
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _nee_twin as T
import _nee_worlds as NW
import _oracle as O
import _kernel_table as KT
from _common import ROOT, as_oracle_world, bits_equal, mismatch_report, pkg

SEED = 1984
SYMBOLS = ["rt_renderer_light_sampling_enable", "rt_renderer_light_sampling_info", "rt_multi_renderer_light_sampling_enable", "rt_world_quad_lights",
           "rt_renderer_kernel_form"]


def cornell_camera(W, H):
    return O.camera_pinhole((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)


def plain_samples(world, cam, W, H, spp, depth):
    """(H, W, spp, 3): the oracle's own per-sample radiance (orc_radiance_batch), the pixels cut into strips over a few threads"""
    keys = np.stack([np.repeat(np.arange(W * H, dtype=np.uint32), spp), np.tile(np.arange(spp, dtype=np.uint32), W * H)], axis=1)
    out = np.zeros((W * H * spp, 3), np.float32)
    strips = np.array_split(np.arange(len(keys)), 16)

    def run(idx):
        k, o = np.ascontiguousarray(keys[idx]), np.zeros((len(idx), 3), np.float32)
        assert O.lib().orc_radiance_batch(C.byref(world), C.byref(cam), W, H, depth, SEED, len(k), k, o) == 0
        out[idx] = o

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(run, strips))
    return out.reshape(H, W, spp, 3)


def test_twin_without_sampling_is_the_oracle_bit_for_bit():
    W = H = 16
    scene = O.Scene.cornell_box()
    cam = cornell_camera(W, H)
    got, followed = T.frame_samples(scene.world, cam, W, H, 4, 6, SEED, light_sampling=False)
    assert followed.all()
    exp = plain_samples(scene.world, cam, W, H, 4, 6)
    assert bits_equal(got, exp), mismatch_report(got, exp)
    assert 0.005 < (exp > 0).any(axis=3).mean() < 0.5   # small light: few plain paths find it, but some do


def test_twin_without_sampling_follows_spheres_metal_and_checker_like_the_oracle():
    """the rest of the twin's scope: sphere normals, metal reflection with fuzz, the checker texture, the sky"""
    p = pkg()
    s = p.Scene()
    ground = s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 10.0)
    s.MakeSphere((0, -100.5, -1), 100.0, ground)
    s.MakeSphere((0, 0, -1), 0.5, s.Lambertian((0.1, 0.2, 0.5)))
    s.MakeSphere((1, 0, -1), 0.5, s.Metal((0.8, 0.6, 0.2), 0.3))
    s.MakeQuad((-2, -0.5, -3), (4, 0, 0), (0, 2, 0), s.Metal((0.9, 0.9, 0.9), 0.0))
    s.BuildBVH_TopDown()
    W, H = 24, 16
    w = as_oracle_world(s.getWorldPtr())
    cam = O.camera_pinhole((0, 0, 0.5), (0, 0, -1), (0, 1, 0), 90.0, W / H)
    got, followed = T.frame_samples(w, cam, W, H, 3, 10, SEED, light_sampling=False)
    assert followed.all()
    exp = plain_samples(w, cam, W, H, 3, 10)
    assert bits_equal(got, exp), mismatch_report(got, exp)


def test_estimator_is_unbiased_against_the_plain_path_tracer():
    """Frame-mean luminance M with its standard error from the per-pixel sample variances, whole frame and the four quadrants:
    |M_on - M_plain| <= 4 sqrt(SE_on^2 + SE_plain^2), sampling on at 256 spp (the twin) against 4096 plain spp (the oracle)."""
    W = H = 24
    depth = 8
    scene = O.Scene.cornell_box()
    cam = cornell_camera(W, H)
    on, followed = T.frame_samples(scene.world, cam, W, H, 256, depth, SEED, light_sampling=True)
    assert followed.all() and np.isfinite(on).all()
    plain = plain_samples(scene.world, cam, W, H, 4096, depth)

    def mean_and_se(samples, rows, cols):
        y = T.luminance(samples[rows, cols].astype(np.float64))          # (h, w, spp)
        n = y.shape[2]
        per_pixel_var_of_mean = y.var(axis=2, ddof=1) / n
        return y.mean(), np.sqrt(per_pixel_var_of_mean.sum()) / (y.shape[0] * y.shape[1])

    regions = {"frame": (slice(0, H), slice(0, W))}
    for qy in (0, 1):
        for qx in (0, 1):
            regions[f"quadrant {qy}{qx}"] = (slice(qy * H // 2, (qy + 1) * H // 2), slice(qx * W // 2, (qx + 1) * W // 2))
    for name, (rows, cols) in regions.items():
        m_on, se_on = mean_and_se(on, rows, cols)
        m_pl, se_pl = mean_and_se(plain, rows, cols)
        print(f"{name}: on {m_on:.5f} +- {se_on:.5f}   plain {m_pl:.5f} +- {se_pl:.5f}   |diff| / bound = {abs(m_on - m_pl) / (4 * np.hypot(se_on, se_pl)):.3f}")
        assert m_pl > 0.01
        assert abs(m_on - m_pl) <= 4.0 * np.hypot(se_on, se_pl), name
    # what the estimator is for: per sample, the frame mean is the better known one (SE^2 * samples is the variance one sample brings)
    assert mean_and_se(on, *regions["frame"])[1] ** 2 * 256 < mean_and_se(plain, *regions["frame"])[1] ** 2 * 4096


def test_symbols_are_declared_exported_bound_and_mirrored():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, f"include/rt06.h does not declare {name}"
        assert name in p.capi.SYMBOLS
        assert hasattr(L, name), f"librt06.so does not export {name}"
        assert getattr(L, name).argtypes, f"capi.py gives {name} no signature"
    assert "RT_MAX_LIGHTS 16" in header
    assert "void SetLightSampling(bool on)" in open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert callable(p.Renderer.kernel_form) and all(f"#define RT_KERNEL_{k}" in header for k in ("BASELINE 0", "STREAM 1", "XCHG 2"))
    assert callable(p.Renderer.light_sampling) and callable(p.Renderer.light_sampling_info) and callable(p.MultiRenderer.light_sampling)
    assert "--light-sampling" in open(os.path.join(ROOT, "tools", "render.py")).read()


def test_form_matrix_is_the_set_of_light_sampling_instantiations():
    """every form of stream_kernel_for()'s NEE family has a recipe in the matrix the GPU tests run, and nothing else has"""
    shipped = KT.family("NEE")
    assert len(shipped) == KT.count("NEE") == 16   # (the reader raises on a line of the table it cannot read)
    assert shipped == set(NW.FORMS), shipped ^ set(NW.FORMS)
    assert len({NW.form_id(f) for f in NW.FORMS}) == len(NW.FORMS)
    assert all(name in NW.MATRIX_WORLDS for name, _, _ in NW.FORMS.values())


def test_counting_changes_no_bit_of_the_twin():
    scene = O.Scene.cornell_box()
    cam = cornell_camera(12, 12)
    plain, f0 = T.frame_samples(scene.world, cam, 12, 12, 4, 6, SEED, light_sampling=True)
    stats = {}
    counted, f1 = T.frame_samples(scene.world, cam, 12, 12, 4, 6, SEED, light_sampling=True, stats=stats)
    assert bits_equal(plain, counted) and np.array_equal(f0, f1)
    assert set(stats) == set(T.new_stats()) and stats["light_samples"][0] > 0 and stats["light_samples"][1:].sum() == 0 and stats["not_followed"] == 0


@pytest.mark.parametrize("name", NW.MATRIX_WORLDS + ("irregular_room",))
def test_matrix_worlds_are_mostly_followed_and_leave_pixels_to_the_cross_form_check(name):
    run = NW.run(name)
    print(name, f"fully followed pixels {run.followed.mean():.3f}", run.stats)
    assert run.scene.getWorldPtr().kind == (pkg().capi.WORLD_LIST if name.endswith("_list") else pkg().capi.WORLD_BVH)
    assert 0.5 <= run.followed.mean() < 1.0   # the dielectric (and the noise and image materials) are in view; elsewhere the twin goes all the way
    assert run.stats["not_followed"] > 0 and np.isfinite(run.sums[run.followed]).all()
    assert run.stats["light_samples"][:run.lights].min() > 0 and run.stats["light_samples"][run.lights:].sum() == 0
    assert run.stats["checker_light_half"] > 0 and run.stats["below_surface"] > 0
    quad, area, n = (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32()
    assert pkg().lib().rt_world_quad_lights(C.byref(run.scene.getWorldPtr()), quad, area, C.byref(n)) == 0 and n.value == run.lights
    if "textured" in name:   # what makes it an EXT = 2 world, and the twin leaves more samples unfollowed for it
        _, _, mats = run.scene.arrays()
        assert {pkg().capi.MAT_LAMBERTIAN_NOISE, pkg().capi.MAT_LAMBERTIAN_IMAGE} <= set(mats["type"].tolist())
        assert run.stats["not_followed"] > NW.run(name.replace("textured_", "")).stats["not_followed"]


@pytest.mark.parametrize("name", NW.EDGE_WORLDS)
def test_edge_worlds_exercise_what_they_are_there_for(name):
    run = NW.run(name)
    st = run.stats
    print(name, st)
    assert run.followed.all() and st["not_followed"] == 0 and np.isfinite(run.sums).all()
    assert st["light_samples"][:run.lights].min() > 0 and st["light_samples"][run.lights:].sum() == 0   # every light index receives a sample
    assert (st["index_clamped"] > 0) == (name == "clamped_index")   # one draw in 2^24: only the world whose seed was searched for it has one
    if name in ("sixteen_lights", "clamped_index"):
        assert run.lights == T.MAX_LIGHTS and st["checker_light_half"] > 0
        quads = run.scene.quads()
        _, _, mats = run.scene.arrays()
        _, areas = T.quad_lights(quads, mats)
        assert len(set(areas.tolist())) == 16   # different sizes: a wrong light's area changes the weight
    if name == "stacked_lights":
        assert st["cos_many_lights"] > 0 and st["cos_one_light"] > 0 and st["checker_light_half"] > 0
    if name == "lights_behind":
        assert st["below_surface"] > 0 and st["light_half_unmet"] > 0


def _lights(p, world):
    quad, area, n = (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32(77)
    rc = p.lib().rt_world_quad_lights(C.byref(world), quad, area, C.byref(n))
    return rc, n.value, list(quad)[: n.value], np.array(list(area)[: n.value], np.float32), p.lib().rt_last_error().decode()


def test_light_table_of_the_cornell_box_and_of_two_lights():
    p = pkg()
    s = p.Scene.cornell_box()
    w = s.getWorldPtr()
    rc, n, quad, area, _ = _lights(p, w)
    assert rc == 0 and n == 1 and area[0] == np.float32(130 * 105)
    ow = as_oracle_world(w)
    quads = np.frombuffer((C.c_char * (ow.n_quads * O.QUAD_DT.itemsize)).from_address(ow.quads), O.QUAD_DT)
    mats = np.frombuffer((C.c_char * (ow.n_materials * O.MAT_DT.itemsize)).from_address(ow.materials), O.MAT_DT)
    t_idx, t_area = T.quad_lights(quads, mats)
    assert list(t_idx) == quad and bits_equal(t_area, area)
    # skew lights between other quads: index order, areas with the twin's bits
    s = p.Scene()
    white, light = s.Lambertian((0.7, 0.7, 0.7)), s.DiffuseLight((4, 4, 4))
    rng = np.random.default_rng(3)
    kinds = [white, light, white, light, light, white]
    for m in kinds:
        s.MakeQuad(rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3), m)
    s.MakeSphere((0, 0, 0), 1.0, light)   # a sphere light emits but is not in the table
    s.BuildBVH_SAH()
    w = s.getWorldPtr()
    rc, n, quad, area, _ = _lights(p, w)
    assert rc == 0 and n == 3 and quad == sorted(quad)   # in the order of the flat world's quads (a builder may have permuted them)
    ow = as_oracle_world(w)
    quads = np.frombuffer((C.c_char * (ow.n_quads * O.QUAD_DT.itemsize)).from_address(ow.quads), O.QUAD_DT)
    mats = np.frombuffer((C.c_char * (ow.n_materials * O.MAT_DT.itemsize)).from_address(ow.materials), O.MAT_DT)
    t_idx, t_area = T.quad_lights(quads, mats)
    assert list(t_idx) == quad and bits_equal(t_area, area)


def test_worlds_without_a_light_sampling_form_are_refused_with_their_cause():
    p = pkg()
    RT_ERR_INVALID = 1

    def room(n_lights, medium=False, traversal=0, sphere_light=False):
        s = p.Scene()
        white, light = s.Lambertian((0.7, 0.7, 0.7)), s.DiffuseLight((4, 4, 4))
        s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 0, 1), white)
        for i in range(n_lights):
            s.MakeQuad((i, 2, 0), (0.5, 0, 0), (0, 0, 0.5), light)
        if sphere_light:
            s.MakeSphere((0, 1, 0), 0.2, light)
        if medium:
            s.MakeConstantMedium((0, 1, 0), 0.5, 0.2, (1, 1, 1))
        s.BuildBVH_TopDown()
        if traversal:
            s.set_traversal(traversal)
        return s

    cases = [(room(0), "no quad light"), (room(0, sphere_light=True), "no quad light"), (room(17), "more than 16 quad lights"),
             (room(1, traversal=1), "queue or wide4 traversal"), (room(1, traversal=2), "queue or wide4 traversal"),
             (room(1, medium=True), "constant medium"), (p.Scene.three_spheres(), "no quad light")]
    for s, cause in cases:
        rc, n, _, _, msg = _lights(p, s.getWorldPtr())
        assert rc == RT_ERR_INVALID and n == 0 and cause in msg, (cause, msg)
    rc, n, _, _, _ = _lights(p, room(16).getWorldPtr())
    assert rc == 0 and n == 16


def test_null_handles_are_refused_before_any_device_is_touched():
    p = pkg()
    L = p.lib()
    out2 = (C.c_uint32 * 2)()
    for call in (lambda: L.rt_renderer_light_sampling_enable(None, 1), lambda: L.rt_renderer_light_sampling_info(None, out2),
                 lambda: L.rt_multi_renderer_light_sampling_enable(None, 1), lambda: L.rt_world_quad_lights(None, (C.c_uint32 * 16)(), (C.c_float * 16)(), C.byref(C.c_uint32()))):
        assert call() == 1   # RT_ERR_INVALID
        assert b"null" in L.rt_last_error()
    with pytest.raises(p.capi.RtError):
        p.Renderer(None, None).light_sampling(True)
