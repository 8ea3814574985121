"""Sphere lights in light sampling (mode 2) without a GPU: the twin that knows both kinds of light (tests/_nee2_twin.py) is pinned —
off to the oracle, in mode 1 to tests/_nee_twin.py, bit for bit — before anything is compared with it; the estimator it states is shown unbiased
against the oracle's plain path tracer on a sphere-lit and on a mixed room; the host surface (rt_world_lights, the prefab, the symbols) is checked;
and every world of tests/_nee2_worlds.py is held to what it is there for, by the twin's own counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _nee2_twin as T2
import _nee2_worlds as NW2
import _nee_twin as T
import _oracle as O
import _kernel_table as KT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg
from test_light_sampling_cpu import cornell_camera, plain_samples

SEED = 1984
RT_ERR_INVALID = 1
QUADS, ALL = 1, 2


def _world_and_cam(name, W, H):
    """(scene, oracle world, oracle camera, depth) of a world of _nee2_worlds; the world borrows the scene's arrays, so the caller keeps the scene"""
    build, (lookfrom, lookat, vfov), _, _, depth, _ = NW2.WORLDS[name]
    p = pkg()
    scene = build(p)
    return scene, as_oracle_world(scene.getWorldPtr()), as_oracle_camera(p.PinholeCamera(lookfrom, lookat, (0, 1, 0), vfov, W / H)), depth


def test_twin_off_is_the_oracle_and_in_mode_1_is_the_quad_twin_bit_for_bit():
    W = H = 16
    scene = O.Scene.cornell_box()
    cam = cornell_camera(W, H)
    off, followed = T2.frame_samples(scene.world, cam, W, H, 4, 6, SEED, mode=0)
    assert followed.all()
    exp = plain_samples(scene.world, cam, W, H, 4, 6)
    assert bits_equal(off, exp), mismatch_report(off, exp)
    one, _ = T2.frame_samples(scene.world, cam, W, H, 4, 6, SEED, mode=1)
    exp1, _ = T.frame_samples(scene.world, cam, W, H, 4, 6, SEED, light_sampling=True)
    assert bits_equal(one, exp1), mismatch_report(one, exp1)
    two, _ = T2.frame_samples(scene.world, cam, W, H, 4, 6, SEED, mode=2)   # no sphere light: mode 2's table is mode 1's
    assert bits_equal(two, exp1)
    # a room with emitting spheres: off it is still the oracle (orc_trace_batch hits them), and in mode 1 the quad twin, which leaves them unsampled
    for name in ("mixed_room", "sphere_world"):
        keep, w, cam, depth = _world_and_cam(name, 16, 12)
        off, followed = T2.frame_samples(w, cam, 16, 12, 3, depth, SEED, mode=0)
        exp = plain_samples(w, cam, 16, 12, 3, depth)
        assert followed.all() and bits_equal(off, exp), name + ": " + mismatch_report(off, exp)
    keep, w, cam, depth = _world_and_cam("mixed_room", 16, 12)
    one, _ = T2.frame_samples(w, cam, 16, 12, 3, depth, SEED, mode=1)
    exp1, _ = T.frame_samples(w, cam, 16, 12, 3, depth, SEED, light_sampling=True)
    two, _ = T2.frame_samples(w, cam, 16, 12, 3, depth, SEED, mode=2)
    assert bits_equal(one, exp1) and not bits_equal(two, one)


def test_counting_changes_no_bit_of_the_twin():
    keep, w, cam, depth = _world_and_cam("mixed_room", 12, 12)
    plain, f0 = T2.frame_samples(w, cam, 12, 12, 4, depth, SEED, mode=2)
    stats = {}
    counted, f1 = T2.frame_samples(w, cam, 12, 12, 4, depth, SEED, mode=2, stats=stats)
    assert bits_equal(plain, counted) and np.array_equal(f0, f1) and set(stats) == set(T2.new_stats())


def _cornell_lamp(W, H):
    keep = pkg().Scene.cornell_lamp()
    return keep, as_oracle_world(keep.getWorldPtr()), cornell_camera(W, H), 8


# (world, mode-2 samples per pixel, plain samples per pixel).  mixed_room runs at §16's counts (256 against 4096).  The two rooms lit by ONE small, bright, distant
# sphere — the case the mode exists for, and the one where a density that loses the sphere's silhouette to rounding shows as a frame that is too bright — run
# at four times both counts, where four standard errors of the frame mean are 0.8 % (lamp_room) and 1.4 % (cornell_lamp) of it.
UNBIASED = {"lamp_room": (1024, 16384), "mixed_room": (256, 4096), "cornell_lamp": (1024, 16384)}


@pytest.mark.parametrize("name", list(UNBIASED))
def test_mode_2_is_unbiased_against_the_plain_path_tracer(name):
    """§16's rule: frame-mean luminance M with its standard error from the per-pixel sample variances, whole frame and the four quadrants:
    |M_on - M_plain| <= 4 sqrt(SE_on^2 + SE_plain^2), mode 2 (the twin) against plain samples (the oracle), 24 x 24, depth 8.
    Measured |diff| / bound, frame and worst quadrant: lamp_room 0.16, 0.19; cornell_lamp 0.38, 0.58."""
    W = H = 24
    spp_on, spp_plain = UNBIASED[name]
    keep, w, cam, depth = _cornell_lamp(W, H) if name == "cornell_lamp" else _world_and_cam(name, W, H)
    on, followed = T2.frame_samples(w, cam, W, H, spp_on, depth, SEED, mode=2)
    assert followed.all() and np.isfinite(on).all()
    plain = plain_samples(w, cam, W, H, spp_plain, depth)

    def mean_and_se(samples, rows, cols):
        y = T.luminance(samples[rows, cols].astype(np.float64))
        n = y.shape[2]
        return y.mean(), np.sqrt((y.var(axis=2, ddof=1) / n).sum()) / (y.shape[0] * y.shape[1])

    regions = {"frame": (slice(0, H), slice(0, W))}
    for qy in (0, 1):
        for qx in (0, 1):
            regions[f"quadrant {qy}{qx}"] = (slice(qy * H // 2, (qy + 1) * H // 2), slice(qx * W // 2, (qx + 1) * W // 2))
    for region, (rows, cols) in regions.items():
        m_on, se_on = mean_and_se(on, rows, cols)
        m_pl, se_pl = mean_and_se(plain, rows, cols)
        print(f"{name} {region}: mode 2 {m_on:.5f} +- {se_on:.5f}   plain {m_pl:.5f} +- {se_pl:.5f}   |diff| / bound = {abs(m_on - m_pl) / (4 * np.hypot(se_on, se_pl)):.3f}")
        assert m_pl > 0.01
        assert abs(m_on - m_pl) <= 4.0 * np.hypot(se_on, se_pl), region
    # what the estimator is for: per sample, the frame mean is the better known one
    assert mean_and_se(on, *regions["frame"])[1] ** 2 * spp_on < mean_and_se(plain, *regions["frame"])[1] ** 2 * spp_plain


def test_symbols_are_declared_exported_bound_and_mirrored():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in ("rt_world_lights", "rt_scene_cornell_lamp"):
        assert name in declared and name in p.capi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    for define in ("RT_LIGHT_SAMPLING_OFF 0", "RT_LIGHT_SAMPLING_QUADS 1", "RT_LIGHT_SAMPLING_ALL 2", "RT_LIGHT_QUAD 0", "RT_LIGHT_SPHERE 1"):
        assert "#define " + define in header
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert "void SetLightSampling(LightSampling mode)" in hpp and "void SetLightSampling(bool on)" in hpp and "All = RT_LIGHT_SAMPLING_ALL" in hpp
    assert callable(p.Scene.cornell_lamp) and callable(p.Renderer.light_sampling_mode)
    assert [p.api.light_sampling_mode(v) for v in (False, True, 0, 1, 2, "off", "quads", "all")] == [0, 1, 0, 1, 2, 0, 1, 2]
    with pytest.raises(ValueError):
        p.api.light_sampling_mode("spheres")
    render = open(os.path.join(ROOT, "tools", "render.py")).read()
    assert "--light-sampling-mode" in render and "cornell_lamp" in render and '"--light-sampling"' in render
    assert "--mode" in open(os.path.join(ROOT, "tools", "light_sampling_cost.py")).read()


def test_stream_kernel_table_gains_no_instantiation():
    assert KT.count("NEE") == 16


def _lights(p, world, mode):
    kind, index, area, n = (C.c_uint32 * 16)(), (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32(77)
    rc = p.lib().rt_world_lights(C.byref(world), mode, kind, index, area, C.byref(n))
    return rc, n.value, list(kind)[: n.value], list(index)[: n.value], np.array(list(area)[: n.value], np.float32), p.lib().rt_last_error().decode()


def _twin_lights(world, mode):
    return T2.lights_of(*T2.world_arrays(as_oracle_world(world)), mode)


def test_light_table_lists_quads_first_then_static_sphere_lights_in_primitive_order():
    p = pkg()
    s = p.Scene()
    white, light = s.Lambertian((0.7, 0.7, 0.7)), s.DiffuseLight((4, 4, 4))
    rng = np.random.default_rng(5)
    for m in (white, light, white, light):
        s.MakeQuad(rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3), m)
    radii = {}
    for i, m in enumerate((light, white, light, light, white, light)):
        c = rng.standard_normal(3) * 4
        radii[s.MakeSphere(c, 0.3 + 0.17 * i, m)] = 0.3 + 0.17 * i
    s.MakeMovingSphere((9, 0, 0), (9, 1, 0), 0.5, light)      # moving: emits, in no table
    s.MakeSphere((0, 9, 0), -0.6, light)                      # negative radius: not a sphere light
    s.BuildBVH_SAH()
    w = s.getWorldPtr()
    rc, n, kind, index, area, _ = _lights(p, w, ALL)
    assert rc == 0 and n == 6 and kind == [0, 0, 1, 1, 1, 1]
    assert index[:2] == sorted(index[:2]) and index[2:] == sorted(index[2:])   # each kind in the order of the flat world's arrays (a builder may have permuted them)
    t_kind, t_index, t_area = _twin_lights(w, ALL)
    assert list(t_kind) == kind and list(t_index) == index and bits_equal(t_area, area)
    _, prims, _ = s.arrays()
    for i, a in zip(index[2:], area[2:]):
        r = np.float32(prims["radius"][i])
        assert r > 0 and not (int(prims["mat"][i]) & 0x80000000) and a == (np.float32(12.566371) * r) * r
    assert len(set(area.tolist())) == 6
    # mode 1 through the same entry point is rt_world_quad_lights: same order, same areas, and the head of mode 2's list
    rc1, n1, kind1, index1, area1, _ = _lights(p, w, QUADS)
    quad, qarea, qn = (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32()
    assert p.lib().rt_world_quad_lights(C.byref(w), quad, qarea, C.byref(qn)) == 0
    assert rc1 == 0 and n1 == qn.value == 2 and kind1 == [0, 0] and index1 == list(quad)[:2] == index[:2]
    assert bits_equal(area1, np.array(list(qarea)[:2], np.float32)) and bits_equal(area1, area[:2])
    # the prefab: one sphere light of radius 40, no quad light
    lamp = p.Scene.cornell_lamp()
    rc, n, kind, index, area, _ = _lights(p, lamp.getWorldPtr(), ALL)
    assert rc == 0 and n == 1 and kind == [1] and area[0] == (np.float32(12.566371) * np.float32(40)) * np.float32(40)
    _, prims, mats = lamp.arrays()
    assert list(prims["c0"][index[0]]) == [278, 470, 278] and prims["radius"][index[0]] == 40 and len(lamp.quads()) == 17
    assert list(mats["albedo"][prims["mat"][index[0]]]) == [40, 40, 40]
    box_quads = p.Scene.cornell_box().quads()
    assert len(box_quads) == 18 and sorted(map(bytes, lamp.quads()["Q"])) == sorted(bytes(q) for q, m in zip(box_quads["Q"], box_quads["mat"]) if m != 3)


def test_refusals_of_mode_2_and_what_mode_1_still_says():
    p = pkg()

    def room(n_quad_lights=0, n_sphere_lights=0, medium=False, traversal=0):
        s = p.Scene()
        white, light = s.Lambertian((0.7, 0.7, 0.7)), s.DiffuseLight((4, 4, 4))
        s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 0, 1), white)
        for i in range(n_quad_lights):
            s.MakeQuad((i, 2, 0), (0.5, 0, 0), (0, 0, 0.5), light)
        for i in range(n_sphere_lights):
            s.MakeSphere((i, 1, 0), 0.2, light)
        if medium:
            s.MakeConstantMedium((0, 1, 0), 0.5, 0.2, (1, 1, 1))
        s.BuildBVH_TopDown()
        if traversal:
            s.set_traversal(traversal)
        return s

    cases = [(room(), ALL, "no light to sample"), (p.Scene.three_spheres(), ALL, "no light to sample"), (room(9, 8), ALL, "more than 16 lights"),
             (room(17), ALL, "more than 16 lights"), (room(0, 17), ALL, "more than 16 lights"),
             (room(0, 1, traversal=1), ALL, "queue or wide4 traversal"), (room(0, 1, traversal=2), ALL, "queue or wide4 traversal"),
             (room(0, 1, medium=True), ALL, "constant medium"),
             (room(0, 1), QUADS, "no quad light"), (room(17, 1), QUADS, "more than 16 quad lights"), (room(1, 1), 0, "mode must be"), (room(1, 1), 3, "mode must be")]
    for s, mode, cause in cases:
        rc, n, _, _, _, msg = _lights(p, s.getWorldPtr(), mode)
        assert rc == RT_ERR_INVALID and n == 0 and cause in msg, (cause, msg)
    for nq, ns in ((16, 0), (0, 16), (7, 9)):
        keep = room(nq, ns)   # the flat view borrows the scene's arrays: the scene outlives the call
        rc, n, kind, _, _, _ = _lights(p, keep.getWorldPtr(), ALL)
        assert rc == 0 and n == 16 and kind == [0] * nq + [1] * ns
    keep = room(0, 1)
    rc, n, kind, _, _, _ = _lights(p, keep.getWorldPtr(), ALL)   # a sphere-only world: accepted in mode 2
    assert rc == 0 and n == 1 and kind == [1]
    # a list world is taken like a BVH world; a node tree is not extended at all and stays what it was to rt_world_quad_lights
    keep = NW2.lamp_room(p, as_list=True)
    assert _lights(p, keep.getWorldPtr(), ALL)[:3] == (0, 1, [1])
    L = p.lib()
    k, i, a, n = (C.c_uint32 * 16)(), (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32()
    keep = room(1, 1)
    w = keep.getWorldPtr()
    for call in (lambda: L.rt_world_lights(None, ALL, k, i, a, C.byref(n)), lambda: L.rt_world_lights(C.byref(w), ALL, k, i, a, None),
                 lambda: L.rt_scene_cornell_lamp(None), lambda: L.rt_renderer_light_sampling_enable(None, 2), lambda: L.rt_multi_renderer_light_sampling_enable(None, 2)):
        assert call() == RT_ERR_INVALID and b"null" in L.rt_last_error()


@pytest.mark.parametrize("name", NW2.ROOM_WORLDS + NW2.LIST_WORLDS)
def test_room_worlds_are_followed_everywhere_and_reach_both_kinds(name):
    run = NW2.run(name)
    st = run.stats
    print(name, st)
    assert run.followed.all() and st["not_followed"] == 0 and np.isfinite(run.sums).all() and (run.sums[..., :3] > 0).any(axis=2).mean() > 0.9
    w = run.scene.getWorldPtr()
    assert w.kind == (pkg().capi.WORLD_LIST if name.endswith("_list") else pkg().capi.WORLD_BVH)
    rc, n, kind, _, _, _ = _lights(pkg(), w, ALL)
    assert rc == 0 and n == run.lights and st["light_samples"][:n].min() > 0 and st["light_samples"][n:].sum() == 0
    assert st["both_roots"] > 0 and st["far_side_sample"] > 0 and st["below_surface"] > 0 and st["checker_light_half"] > 0
    assert st["sphere_light_half"] == st["light_samples"][[k == 1 for k in kind] + [False] * (16 - n)].sum()
    if name.startswith("lamp_room"):
        assert w.n_quads == 6 and kind == [1] and _lights(pkg(), w, QUADS)[0] == RT_ERR_INVALID
    if name.startswith("mixed_room"):
        assert kind == [0, 1] and st["sphere_and_other"] > 0 and _lights(pkg(), w, QUADS)[1] == 1
        _, prims, mats = run.scene.arrays()
        assert sum(1 for pr in prims if mats["type"][pr["mat"] & 0x7fffffff] == 4) == 2   # the moving light is there, and in no table
    if name == "sphere_world":
        assert w.n_quads == 0 and kind == [1, 1]


@pytest.mark.parametrize("name", NW2.TEXTURED_WORLDS)
def test_textured_rooms_are_ext_2_worlds_and_leave_pixels_to_the_cross_form_check(name):
    run = NW2.run(name)
    print(name, f"fully followed pixels {run.followed.mean():.3f}", run.stats)
    _, _, mats = run.scene.arrays()
    assert {pkg().capi.MAT_LAMBERTIAN_NOISE, pkg().capi.MAT_LAMBERTIAN_IMAGE} <= set(mats["type"].tolist())
    assert 0.5 <= run.followed.mean() < 1.0 and run.stats["not_followed"] > 0 and np.isfinite(run.sums[run.followed]).all()
    assert run.stats["sphere_light_half"] > 0 and run.stats["light_samples"][:2].min() > 0 and run.stats["sphere_and_other"] > 0
    assert _lights(pkg(), run.scene.getWorldPtr(), ALL)[2] == [0, 1]


@pytest.mark.parametrize("name", NW2.EDGE_WORLDS)
def test_edge_worlds_exercise_what_they_are_there_for(name):
    run = NW2.run(name)
    st = run.stats
    print(name, st)
    assert run.followed.all() and st["not_followed"] == 0 and np.isfinite(run.sums).all()
    assert st["light_samples"][:run.lights].min() > 0 and st["light_samples"][run.lights:].sum() == 0
    assert (st["index_clamped"] > 0) == (name == "clamped_sphere_index")
    if name == "far_small_lamp":
        assert st["disc_nonpos_light_half"] > 0 and st["light_half_unmet"] >= st["disc_nonpos_light_half"]   # the drawn point lost on the silhouette: a failed scatter
    if name == "inside_a_light":
        assert st["one_root"] > 0 and st["both_roots"] > 0   # the dome from inside; the small light from outside
    if name == "tangent_light":
        assert st["near_surface"] > 0 and st["disc_nonpos_light_half"] > 0 and st["below_surface"] > 0
    if name == "stacked_sphere_and_quad":
        assert st["sphere_and_other"] > 0 and st["cos_many_lights"] > 0 and st["cos_one_light"] > 0
    if name in ("sixteen_sphere_lights", "clamped_sphere_index"):
        _, _, kind, _, area, _ = _lights(pkg(), run.scene.getWorldPtr(), ALL)
        assert kind == [1] * 16 and len(set(area.tolist())) == 16 and st["checker_light_half"] > 0
