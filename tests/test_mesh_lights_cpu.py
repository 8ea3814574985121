"""Triangle and mesh lights in light sampling (mode 4) without a GPU: the host surface (the defines, rt_world_light_table, the mirrors); the
twin that knows the triangle kind of light (tests/_mesh_light_twin.py) pinned to tests/_tri_twin.py — bit for bit in modes 0, 1 and 2, and in mode 4 wherever
no triangle light is in the table — before anything is compared with it; the fold at its edge; the two rules mode 4 adds held to mathematics that no kernel
shares (uniformity over the triangle, the mean of 1 / pl against the solid angle); and every world of tests/_mesh_light_worlds.py held to what it is there for,
by the twin's own counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _mesh_light_twin as MT
import _mesh_light_worlds as MW
import _nee2_worlds as NW2
import _tri_twin as TT
import _tri_worlds as TW
import _kernel_table as KT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

F = np.float32
RT_ERR_INVALID = 1
QUADS, ALL, MESH = 1, 2, 4
QUAD, SPHERE, TRIANGLE = 0, 1, 2


def _table(p, world, mode, capacity=64):
    kind, index, area, n = (C.c_uint32 * max(capacity, 1))(), (C.c_uint32 * max(capacity, 1))(), (C.c_float * max(capacity, 1))(), C.c_uint32(77)
    rc = p.lib().rt_world_light_table(C.byref(world), mode, capacity, kind, index, area, C.byref(n))
    return rc, n.value, list(kind)[: n.value], list(index)[: n.value], np.array(list(area)[: n.value], F), p.lib().rt_last_error().decode()


def _lights(p, world, mode):
    kind, index, area, n = (C.c_uint32 * 16)(), (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32(77)
    rc = p.lib().rt_world_lights(C.byref(world), mode, kind, index, area, C.byref(n))
    return rc, n.value, list(kind)[: n.value], list(index)[: n.value], np.array(list(area)[: n.value], F), p.lib().rt_last_error().decode()


# ---- header and ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_bound_and_mirrored():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    assert "rt_world_light_table" in declared and "rt_world_light_table" in p.capi.SYMBOLS and L.rt_world_light_table.argtypes
    for define in ("RT_LIGHT_SAMPLING_MESH 4", "RT_LIGHT_TRIANGLE 2", "RT_MAX_LIGHTS_MESH 64", "RT_MAX_LIGHTS 16"):
        assert "#define " + define in header
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert "Mesh = RT_LIGHT_SAMPLING_MESH" in hpp and "void SetLightSampling(LightSampling mode)" in hpp
    assert [p.api.light_sampling_mode(v) for v in (False, True, 0, 1, 2, 4, "off", "quads", "all", "mesh")] == [0, 1, 0, 1, 2, 4, 0, 1, 2, 4]
    with pytest.raises(ValueError):
        p.api.light_sampling_mode("triangles")
    assert callable(p.Scene.light_table)
    assert '"mesh"' in open(os.path.join(ROOT, "tools", "render.py")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }" in design and "if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }" in header   # §19 states the rule as rt06.h does


@pytest.mark.parametrize("name", list(NW2.WORLDS))
def test_light_table_is_rt_world_lights_in_modes_1_and_2(name):
    p = pkg()
    scene = NW2.WORLDS[name][0](p)
    w = scene.getWorldPtr()
    for mode in (QUADS, ALL):
        exp = _lights(p, w, mode)
        got = _table(p, w, mode)
        assert got[:4] == exp[:4] and bits_equal(got[4], exp[4]) and (exp[0] == 0 or got[5] == exp[5]), (name, mode, got, exp)
        if exp[0] == 0:
            k, i, a = scene.light_table(mode)
            assert k.tolist() == exp[2] and i.tolist() == exp[3] and bits_equal(a, exp[4])
    rc, n, kind, index, area, _ = _table(p, w, MESH)   # no triangle in these worlds: mode 4's table is mode 2's
    exp = _lights(p, w, ALL)
    assert (rc, n, kind, index) == exp[:4] and bits_equal(area, exp[4])


def test_mode_4_lists_mode_2s_table_then_the_triangle_lights_in_quad_index_order():
    p = pkg()
    s = MW.scene("three_kinds")
    w = s.getWorldPtr()
    rc, n, kind, index, area, _ = _table(p, w, MESH)
    assert rc == 0 and n == 3 and kind == [QUAD, SPHERE, TRIANGLE]
    rc2, n2, kind2, index2, area2, _ = _table(p, w, ALL)
    assert (kind[:2], index[:2]) == (kind2, index2) and bits_equal(area[:2], area2)
    q = s.quads()[index[2]]
    assert q["kind"] == 1 and s.arrays()[2]["type"][q["mat"]] == p.capi.MAT_DIFFUSE_LIGHT
    nrm = TT.cross(q["u"][None, :].astype(F), q["v"][None, :].astype(F))
    assert area[2] == F(0.5) * np.sqrt(TT.dot(nrm, nrm))[0] and abs(area[2] - 4.0) < 1e-5   # the triangle (0.2, 6, 3), (0.2, 8, 5), (0.2, 6, 7): base 4, height 2
    # several triangle lights between triangles that are none: quad-index order, each with its own area; the twin's table is the host's
    for name in ("mesh_lamp", "tetrahedron_lamp", "sixty_four", "triangle_lit", "triangle_lit_list", "plain_lamp"):
        s = MW.scene(name)
        w = s.getWorldPtr()
        rc, n, kind, index, area, _ = _table(p, w, MESH)
        t_kind, t_index, t_area = MT.lights_of(*MT.world_arrays(as_oracle_world(w)), 4)
        assert rc == 0 and n == MW.WORLDS[name][3] and list(t_kind) == kind and list(t_index) == index and bits_equal(t_area, area), name
        tri = [i for i, k in zip(index, kind) if k == TRIANGLE]
        assert tri == sorted(tri) and all(s.quads()["kind"][i] == 1 for i in tri)
        k, i, a = s.light_table("mesh")
        assert k.tolist() == kind and i.tolist() == index and bits_equal(a, area)
    assert len(set(_table(p, MW.scene("sixty_four").getWorldPtr(), MESH)[4].tolist())) == 64   # different areas


def test_sixty_four_lights_are_accepted_and_refusals():
    p = pkg()
    keep64, keep65 = MW.scene("sixty_four"), MW.scene("sixty_five")
    assert _table(p, keep64.getWorldPtr(), MESH)[:2] == (0, 64)
    rc, n, _, _, _, msg = _table(p, keep65.getWorldPtr(), MESH)
    assert rc == RT_ERR_INVALID and n == 0 and "more than 64 lights" in msg
    rc, n, _, _, _, msg = _table(p, keep64.getWorldPtr(), MESH, capacity=63)
    assert rc == RT_ERR_INVALID and n == 0 and "the caller's arrays hold 63" in msg
    keep3 = MW.scene("three_kinds")
    assert _table(p, keep3.getWorldPtr(), MESH, capacity=3)[:2] == (0, 3) and _table(p, keep3.getWorldPtr(), MESH, capacity=2)[0] == RT_ERR_INVALID
    assert _table(p, keep3.getWorldPtr(), ALL, capacity=1)[0] == RT_ERR_INVALID and _table(p, keep3.getWorldPtr(), QUADS, capacity=1)[:2] == (0, 1)
    for mode in (0, 3, 5, 8):
        rc, n, _, _, _, msg = _table(p, keep3.getWorldPtr(), mode)
        assert rc == RT_ERR_INVALID and "mode must be" in msg
    rc, n, _, _, _, msg = _lights(p, keep3.getWorldPtr(), MESH)   # the older query stays what it was
    assert rc == RT_ERR_INVALID and "mode must be" in msg
    s = p.Scene()
    s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), s.Lambertian((0.5, 0.5, 0.5)))
    s.BuildBVH_TopDown()
    rc, n, _, _, _, msg = _table(p, s.getWorldPtr(), MESH)
    assert rc == RT_ERR_INVALID and "no light to sample" in msg
    for traversal, cause in ((1, "queue or wide4 traversal"), (2, "queue or wide4 traversal")):
        t = TW.tri_room(p, tri_light=True, traversal=traversal)
        assert cause in _table(p, t.getWorldPtr(), MESH)[5]
    L = p.lib()
    k, i, a, n = (C.c_uint32 * 64)(), (C.c_uint32 * 64)(), (C.c_float * 64)(), C.c_uint32()
    w = keep3.getWorldPtr()
    for call in (lambda: L.rt_world_light_table(None, MESH, 64, k, i, a, C.byref(n)), lambda: L.rt_world_light_table(C.byref(w), MESH, 64, k, i, a, None),
                 lambda: L.rt_world_light_table(C.byref(w), MESH, 64, None, i, a, C.byref(n))):
        assert call() == RT_ERR_INVALID and b"null" in L.rt_last_error()


def test_stream_kernel_table_gains_no_instantiation():
    assert KT.count("NEE") == 16 and KT.count("TRI_NEE") == 16


# ---- pins -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", [{}, {"as_list": True}, {"lamp": True}, {"lamp": True, "textured": True}], ids=["room", "list", "lamp", "textured"])
def test_without_a_triangle_light_mode_4_is_tri_twins_mode_2_bit_for_bit(room):
    old = TW.run(mode=2, **room)
    cam = as_oracle_camera(old.cam)
    stats = {}
    new, followed = MT.frame_samples(old.world, cam, TW.W, TW.H, TW.SPP, TW.DEPTH, TW.SEED, mode=4, stats=stats)
    assert bits_equal(new[followed], old.samples[followed]), mismatch_report(new[followed], old.samples[followed])
    assert bits_equal(followed.all(axis=2), old.pixel_followed) and stats["tri_light_half"] == 0 and stats["light_samples"].sum() > 0


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("room", [{"lamp": True, "tri_light": True}, {"lamp": True, "tri_light": True, "as_list": True}], ids=["bvh", "list"])
def test_in_modes_0_1_2_the_twin_is_tri_twin_on_triangle_lit_worlds(room, mode):
    old = TW.run(mode=mode, **room)
    new, followed = MT.frame_samples(old.world, as_oracle_camera(old.cam), TW.W, TW.H, TW.SPP, TW.DEPTH, TW.SEED, mode=mode)
    assert followed.all() and bits_equal(new, old.samples), mismatch_report(new, old.samples)


def test_off_the_twin_is_tri_twin_on_a_world_lit_by_triangles_alone():
    run = MW.run("mesh_lamp", 0)
    old, followed = TT.frame_samples(run.world, as_oracle_camera(run.cam), run.W, run.H, run.spp, run.depth, run.seed, mode=0)
    assert followed.all() and bits_equal(run.samples, old)
    assert not bits_equal(run.sums, MW.run("mesh_lamp", 4).sums)   # mode 4 is another sequence of draws


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_fold_is_one_fp32_add_and_a_sum_of_exactly_1_stays():
    Q, u, v = F([1, 2, 3]), F([2, 0, 0]), F([0, 0, 4])
    zero = np.zeros((1, 3), F)

    def at(a, b):
        return (Q + u * F(a)) + v * F(b)

    def point(a, b):
        return MT._tri_point(F([a]), F([b]), Q, u, v, zero)[0]

    assert F(0.25) + F(0.75) == F(1) and bits_equal(point(0.25, 0.75), at(0.25, 0.75))          # a + b exactly 1: not folded
    assert bits_equal(point(0.5, 0.5), at(0.5, 0.5))
    up = F(0.5) + TW.EPS                                                                         # 0.5 + 2^-23: the sum is 1 + 2^-23, one ulp above 1
    assert F(0.5) + up > F(1) and bits_equal(point(0.5, up), at(0.5, F(1) - up)) and F(1) - up == F(0.5) - TW.EPS
    assert not bits_equal(point(0.5, up), at(0.5, up))
    assert bits_equal(point(0.75, 0.75), at(0.25, 0.25))                                         # (0.75, 0.75) lands at (0.25, 0.25)
    assert bits_equal(point(0.25, 0.25), at(0.25, 0.25)) and bits_equal(point(1.0, 1.0), at(0.0, 0.0))
    # a tie of the add: 0.25 + (0.75 + 2^-24) rounds to 1 (to even) and is not folded — the test is the fp32 sum, not the real one
    tie = np.nextafter(F(0.75), F(1))
    assert F(0.25) + tie == F(1) and bits_equal(point(0.25, tie), at(0.25, tie))
    hp = F([[0.5, -1, 2]])
    assert bits_equal(MT._tri_point(F([0.75]), F([0.75]), Q, u, v, hp)[0], at(0.25, 0.25) - hp[0])   # the direction is the point minus hit_p, not normalised


# ---- the estimator's mathematics, through the twin's own _tri_point / _tri_pl ---------------------------------------------------------------------------
# Three vertices and a hit point in front of the triangle.  How thin may the sliver be?  These two tests resolve 5 standard errors of 10^6 draws, about 1e-3 of
# the mean (one standard error: 2e-4).  A drawn point is rounded in fp32 — delta of a few ulp(4) = 5e-7 over (Q + u a) + v b, - hit_p, and the test's own t and
# planar — and the rule gives pl = 0 to a point that rounding put outside its triangle: a boundary layer of about perimeter * delta / area = 4 delta / h of the
# draws, h the short altitude.  For the mathematics, not that layer, to be what is resolved, 4 delta / h stays under one standard error: h >= 4e-6 / 2e-4 = 0.02.
# "sliver" has h = 0.03 on edges of 3.2 (100 : 1).  "thin_sliver" (h = 2e-3, the 1e-3 aspect tools/fuzz_campaign.py draws) is past that line on purpose: it is
# held to the bound that counts the layer (test_a_thin_slivers_deficit_is_its_lost_boundary_layer), not to 5 standard errors.
TRIANGLES = {
    "axis_aligned": (((0, 0, 0), (2, 0, 0), (0, 0, 3)), (0.7, -2.0, 0.9)),
    "sliver": (((1, 1, 1), (4, 1.5, 2), (4.03, 1.5, 2.015)), (2.5, 3.0, 0.5)),
    "oblique": (((-1, 0.5, 2), (1.5, 2.0, 3.5), (0.2, -1.0, 4.0)), (0.3, 1.2, -1.0)),
}
THIN_SLIVER = (((1, 1, 1), (4, 1.5, 2), (4.002, 1.5, 2.001)), (2.5, 3.0, 0.5))
N_DRAWS = 10 ** 6
SUB = np.array([[0.1, 0.1], [0.7, 0.2], [0.2, 0.5]])   # a sub-triangle in the (a, b) frame of the triangle, neither symmetric in a and b nor touching the fold line


def _record(p, name):
    (a, b, c), hit_p = THIN_SLIVER if name == "thin_sliver" else TRIANGLES[name]
    s = p.Scene()
    s.MakeTriangle(a, b, c, s.DiffuseLight((1, 1, 1)))
    s.MakeHittableList()
    q = s.quads()[0]
    assert q["kind"] == 1
    return q, F([hit_p])


def _draws(name):
    rng = np.random.default_rng(sorted(list(TRIANGLES) + ["thin_sliver"]).index(name) + 19)
    return rng.random(N_DRAWS, dtype=F), rng.random(N_DRAWS, dtype=F)


@pytest.mark.parametrize("name", list(TRIANGLES))
def test_drawn_points_are_uniform_over_the_triangle(name):
    """the share of points inside a fixed sub-triangle equals its share of the area within 5 binomial standard errors"""
    q, hit_p = _record(pkg(), name)
    a, b = _draws(name)
    d = MT._tri_point(a, b, q["Q"], q["u"], q["v"], np.broadcast_to(hit_p, (N_DRAWS, 3)))
    pts = (d.astype(np.float64) + hit_p.astype(np.float64)) - q["Q"].astype(np.float64)
    basis = np.stack([q["u"], q["v"]], axis=1).astype(np.float64)           # the point's coordinates in (u, v): least squares in float64
    ab = np.linalg.lstsq(basis, pts.T, rcond=None)[0].T
    n64 = np.cross(q["u"].astype(np.float64), q["v"].astype(np.float64))
    edges = [q["u"].astype(np.float64), q["v"].astype(np.float64), q["v"].astype(np.float64) - q["u"].astype(np.float64)]
    h = np.linalg.norm(n64) / max(np.linalg.norm(e) for e in edges)         # the short altitude
    tol = 8 * np.spacing(F(4)) / h                                          # a few ulp of the coordinates, in units of (a, b)
    assert (ab.min() > -tol) and ((ab[:, 0] + ab[:, 1]).max() < 1 + tol)    # every point is a point of the triangle
    e1, e2 = SUB[1] - SUB[0], SUB[2] - SUB[0]
    det = e1[0] * e2[1] - e1[1] * e2[0]
    share = abs(det)                                                        # sub-triangle area / triangle area: (|det| / 2) / (1 / 2)
    rel = ab - SUB[0]
    s_ = (rel[:, 0] * e2[1] - rel[:, 1] * e2[0]) / det
    t_ = (e1[0] * rel[:, 1] - e1[1] * rel[:, 0]) / det
    inside = (s_ >= 0) & (t_ >= 0) & (s_ + t_ <= 1)
    se = np.sqrt(share * (1 - share) / N_DRAWS)
    print(f"{name}: share inside {inside.mean():.6f}, area share {share:.6f}, |diff| / (5 se) = {abs(inside.mean() - share) / (5 * se):.3f}")
    assert abs(inside.mean() - share) <= 5 * se


def _mean_inverse_density(p, name):
    """(mean of 1 / pl, its standard error, max of 1 / pl, share of draws whose own triangle rejects them, solid angle) over N_DRAWS points of TRIANGLES[name]"""
    verts, hit = THIN_SLIVER if name == "thin_sliver" else TRIANGLES[name]
    q, hit_p = _record(p, name)
    s = p.Scene()
    s.MakeTriangle(*verts, s.DiffuseLight((1, 1, 1)))
    s.MakeHittableList()
    rc, n, kind, _, area, _ = _table(p, s.getWorldPtr(), MESH)   # the area is the table's own
    assert rc == 0 and n == 1 and kind == [TRIANGLE]
    a, b = _draws(name)
    hp = np.ascontiguousarray(np.broadcast_to(hit_p, (N_DRAWS, 3)))
    with np.errstate(all="ignore"):
        d = MT._tri_point(a, b, q["Q"], q["u"], q["v"], hp)
        len2 = TT.dot(d, d)
        pl, thit = MT._tri_pl(q, area[0], hp, d, len2, np.sqrt(len2))
        inv = np.where(thit & (pl > 0), 1.0 / pl.astype(np.float64), 0.0)   # a point that rounding put outside its own triangle has pl = 0 and no weight
    return inv.mean(), inv.std(ddof=1) / np.sqrt(N_DRAWS), inv.max(), (~thit).mean(), _solid_angle(verts, hit)


def _solid_angle(verts, hit_p):
    """Van Oosterom and Strackee (1983), float64"""
    r = [np.array(v, np.float64) - np.array(hit_p, np.float64) for v in verts]
    l = [np.linalg.norm(x) for x in r]
    num = abs(np.dot(r[0], np.cross(r[1], r[2])))
    den = l[0] * l[1] * l[2] + np.dot(r[0], r[1]) * l[2] + np.dot(r[0], r[2]) * l[1] + np.dot(r[1], r[2]) * l[0]
    return 2 * np.arctan2(num, den)


@pytest.mark.parametrize("name", list(TRIANGLES))
def test_the_mean_of_one_over_pl_is_the_solid_angle(name):
    """E[1 / pl] over area-uniform points = the integral of cos / dist^2 over the triangle = its solid angle from the hit point; within 5 standard errors
    of the mean.  area is the table's own (rt_world_light_table), so a wrong area, a wrong fold or a wrong density shows here whatever a kernel does."""
    mean, se, _, missed, omega = _mean_inverse_density(pkg(), name)
    print(f"{name}: mean 1/pl {mean:.6e} +- {se:.2e}, solid angle {omega:.6e}, |diff| / (5 se) = {abs(mean - omega) / (5 * se):.3f}, own point missed {missed:.2e}")
    assert abs(mean - omega) <= 5 * se


def test_a_thin_slivers_deficit_is_its_lost_boundary_layer():
    """a sliver with a short altitude of 2e-3 at coordinates of 4: rounding puts a measurable share of the drawn points outside their own triangle, where the rule
    gives pl = 0 (rt06.h).  What the mean of 1 / pl then lacks is at most that share times the largest 1 / pl, and it cannot exceed the solid angle by more than
    the statistics allow: a bound with the layer counted, from the same draws.  (Measured: 0.196 % of the draws, mean 3.5457e-5 against 3.5518e-5.)"""
    mean, se, largest, missed, omega = _mean_inverse_density(pkg(), "thin_sliver")
    print(f"thin_sliver: mean 1/pl {mean:.6e} +- {se:.2e}, solid angle {omega:.6e}, own point missed {missed:.2e}, allowed deficit {missed * largest + 5 * se:.3e}")
    assert 0 < missed < 0.01 and -5 * se <= omega - mean <= missed * largest + 5 * se


# ---- the worlds -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MW.EDGE_WORLDS + ("triangle_lit_list", "three_kinds_list"))
def test_worlds_exercise_what_they_are_there_for(name):
    run = MW.run(name)
    st = run.stats
    print(name, st)
    assert run.followed and st["not_followed"] == 0 and np.isfinite(run.sums).all() and (run.sums[..., :3] > 0).any(axis=2).mean() > 0.9
    assert st["light_samples"][:run.lights].min() > 0 and st["light_samples"][run.lights:].sum() == 0
    assert st["tri_light_half"] > 0 and 0.3 < st["tri_folded"] / st["tri_light_half"] < 0.7 and st["below_surface"] > 0 and st["checker_light_half"] > 0
    assert (st["index_clamped"] > 0) == (name == "clamped_triangle_index")
    if name.startswith("triangle_lit"):
        assert run.lights == 1 and st["tri_light_half"] == st["light_samples"][0]   # one light: no index draw
    if name.startswith("three_kinds"):
        assert st["sphere_light_half"] > 0 and st["tri_and_other"] > 0 and st["both_roots"] > 0
    if name in ("mesh_lamp", "tetrahedron_lamp"):
        assert st["two_tri_crossings"] > 0.9 * st["tri_light_half"]   # a closed mesh: a direction to a point of it crosses two table entries
    if name in ("sixty_four", "clamped_triangle_index"):
        assert run.lights == 64


@pytest.mark.parametrize("name", ["three_kinds_textured", "three_kinds_textured_list"])
def test_textured_rooms_leave_pixels_to_the_cross_form_check(name):
    run = MW.run(name)
    assert 0.8 < run.pixel_followed.mean() < 1.0 and run.stats["tri_light_half"] > 0 and np.isfinite(run.sums[run.pixel_followed]).all()
