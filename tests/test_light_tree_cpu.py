"""The light tree and the choice by area (mode 16) without a GPU: the host surface (the defines, rt_world_light_table in mode 16,
rt_world_light_tree, the mirrors) against the twin's builder, bit for bit; the refusals; the twin (tests/_light_tree_twin.py) pinned to
tests/_mesh_light_twin.py in modes 0, 1, 2 and 4 before anything is compared with it; THE PIN THAT CARRIES THE PAD — the walk's density against the linear loop
over the same table on 10^6 directions per table, aimed at interiors, vertices, edges, one ulp beside edges and along the axes: equal bit for bit, no light with
pl_j > 0 missed; the mathematics of the choice and of the density through the twin's own functions; the binary search against a linear scan; the kernel table;
and every world of tests/_light_tree_worlds.py held to what it is there for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _light_tree_twin as LT
import _light_tree_worlds as LW
import _mesh_light_twin as MT
import _tri_worlds as TW
import _kernel_table as KT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

F = np.float32
RT_ERR_INVALID = 1
QUAD, SPHERE, TRIANGLE = 0, 1, 2


# ---- header, ABI, mirrors ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_bound_and_mirrored():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for sym in ("rt_world_light_tree", "rt_renderer_kernel_light_tree"):
        assert sym in declared and sym in p.capi.SYMBOLS and getattr(L, sym).argtypes
    for define in ("RT_LIGHT_SAMPLING_TREE 16", "RT_MAX_LIGHTS_TREE 4096", "RT_LIGHT_TREE_PAD 0x1p-10f", "RT_LIGHT_TREE_PAD_SPHERE 0x1p-18f", "RT_LIGHT_TREE_K 0x1.0001p+0f",
                   "RT_LIGHT_SAMPLING_MESH 4", "RT_MAX_LIGHTS_MESH 64", "RT_MAX_LIGHTS 16"):
        assert "#define " + define in header
    assert LT.PAD == F(float.fromhex("0x1p-10")) and LT.PAD_SPHERE == F(float.fromhex("0x1p-18")) and LT.TREE_K == F(float.fromhex("0x1.0001p+0"))
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert "Tree = RT_LIGHT_SAMPLING_TREE" in hpp
    assert [p.api.light_sampling_mode(v) for v in (16, "tree", "mesh", 4, True)] == [16, 16, 4, 4, 1]
    assert callable(p.Scene.light_tree) and callable(p.Renderer.kernel_light_tree)
    assert '"tree"' in open(os.path.join(ROOT, "tools", "render.py")).read()
    assert "--light-tree" in open(os.path.join(ROOT, "tools", "fuzz_campaign.py")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "tmin <= tmax * RT_LIGHT_TREE_K && tmax > 0" in design and "tmin <= tmax * RT_LIGHT_TREE_K && tmax > 0" in header   # §20 states the rule as rt06.h does


# ---- the host's table and tree against the twin's builder -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LW.HOST_WORLDS)
def test_host_table_and_tree_are_the_twins_builder_bit_for_bit(name):
    """1, 2, 3, 20, 65, 82 and 320 lights; a centroid tie; the three kinds mixed; areas 1 : 10^4; worlds without a triangle"""
    s = LW.scene(name)
    t = LT.tree_of(as_oracle_world(s.getWorldPtr()))
    kind, index, area = s.light_table("tree")
    nodes, cdf = s.light_tree()
    assert t.n_l == LW.WORLDS[name][2] == len(kind) and nodes.shape == (2 * t.n_l - 1, 8) and t.refused is None
    assert kind.tolist() == t.kind.tolist() and index.tolist() == t.index.tolist() and bits_equal(area, t.area)
    assert bits_equal(cdf, t.cdf) and bits_equal(nodes, LT.nodes_as_floats(t)), mismatch_report(nodes, LT.nodes_as_floats(t))
    # the table is a permutation of mode 4's, the sum is sequential, the numbering is preorder with leaves in table order
    k4, i4, a4 = MT.lights_of(*MT.world_arrays(as_oracle_world(s.getWorldPtr())), 4)
    assert sorted(zip(k4.tolist(), i4.tolist())) == sorted(zip(kind.tolist(), index.tolist()))
    assert bits_equal(np.array([k4[o] for o in t.order]), np.asarray(t.kind))
    c = F(0)
    for j in range(t.n_l):
        c = F(c + area[j])
        assert c == cdf[j] and (j == 0 or cdf[j] > cdf[j - 1])
    leaves = t.leaf[t.leaf != LT.INNER]
    assert leaves.tolist() == list(range(t.n_l)) and t.skip[0] == t.n_nodes and (t.skip > np.arange(t.n_nodes)).all()
    for i in range(t.n_nodes):   # a subtree's boxes lie in its root's
        assert (t.lo[i + 1:t.skip[i]] >= t.lo[i]).all() and (t.hi[i + 1:t.skip[i]] <= t.hi[i]).all()


def test_the_centroid_tie_keeps_mode_4s_order():
    s = LW.scene("tie")
    kind, index, _ = s.light_table("tree")
    k4, i4, _ = s.light_table("mesh")
    pos = {int(i): n for n, i in enumerate(index)}
    assert i4[0] < i4[1] and pos[int(i4[0])] + 1 == pos[int(i4[1])]   # the coincident pair, adjacent, in quad-index order


def _tree_call(p, world, capacity):
    nodes, cdf, n = (C.c_float * (8 * max(2 * capacity - 1, 1)))(), (C.c_float * max(capacity, 1))(), C.c_uint32(77)
    rc = p.lib().rt_world_light_tree(C.byref(world), capacity, nodes, C.byref(n), cdf)
    return rc, n.value, p.lib().rt_last_error().decode()


def test_refusals():
    p = pkg()
    s = p.Scene()
    emit = s.DiffuseLight((1, 1, 1))
    for i in range(4097):
        x, z = 0.1 * (i % 64), 0.1 * (i // 64)
        s.MakeTriangle((x, 0, z), (x + 0.05, 0, z), (x, 0, z + 0.05), emit)
    s.MakeHittableList()
    with pytest.raises(p.capi.RtError, match="more than 4096 lights"):
        s.light_table("tree")
    with pytest.raises(p.capi.RtError, match="more than 4096 lights"):
        s.light_tree()
    with pytest.raises(p.capi.RtError, match="more than 64 lights"):
        s.light_table("mesh")
    # a light whose area vanishes in the running sum: a 10^4 x 10^4 quad between two triangles of area 1 — the second triangle's c_j is the quad's
    s = p.Scene()
    emit = s.DiffuseLight((1, 1, 1))
    s.MakeQuad((-5000, 0, -5000), (10000, 0, 0), (0, 0, 10000), emit)
    s.MakeTriangle((-9000, 0, 0), (-9000, 0, 2), (-9001, 0, 0), emit)
    s.MakeTriangle((9000, 0, 0), (9000, 0, 2), (9001, 0, 0), emit)
    s.MakeHittableList()
    assert len(s.light_table("mesh")[0]) == 3
    for call in (lambda: s.light_table("tree"), s.light_tree):
        with pytest.raises(p.capi.RtError, match="lost in the fp32 running sum"):
            call()
    assert LT.tree_of(as_oracle_world(s.getWorldPtr())).refused is not None
    s = p.Scene()
    s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), s.Lambertian((0.5, 0.5, 0.5)))
    s.BuildBVH_TopDown()
    with pytest.raises(p.capi.RtError, match="no light to sample"):
        s.light_table("tree")
    for traversal in (1, 2):
        with pytest.raises(p.capi.RtError, match="queue or wide4 traversal"):
            TW.tri_room(p, tri_light=True, traversal=traversal).light_tree()
    three = LW.scene("three_kinds").getWorldPtr()
    assert _tree_call(p, three, 3)[:2] == (0, 5)
    rc, n, msg = _tree_call(p, three, 2)
    assert rc == RT_ERR_INVALID and n == 0 and "the caller's arrays hold 2" in msg
    L = p.lib()
    nodes, cdf, n = (C.c_float * 40)(), (C.c_float * 3)(), C.c_uint32()
    for call in (lambda: L.rt_world_light_tree(None, 3, nodes, C.byref(n), cdf), lambda: L.rt_world_light_tree(C.byref(three), 3, None, C.byref(n), cdf),
                 lambda: L.rt_world_light_tree(C.byref(three), 3, nodes, None, cdf), lambda: L.rt_world_light_tree(C.byref(three), 3, nodes, C.byref(n), None)):
        assert call() == RT_ERR_INVALID and b"null" in L.rt_last_error()


def test_the_kernel_table_has_sixteen_light_tree_forms_with_the_triangle_familys_keys():
    assert KT.count("LIGHT_TREE") == 16
    assert KT.count("NEE") == 16 and KT.count("TRI") == 16 and KT.count("TRI_NEE") == 16
    keys = KT.family("LIGHT_TREE")
    assert keys == set(TW.FORMS) and len(keys) == 16


# ---- the twin, pinned to its elder in the modes both know -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [(n, m) for n in ("three_kinds", "three_kinds_list", "mesh_lamp") for m in (0, 1, 2, 4)
                                       if not (n == "mesh_lamp" and m in (1, 2))])   # a world lit by triangles alone has no table in modes 1 and 2
def test_in_modes_0_1_2_4_the_twin_is_mesh_light_twin_bit_for_bit(name, mode):
    s = LW.scene(name)
    world, cam = as_oracle_world(s.getWorldPtr()), as_oracle_camera(LW.camera(name))
    old_stats, new_stats = {}, {}
    old, fo = MT.frame_samples(world, cam, 32, 32, LW.SPP, LW.DEPTH, LW.SEED, mode=mode, stats=old_stats)
    new, fn = LT.frame_samples(world, cam, 32, 32, LW.SPP, LW.DEPTH, LW.SEED, mode=mode, stats=new_stats)
    assert fo.all() and fn.all() and bits_equal(new, old), mismatch_report(new, old)
    assert all(np.array_equal(new_stats[k], old_stats[k]) for k in old_stats)


# ---- the pin that carries the pad --------------------------------------------------------------------------------------------------------------------
N_PIN = 10 ** 6
CHUNK = 50000


def _wall_points(rng, n):
    """n points on the six walls of the 10 x 10 x 10 room, a hair inside none of them: the hit points of wall hits"""
    pts = rng.random((n, 3)) * 10
    face = rng.integers(0, 6, n)
    pts[np.arange(n), face % 3] = np.where(face < 3, 0.0, 10.0)
    return pts.astype(F)


def pin_rays(t, prims, quads, rng, n):
    """(hit_p, d) (n, 3) float32: from points on the room's walls to targets on the lights — interior points; vertices; edge midpoints; points one ulp to either
    side of an edge (the midpoint and a vertex-near point with each coordinate moved by one ulp up or down); and, a sixth of them, axis-parallel directions with
    two zero components from the wall point straight under, over or beside a target.  A sphere's targets: points of its surface, its centre, silhouette points."""
    hit_p = _wall_points(rng, n)
    j = rng.integers(0, t.n_l, n)
    target = np.zeros((n, 3), F)
    what = rng.integers(0, 6, n)
    for light in range(t.n_l):
        rows = np.nonzero(j == light)[0]
        if len(rows) == 0:
            continue
        w = what[rows]
        if t.kind[light] == SPHERE:
            pr = prims[t.index[light]]
            c, r = pr["c0"].astype(np.float64), float(pr["radius"])
            u = rng.normal(size=(len(rows), 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            to_c = c[None, :] - hit_p[rows].astype(np.float64)
            perp = np.cross(to_c, u)
            perp /= np.maximum(np.linalg.norm(perp, axis=1), 1e-30)[:, None]
            pt = np.where((w == 0)[:, None], c[None, :], np.where((w == 1)[:, None] | (w == 2)[:, None], c[None, :] + perp * r, c[None, :] + u * r))
            target[rows] = pt.astype(F)
            continue
        q = quads[t.index[light]]
        Q, u, v = q["Q"].astype(F), q["u"].astype(F), q["v"].astype(F)
        tri = t.kind[light] == TRIANGLE
        a, b = rng.random(len(rows), dtype=F), rng.random(len(rows), dtype=F)
        corner = rng.integers(0, 3 if tri else 4, len(rows))
        ca, cb = np.array([0, 1, 0, 1], F)[corner], np.array([0, 0, 1, 1], F)[corner]
        edge = rng.integers(0, 3, len(rows))   # u edge (b = 0), v edge (a = 0), the far edge (a + b = 1: the diagonal, a quad's too)
        s_ = rng.random(len(rows), dtype=F)
        s_ = np.where(w == 2, F(0.5), s_)      # what 2: edge midpoints
        ea = np.where(edge == 0, s_, np.where(edge == 1, F(0), s_))
        eb = np.where(edge == 0, F(0), np.where(edge == 1, s_, F(1) - s_))
        interior = LT._tri_point(a, b, Q, u, v, np.zeros((len(rows), 3), F)) if tri else (Q + u * a[:, None]) + v * b[:, None]
        vertex = (Q + u * ca[:, None]) + v * cb[:, None]
        on_edge = (Q + u * ea[:, None]) + v * eb[:, None]
        step = rng.integers(0, 2, (len(rows), 3)) * 2 - 1
        beside = np.nextafter(on_edge, np.where(step > 0, F(np.inf), F(-np.inf)).astype(F))
        target[rows] = np.where((w == 0)[:, None], interior, np.where((w == 1)[:, None], vertex, np.where((w == 2)[:, None] | (w == 3)[:, None], on_edge, beside)))
    axis = what == 5                      # straight along an axis: the wall point that shares two coordinates with the target
    ax = rng.integers(0, 3, n)
    wall = np.where(rng.integers(0, 2, n) == 0, F(0), F(10))
    moved = target.copy()
    moved[np.arange(n), ax] = wall
    hit_p = np.where(axis[:, None], moved, hit_p)
    d = target - hit_p
    assert (d[axis] == 0).sum(axis=1).min() >= 2
    return hit_p, d


def pin_check(name, n, seed=7):
    """(rays, rays whose linear sum is > 0, positive terms, leaf visits, misses, sums that differ) of the pin on LW.scene(name)"""
    world = as_oracle_world(LW.scene(name).getWorldPtr())
    prims, quads, _ = LT.world_arrays(world)
    t = LT.tree_of(world)
    rng = np.random.default_rng(seed)
    lit = positive = visits = misses = differ = 0
    with np.errstate(all="ignore"):
        for first in range(0, n, CHUNK):
            k = min(CHUNK, n - first)
            hp, dd = pin_rays(t, prims, quads, rng, k)
            len2 = LT.dot(dd, dd)
            ln = np.sqrt(len2)
            terms = np.zeros((t.n_l, k), F)
            linear = np.zeros(k, F)
            for j in range(t.n_l):   # the linear loop over the permuted table, every term kept
                terms[j] = LT.leaf_term(t, prims, quads, j, hp, dd, len2, ln)[0]
                linear = linear + terms[j]
            reached = np.zeros((t.n_l, k), bool)
            walked = np.zeros(k, F)

            def visit(rows, leaves):
                reached[leaves, rows] = True
                walked[rows] = walked[rows] + terms[leaves, rows]   # leaf_term's own value of that leaf on that ray (one function, one result)

            LT.tree_walk(t, hp, dd, visit)
            pos = terms > 0
            lit += int((linear > 0).sum())
            positive += int(pos.sum())
            visits += int(reached.sum())
            misses += int((pos & ~reached).sum())
            differ += int((walked.view(np.uint32) != linear.view(np.uint32)).sum())
    return n, lit, positive, visits, misses, differ


@pytest.mark.parametrize("name", LW.PIN_WORLDS)
def test_the_walk_misses_no_light_and_its_sum_is_the_linear_loops_bit_for_bit(name):
    """A closed icosphere(2) (320 lights), E10's 64-triangle panel, and a quad, a sphere and an icosphere(1) mixed (82): 10^6 directions each.  Zero misses is a
    condition: a miss means the pad or k is wrong, not this test."""
    n, lit, positive, visits, misses, differ = pin_check(name, N_PIN)
    n_l = LW.WORLDS[name][2]
    print(f"{name}: {n} directions, {lit} with a light term > 0, {positive} positive terms, {visits} leaf visits ({visits / n:.2f} per direction of {n_l} lights), "
          f"{misses} misses, {differ} sums differ")
    assert lit > 0.7 * n and positive >= lit and visits >= positive   # the targets are met; a closed mesh twice
    assert visits < 0.25 * n * n_l                                    # and the tree prunes
    assert misses == 0 and differ == 0


def test_tree_density_computes_what_the_pin_looks_up():
    """tree_density (the twin's own path: leaf_term at each leaf visit) against linear_density on a smaller set of the pin's rays"""
    for name in LW.PIN_WORLDS:
        world = as_oracle_world(LW.scene(name).getWorldPtr())
        prims, quads, _ = LT.world_arrays(world)
        t = LT.tree_of(world)
        hp, dd = pin_rays(t, prims, quads, np.random.default_rng(3), 4000)
        with np.errstate(all="ignore"):
            len2 = LT.dot(dd, dd)
            ln = np.sqrt(len2)
            walked = LT.tree_density(t, prims, quads, hp, dd, len2, ln)
            linear, positive = LT.linear_density(t, prims, quads, hp, dd, len2, ln)
        assert bits_equal(walked, linear) and (positive > 0).mean() > 0.7


def test_nan_slabs_enter_nothing_a_light_could_be_met_through():
    """a ray with a zero component that starts IN a face plane of a padded box: 0 * inf; the glm selections keep or drop the NaN by position, and either way the
    walk's sum is the linear loop's"""
    world = as_oracle_world(LW.scene("two").getWorldPtr())
    prims, quads, _ = LT.world_arrays(world)
    t = LT.tree_of(world)
    rows = []
    for i in range(t.n_nodes):
        for ax in range(3):
            for plane in (t.lo[i, ax], t.hi[i, ax]):
                for other in range(3):
                    if other == ax:
                        continue
                    o = ((t.lo[i] + t.hi[i]) * F(0.5)).astype(F)
                    o[ax] = plane
                    o[other] = F(0)
                    d = np.zeros(3, F)
                    d[other] = F(1)
                    rows.append((o, d))
    hp, dd = np.array([r[0] for r in rows], F), np.array([r[1] for r in rows], F)
    with np.errstate(all="ignore"):
        len2 = LT.dot(dd, dd)
        ln = np.sqrt(len2)
        assert np.isnan((t.lo[0] - hp) * (F(1) / dd)).any()
        walked = LT.tree_density(t, prims, quads, hp, dd, len2, ln)
        linear, _ = LT.linear_density(t, prims, quads, hp, dd, len2, ln)
    assert bits_equal(walked, linear)


# ---- the mathematics, through the twin's own functions ----------------------------------------------------------------------------------------------
N_DRAWS = 10 ** 6


def test_drawn_indices_follow_the_areas():
    """the share of draws that choose light j is area_j / A within 5 binomial standard errors, for every light of a table with areas 1 : 10^4 and of the mixed one"""
    for name in ("areas", "mixed", "three_kinds"):
        t = LT.tree_of(as_oracle_world(LW.scene(name).getWorldPtr()))
        rng = np.random.default_rng(11)
        nxt = ((rng.integers(0, 1 << 24, N_DRAWS) + 1).astype(np.float64) / (1 << 24)).astype(F)   # the stream's uniforms: k 2^-24, k in [1, 2^24]
        li = LT.choose(t.cdf, nxt * t.A)
        share = np.bincount(li, minlength=t.n_l) / N_DRAWS
        want = t.area.astype(np.float64) / t.area.astype(np.float64).sum()
        se = np.sqrt(want * (1 - want) / N_DRAWS)
        worst = np.abs(share - want) / (5 * se)
        print(f"{name}: {t.n_l} lights, area shares {want.min():.2e} .. {want.max():.2e}, worst |diff| / (5 se) = {worst.max():.3f}")
        assert (np.abs(share - want) <= 5 * se).all() and share.min() > 0


def _solid_angle_triangle(verts, hit_p):
    """Van Oosterom and Strackee (1983), float64"""
    r = [np.array(v, np.float64) - np.array(hit_p, np.float64) for v in verts]
    l = [np.linalg.norm(x) for x in r]
    num = abs(np.dot(r[0], np.cross(r[1], r[2])))
    den = l[0] * l[1] * l[2] + np.dot(r[0], r[1]) * l[2] + np.dot(r[0], r[2]) * l[1] + np.dot(r[1], r[2]) * l[0]
    return 2 * np.arctan2(num, den)


def test_the_mean_of_one_over_pl_is_the_summed_solid_angle():
    """Mode 16's light draws — the choice by area, the kind's point, the walk's density over A — on a table whose lights do not overlap as seen from the hit point:
    E[1 / pl] = the solid angle of the support = the sum over the lights (triangles: Van Oosterom and Strackee in float64, a quad as two; a sphere: the cap
    2 pi (1 - sqrt(1 - r^2 / D^2))), within 5 standard errors of the mean"""
    p = pkg()
    s = p.Scene()
    emit = s.DiffuseLight((1, 1, 1))
    hit = (5.0, 0.0, 5.0)
    tris = [((1, 8, 1), (3, 8, 1.5), (1.5, 9, 3)), ((7, 6, 7), (9, 6.5, 7), (8, 8, 9)), ((4.5, 9, 4.5), (5.5, 9, 4.7), (5, 9.5, 5.6))]
    quad = ((1, 7, 7), (2, 0, 0), (0, 0.5, 1.5))
    sphere = ((8, 7, 2), 0.8)
    for tri in tris:
        s.MakeTriangle(*tri, emit)
    s.MakeQuad(*quad, emit)
    s.MakeSphere(*sphere, emit)
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), s.Lambertian((0.5, 0.5, 0.5)))   # the floor the hit point lies on: the world's bounds
    s.MakeHittableList()
    world = as_oracle_world(s.getWorldPtr())
    prims, quads, _ = LT.world_arrays(world)
    t = LT.tree_of(world)
    assert t.n_l == 5 and sorted(t.kind.tolist()) == [QUAD, SPHERE, TRIANGLE, TRIANGLE, TRIANGLE]
    Q, u, v = (np.array(x, np.float64) for x in quad)
    omega = sum(_solid_angle_triangle(tri, hit) for tri in tris) + _solid_angle_triangle((Q, Q + u, Q + v), hit) + _solid_angle_triangle((Q + u + v, Q + u, Q + v), hit)
    D2 = sum((a - b) ** 2 for a, b in zip(sphere[0], hit))
    omega += 2 * np.pi * (1 - np.sqrt(1 - sphere[1] ** 2 / D2))
    rng = np.random.default_rng(23)
    li = LT.choose(t.cdf, rng.random(N_DRAWS, dtype=F) * t.A)
    hp = np.ascontiguousarray(np.broadcast_to(F(hit), (N_DRAWS, 3)))
    dd = np.zeros((N_DRAWS, 3), F)
    for j in range(t.n_l):
        rows = np.nonzero(li == j)[0]
        a, b = rng.random(len(rows), dtype=F), rng.random(len(rows), dtype=F)
        if t.kind[j] == SPHERE:
            pr = prims[t.index[j]]
            g = rng.normal(size=(len(rows), 3))
            on_unit = (g / np.linalg.norm(g, axis=1)[:, None]).astype(F)
            dd[rows] = (pr["c0"].astype(F) + on_unit * F(pr["radius"])) - hp[rows]
        else:
            q = quads[t.index[j]]
            if t.kind[j] == TRIANGLE:
                dd[rows] = LT._tri_point(a, b, q["Q"], q["u"], q["v"], hp[rows])
            else:
                dd[rows] = ((q["Q"].astype(F) + q["u"].astype(F) * a[:, None]) + q["v"].astype(F) * b[:, None]) - hp[rows]
    with np.errstate(all="ignore"):
        len2 = LT.dot(dd, dd)
        pl = LT.tree_density(t, prims, quads, hp, dd, len2, np.sqrt(len2)) / t.A
        inv = np.where(pl > 0, 1.0 / pl.astype(np.float64), 0.0)
    mean, se = inv.mean(), inv.std(ddof=1) / np.sqrt(N_DRAWS)
    print(f"mean 1/pl {mean:.6e} +- {se:.2e}, summed solid angle {omega:.6e}, |diff| / (5 se) = {abs(mean - omega) / (5 * se):.3f}, draws with pl = 0: {(pl <= 0).mean():.2e}")
    assert abs(mean - omega) <= 5 * se


def _linear_scan(cdf, x):
    out = np.full(len(x), len(cdf) - 1, np.int64)
    for i, xi in enumerate(x):
        for j in range(len(cdf)):
            if cdf[j] > xi:
                out[i] = j
                break
    return out


@pytest.mark.parametrize("name", ["two", "three_kinds", "mesh_lamp", "sixty_five", "areas"])
def test_the_binary_search_is_a_linear_scan_at_every_edge(name):
    t = LT.tree_of(as_oracle_world(LW.scene(name).getWorldPtr()))
    xs = [F(0), np.nextafter(F(0), F(1)), t.A, F(F(1) * t.A), np.nextafter(t.A, F(0)), np.nextafter(t.A, F(np.inf))]
    for c in t.cdf:
        xs += [c, np.nextafter(c, F(0)), np.nextafter(c, F(np.inf))]
    xs = np.array(xs, F)
    got = LT.choose(t.cdf, xs)
    assert got.tolist() == _linear_scan(t.cdf, xs).tolist()
    assert LT.choose(t.cdf, np.array([t.A], F))[0] == t.n_l - 1 and LT.choose(t.cdf, np.array([F(1) * t.A], F))[0] == t.n_l - 1   # next = 1: the clamped last index
    assert LT.choose(t.cdf, t.cdf[:1])[0] == min(1, t.n_l - 1)                                                                      # x = c_0 belongs to light 1


# ---- the worlds -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [w for w in LW.SHAPE_WORLDS if w != "icosphere2"] + ["no_triangles", "three_kinds_list"])
def test_worlds_exercise_what_they_are_there_for(name):
    run = LW.run(name)
    st = run.stats
    print(name, {k: v for k, v in st.items() if k != "light_samples"})
    assert run.followed and st["not_followed"] == 0 and np.isfinite(run.sums).all() and (run.sums[..., :3] > 0).any(axis=2).mean() > 0.5
    assert st["light_samples"][run.lights:].sum() == 0 and st["light_samples"].sum() > 0 and st["tree_leaves"] > 0
    assert (st["index_clamped"] > 0) == (name == "clamped_last_index")
    assert st["tree_sphere_uncredited"] > 0 or name != "silhouette"   # (a room's own lamp may lose a draw on its silhouette too)
    if name == "mesh_lamp":
        assert st["two_tri_crossings"] > 0.9 * st["tri_light_half"]
    if name == "areas":
        assert st["light_samples"][:2].min() == 0 or st["light_samples"][:2].max() > 50 * max(st["light_samples"][:2].min(), 1)
    if name in ("no_triangles", "silhouette"):
        assert run.scene.getWorldPtr().n_quads > 0 and st["tri_light_half"] == 0
        n_tri = C.c_uint32(7)
        assert pkg().lib().rt_world_triangles(C.byref(run.scene.getWorldPtr()), C.byref(n_tri)) == 0 and n_tri.value == 0
    if name == "sixty_five":
        with pytest.raises(pkg().capi.RtError, match="more than 64 lights"):
            run.scene.light_table("mesh")


def test_the_uniform_by_count_choice_is_what_mode_4_does_and_area_weighting_is_not():
    """a ceiling panel beside a closed mesh: by count the panel gets 1 / n_l of the light draws, by area its share of the area"""
    t = LT.tree_of(as_oracle_world(LW.scene("mixed").getWorldPtr()))
    quad = int(np.nonzero(t.kind == QUAD)[0][0])
    assert t.n_l == 82 and t.area[quad] / t.A > 5.0 / 82
