"""Triangles without a GPU: the twin's two pins, the oracle's triangle rule pinned to the twin (crafted rays, room rays, whole samples), what
the worlds of tests/test_gpu_triangles_oracle.py hold, rt_quad's layout, that no earlier world moved a byte, the order of a flat world, bounds, refusals, the
mesh transform, what light sampling does with a triangle, and the estimator's sanity on the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _nee2_twin as T2
import _nee_twin as T
import _oracle as O
import _tri_twin as TT
import _tri_worlds as TW
import _kernel_table as KT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg, random_mixed_scene
from test_light_sampling_cpu import cornell_camera, plain_samples

SEED = 1984
RT_ERR_INVALID = 1
F = np.float32


# ---- the pins: before anything is compared with the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1, 2, 3], ids=["topdown", "sah", "bottomup", "list"])
def test_pin_1_closest_intersection_is_orc_trace_batch_on_worlds_without_triangles(builder):
    p = pkg()
    rng = np.random.default_rng(70 + builder)
    s = p.Scene()
    mats = [s.Lambertian((0.5, 0.5, 0.5)), s.Metal((0.8, 0.8, 0.8), 0.2), s.DiffuseLight((4, 4, 4))]
    for i in range(19):
        s.MakeSphere((rng.random(3, dtype=F) * 10 - 5), float(0.2 + rng.random() * 0.8), mats[i % 3])
    for i in range(17):
        Q = (rng.random(3, dtype=F) * 12 - 6)
        u, v = ((F([rng.random() * 4 + 0.5, 0, 0]), F([0, 0, rng.random() * 4 + 0.5])) if i % 3 == 0 else ((rng.standard_normal(3) * 2).astype(F), (rng.standard_normal(3) * 2).astype(F)))
        s.MakeQuad(Q, u, v, mats[i % 3])
    [s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList][builder]()
    w = as_oracle_world(s.getWorldPtr())
    n = 4000
    rays = np.zeros((n, 7), F)
    rays[:, 0:3] = rng.random((n, 3), dtype=F) * 16 - 8
    rays[:, 3:6] = (rng.random((n, 3), dtype=F) * 10 - 5) - rays[:, 0:3]   # towards the objects
    rays[: n // 8, 3 + builder % 3] = 0          # axis-parallel rays: the box test's 0 / 0 and x / 0
    hit, t, prim, normal = np.zeros(n, np.int32), np.zeros(n, F), np.zeros(n, np.int32), np.zeros((n, 3), F)
    assert O.lib().orc_trace_batch(C.byref(w), n, rays, hit, t, prim, normal) == 0
    got = TT.closest_intersection(w, rays)
    assert np.array_equal(got[0], hit) and np.array_equal(got[2], prim)
    assert bits_equal(got[1], t) and bits_equal(got[3], normal), mismatch_report(got[3], normal)
    assert 0.2 < hit.mean() < 0.98 and (prim >= 19).any() and ((prim >= 0) & (prim < 19)).any()


def test_pin_2_a_whole_sample_is_the_oracle_and_with_sampling_on_the_light_sampling_twin():
    p = pkg()
    W = H = 16
    scene = O.Scene.cornell_box()
    cam = cornell_camera(W, H)
    off, followed = TT.frame_samples(scene.world, cam, W, H, 4, 6, SEED, mode=0)
    exp = plain_samples(scene.world, cam, W, H, 4, 6)
    assert followed.all() and bits_equal(off, exp), mismatch_report(off, exp)
    for builder_args in ({}, {"as_list": True}):
        keep = TW.tri_room(p, plain=True, lamp=True, **builder_args)
        w, c = as_oracle_world(keep.getWorldPtr()), as_oracle_camera(TW.camera(p, 16, 12))
        off, followed = TT.frame_samples(w, c, 16, 12, 3, 8, SEED, mode=0)
        exp = plain_samples(w, c, 16, 12, 3, 8)
        assert followed.all() and bits_equal(off, exp), mismatch_report(off, exp)
        for mode in (1, 2):
            got, f1 = TT.frame_samples(w, c, 16, 12, 3, 8, SEED, mode=mode)
            exp, f2 = T2.frame_samples(w, c, 16, 12, 3, 8, SEED, mode=mode)
            assert f1.all() and f2.all() and bits_equal(got, exp), mismatch_report(got, exp)
        assert not bits_equal(got, off)


# ---- the oracle's kind rule, pinned to the twin: two independent statements of `alpha + beta <= 1`, one in C and one in numpy ------------------------
def orc_trace(w, rays):
    n = len(rays)
    hit, t, prim, normal = np.zeros(n, np.int32), np.zeros(n, F), np.zeros(n, np.int32), np.zeros((n, 3), F)
    assert O.lib().orc_trace_batch(C.byref(w), n, np.ascontiguousarray(rays, F), hit, t, prim, normal) == 0
    return hit, t, prim, normal


def assert_oracle_is_twin(w, rays):
    """hit, t, primitive and normal of every ray, bit for bit, nothing masked; returns the oracle's answer"""
    got, exp = orc_trace(w, rays), TT.closest_intersection(w, rays)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[2]), np.nonzero(got[2] != exp[2])[0][:5]
    assert bits_equal(got[1], exp[1]), mismatch_report(got[1], exp[1])
    assert bits_equal(got[3], exp[3]), mismatch_report(got[3], exp[3])
    return got


def test_oracle_quad_keeps_its_layout_and_has_the_kind():
    dt = O.QUAD_DT
    assert dt.itemsize == 80 and {n: dt.fields[n][1] for n in dt.names} == {"Q": 0, "D": 12, "u": 16, "mat": 28, "v": 32, "kind": 44, "normal": 48, "pad1": 60, "w": 64, "pad2": 76}
    assert dt.fields["kind"][0] == np.dtype("<u4") and dt == pkg().capi.QUAD_DT
    header = open(os.path.join(ROOT, "oracle", "rt_oracle.h")).read()
    assert "pad0" not in header and "sizeof(orc_quad) == 80 && offsetof(orc_quad, kind) == 44" in header   # the compile-time statement


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_pin_3_the_oracle_meets_crafted_rays_as_the_twin_does(as_list):
    p = pkg()
    rays = TW.crafted_rays()
    keep = [TW.unit_world(p, True, as_list), TW.unit_world(p, False, as_list), TW.unit_world(p, True, as_list, second=True), TW.equal_distance_world(p, as_list)]
    tri_w, quad_w, diagonal_w, equal_w = (as_oracle_world(s.getWorldPtr()) for s in keep)   # (a flat world points into its scene: `keep` outlives the views)
    tri, quad = assert_oracle_is_twin(tri_w, rays), assert_oracle_is_twin(quad_w, rays)
    # inside; alpha + beta exactly 1: inside; one ulp more: outside; (0.75, 0.75) hits the quad and misses the triangle (primitive 0 is the sphere behind the plane)
    assert tri[2][:4].tolist() == [1, 1, 0, 0] and quad[2][:4].tolist() == [1, 1, 1, 1]
    if as_list:
        assert tri[2][4:9].tolist() == [1, 1, 1, 1, 1]     # every vertex and edge midpoint is inside
    assert (tri[2][9:] != 1).all() and (quad[2][9:] != 1).all()
    diagonal = assert_oracle_is_twin(diagonal_w, TW.down_z(TW.DIAGONAL))
    assert diagonal[2].tolist() == [1, 1, 1, 1, 2]          # a point of the shared diagonal is inside both triangles: the first visited keeps it
    equal = assert_oracle_is_twin(equal_w, TW.down_z(TW.EQUAL_DISTANCE))
    assert equal[1].tolist() == [1.0, 1.0, 1.0] and equal[2][2] == 1   # (0.75, 0.75): the quad alone
    if as_list:
        assert equal[2].tolist() == [1, 1, 1]                # the quad was there first; both triangles met rec.distance == t


@pytest.mark.parametrize("builder", ["BuildBVH_TopDown", "BuildBVH_SAH", "BuildBVH_BottomUp", "MakeHittableList"])
def test_pin_3_the_oracle_meets_4096_room_rays_as_the_twin_does(builder):
    p = pkg()
    scene = TW.tri_room(p, as_list=builder == "MakeHittableList", builder=builder)
    got = assert_oracle_is_twin(as_oracle_world(scene.getWorldPtr()), TW.room_rays(4096))
    assert got[0].all() and 0.1 < (got[2] >= 7).mean() < 0.9   # a closed room; rays end on triangles and on parallelograms


def test_pin_4_whole_samples_of_the_oracle_are_the_twins():
    run = TW.run()
    assert run.followed
    w, cam = run.world, as_oracle_camera(run.cam)
    samples = plain_samples(w, cam, TW.W, TW.H, TW.SPP, TW.DEPTH)   # orc_radiance_batch, one call per sample index
    assert bits_equal(samples, run.samples), mismatch_report(samples, run.samples)
    sums = TT.in_order_sums(samples)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    frame, _ = O.render(w, cam, TW.W, TW.H, TW.SPP, TW.DEPTH, TW.SEED)
    assert bits_equal(frame, run.frame), mismatch_report(frame, run.frame)
    assert not bits_equal(frame, TW.run(lamp=True).frame)


def test_the_oracles_scene_builders_refuse_a_triangle():
    mats = np.zeros(1, O.MAT_DT)
    quads = np.zeros(2, O.QUAD_DT)
    quads["u"], quads["v"] = (1, 0, 0), (0, 1, 0)
    quads["Q"][1] = (0, 0, 1)
    for builder in (0, 1, 2, 3):
        assert O.Scene.from_arrays_ext(np.zeros(0, O.PRIM_DT), quads, mats, builder).h   # parallelograms: built as ever
    quads["kind"][1] = 1
    for builder in (0, 1, 2, 3):
        assert O.lib().orc_scene_from_arrays_ext(0, None, 2, quads.ctypes.data, 1, mats.ctypes.data, builder, 0, None) is None   # NULL, not a mis-sorted world


# ---- what the worlds of tests/test_gpu_triangles_oracle.py hold ---------------------------------------------------------------------------------------
def contents(scene):
    """(n_prims, n_plain_quads, triangles, materials in use on a primitive, moving spheres)"""
    w, q = scene.getWorldPtr(), scene.quads()
    _, prims, mats = scene.arrays()
    used = set(mats["type"][q["mat"]].tolist()) | set(mats["type"][prims["mat"] & np.uint32(0x7fffffff)].tolist())
    n_plain = int((q["kind"] == 0).sum())
    assert scene.n_triangles() == w.n_quads - n_plain and (q["kind"][:n_plain] == 0).all() and (q["kind"][n_plain:] == 1).all()
    return w.n_prims, n_plain, scene.n_triangles(), used, int((prims["mat"] >> 31).sum())


def ext_level(scene):
    """the EXT level of the kernel a world gets (DeviceScene::pack): 2 with a noise or image material, else 1 with anything beyond the reference's features"""
    w = scene.getWorldPtr()
    types = scene.arrays()[2]["type"]
    return 2 if (types >= TW.MAT["noise"]).any() else int(w.n_quads != 0 or w.background != 0 or (types >= TW.MAT["light"]).any())


M = TW.MAT


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_the_wide_rooms_hold_what_they_are_for(as_list):
    p = pkg()
    base = contents(TW.tri_room(p, as_list=as_list))
    assert base == (0, 7, 85, {M["lambertian"], M["metal"], M["checker"], M["light"]}, 0)
    wide = TW.wide_room(p, as_list=as_list)
    # one wall less; icosphere(1) of glass (80) and a metal tetrahedron (4) more; one moving sphere
    assert contents(wide) == (1, 6, 85 + 84, {M["lambertian"], M["metal"], M["dielectric"], M["checker"], M["light"]}, 1) and ext_level(wide) == 1
    w, q, mats = wide.getWorldPtr(), wide.quads(), wide.arrays()[2]
    assert w.background == 1 and tuple(w.background_color) == tuple(F(TW.SKY)) and w.kind == int(as_list)
    assert (mats["type"][q["mat"][q["kind"] == 1]] == M["dielectric"]).sum() == 80
    fuzzy = q[(q["kind"] == 1) & (mats["type"][q["mat"]] == M["metal"]) & (mats["param"][q["mat"]] == F(0.4))]
    assert len(fuzzy) == 4
    assert not ((q["kind"] == 0) & (q["Q"] == F([10, 0, 0])).all(axis=1)).any()   # the right wall is gone
    ext2 = TW.wide_room(p, ext=2, as_list=as_list)
    assert contents(ext2) == (2, 6, 85 + 84 + 2, set(range(8)), 1) and ext_level(ext2) == 2
    q2, mats2, prims2 = ext2.quads(), ext2.arrays()[2], ext2.arrays()[1]
    for kind in ("noise", "image"):   # each on exactly one triangle, and on nothing else
        assert (mats2["type"][q2["mat"]] == M[kind]).sum() == 1 and q2["kind"][mats2["type"][q2["mat"]] == M[kind]].tolist() == [1]
    assert (mats2["type"][prims2["mat"] & np.uint32(0x7fffffff)] == M["isotropic"]).sum() == 1
    assert ext2.getWorldPtr().perlin and ext2.getWorldPtr().image
    assert contents(TW.wide_room(p, ext=2, medium=False, as_list=as_list))[:3] == (1, 6, 171)


@pytest.mark.parametrize("builder", TW.BUILDERS)
def test_the_boundary_worlds_hold_what_they_are_for(builder):
    p = pkg()
    expect = {"triangles_only": (0, 0, 86), "one_quad": (1, 1, 84), "one_triangle": (1, 14, 1), "siblings": (0, 7, 7)}
    for which, exp in expect.items():
        s = TW.boundary_world(p, which, builder)
        assert contents(s)[:3] == exp and ext_level(s) == 1 and s.getWorldPtr().kind == int(builder == "MakeHittableList")
    assert M["dielectric"] in contents(TW.boundary_world(p, "one_quad", builder))[3] and M["dielectric"] in contents(TW.boundary_world(p, "one_triangle", builder))[3]


def test_the_last_parallelogram_and_the_first_triangle_are_the_two_leaves_of_one_node():
    """a leaf of the flat tree holds one primitive, so two primitives are never closer in it than as the two leaf children of one inner node"""
    p = pkg()
    s = TW.boundary_world(p, "siblings", "BuildBVH_SAH")
    n_prims, n_plain, _, _, _ = contents(s)
    last, first = n_prims + n_plain - 1, n_prims + n_plain
    assert (last, first) in TW.sibling_leaves(s) or (first, last) in TW.sibling_leaves(s)
    q = s.quads()
    assert q["kind"][n_plain - 1] == 0 and q["kind"][n_plain] == 1 and q["Q"][n_plain - 1].tolist() == [0.5, 0, 0] and bits_equal(q["Q"][n_plain], F([1.6, 0, 0]))


def test_the_mesh_rooms_and_the_closed_mesh_hold_what_they_are_for():
    p = pkg()
    assert contents(TW.mesh_room(p, 2))[:3] == (0, 7, 85 + 320) and contents(TW.mesh_room(p, 4))[:3] == (0, 7, 85 + 5120)
    assert M["dielectric"] in contents(TW.mesh_room(p, 2))[3]
    for as_list in (False, True):
        s, rays, (nv, ne, nf) = TW.closed_mesh_world(p, as_list)
        assert contents(s)[:3] == (0, 0, 320) and (nv, ne, nf) == (162, 480, 320) and len(rays) == 2 * (nv + ne + nf)
        hit = orc_trace(as_oracle_world(s.getWorldPtr()), rays)[0]
        print(f"closed icosphere(2), {'list' if as_list else 'bvh'}: {int((hit == 0).sum())} of {len(rays)} rays at vertices, edge midpoints and centroids pass through")   # a measurement (§18)
        assert hit[nv + ne:nv + ne + nf].all() and hit[-nf:].all()   # the centroids are well inside their faces


def test_the_random_triangle_worlds_cover_what_they_are_for():
    p = pkg()
    seen = {"builder": set(), "camera": set(), "ext": set(), "mats": set(), "shapes": set(), "meshes": set()}
    specials = moving = no_quads = 0
    for seed in range(12):
        s, cam, W, H, spp, depth, r = TW.random_tri_world(p, seed)
        n_prims, n_plain, n_tri, used, n_moving = contents(s)
        assert n_tri >= 5 and W <= 48 and H <= 32 and 1 <= spp <= 8 and ext_level(s) == r["ext"]
        assert 1 <= len(r["triangles"]["meshes"]) <= 3 and 5 <= n_tri - sum(n for _, n in r["triangles"]["meshes"]) <= 30
        seen["builder"].add(r["builder"]); seen["camera"].add(r["camera"]); seen["ext"].add(r["ext"]); seen["mats"] |= used
        seen["shapes"] |= {k for k, v in r["triangles"]["free"].items() if v}
        seen["meshes"] |= {name for name, _ in r["triangles"]["meshes"]}
        specials += any(float(F(x)) in [float(F(v)) for v in TW.EYE_SPECIALS] for x in r["eye"])
        moving += n_moving > 0
        no_quads += n_plain == 0
    assert seen["builder"] == set(TW.BUILDERS) and seen["camera"] == set(TW.CAMERAS) and seen["ext"] == {1, 2} and seen["mats"] == set(range(8))
    assert seen["shapes"] == {"plain", "axis", "sliver", "large"} and seen["meshes"] == {"tetrahedron", "icosphere(0)", "icosphere(1)", "icosphere(2)"}
    assert specials >= 1 and moving >= 6 and no_quads >= 1


# ---- data ----------------------------------------------------------------------------------------------------------------------------------------
def test_rt_quad_keeps_its_layout_and_the_c_check_agrees():
    p = pkg()
    dt = p.capi.QUAD_DT
    assert dt.itemsize == 80 and C.sizeof(p.capi.WorldFlat) == 128
    assert {n: dt.fields[n][1] for n in dt.names} == {"Q": 0, "D": 12, "u": 16, "mat": 28, "v": 32, "kind": 44, "normal": 48, "pad1": 60, "w": 64, "pad2": 76}
    assert dt.fields["kind"][0] == np.dtype("<u4") and (p.capi.QUAD_PARALLELOGRAM, p.capi.QUAD_TRIANGLE) == (0, 1)
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    assert "#define RT_QUAD_PARALLELOGRAM 0u" in header and "#define RT_QUAD_TRIANGLE 1u" in header and "pad0" not in header
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in ("rt_scene_add_triangle", "rt_scene_add_mesh", "rt_world_triangles", "rt_renderer_kernel_triangles"):
        assert name in declared and name in p.capi.SYMBOLS and getattr(p.lib(), name).argtypes, name
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert "int32_t AddTriangle(" in hpp and "uint32_t AddMesh(" in hpp
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])   # as the other ABI tests do: the check is built where it is missing
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_triangles")])
    out = subprocess.check_output([os.path.join(ROOT, "tests", "cpp_triangles", "triangle_abi_check")], text=True)
    assert out.strip() == "triangle ABI ok"


@pytest.mark.parametrize("which", ["cornell_box", "book2_final"])
def test_earlier_worlds_keep_every_byte(which):
    p = pkg()
    s = getattr(p.Scene, which)() if which == "cornell_box" else getattr(p.Scene, which)(SEED)
    o = getattr(O.Scene, which)() if which == "cornell_box" else getattr(O.Scene, which)(SEED)
    nodes, prims, mats = s.arrays()
    assert s.quads().tobytes() == o.quads.tobytes() and nodes.tobytes() == o.nodes.tobytes() and prims.tobytes() == o.prims.tobytes() and mats.tobytes() == o.materials.tobytes()
    assert not s.quads()["kind"].any() and s.n_triangles() == 0


def test_cornell_lamp_keeps_every_byte():
    p = pkg()
    lamp, box = p.Scene.cornell_lamp().quads(), p.Scene.cornell_box().quads()
    assert len(lamp) == 17 and not lamp["kind"].any() and not lamp["pad1"].any() and not lamp["pad2"].any()
    assert sorted(map(bytes, lamp)) == sorted(bytes(q) for q in box if q["mat"] != 3)


@pytest.mark.parametrize("builder", ["BuildBVH_TopDown", "BuildBVH_SAH", "BuildBVH_BottomUp", "MakeHittableList"])
def test_triangles_follow_the_quads_whatever_the_order_of_the_calls(builder):
    p = pkg()
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    rng = np.random.default_rng(5)
    order = []
    for i in range(24):
        a = rng.random(3) * 8
        if i % 3 == 1:
            assert s.MakeQuad(a, (1, 0, 0.2), (0, 1, 0.1), m) == order.count("q")   # in front of the triangles
            order.append("q")
        elif i % 3 == 2:
            s.MakeSphere(a, 0.4, m)
        else:
            assert s.MakeTriangle(a, a + (1, 0, 0), a + (0, 1, 0.5), m) == len(order)
            order.append("t")
    getattr(s, builder)()
    q = s.quads()
    assert q["kind"].tolist() == [0] * 8 + [1] * 8 and s.n_triangles() == 8
    nodes, prims, _ = s.arrays()
    if builder != "MakeHittableList":
        leaves = sorted(int(n["right"]) for n in nodes if n["left"] == -1)
        assert leaves == list(range(8 + 16))
        for n in nodes[nodes["left"] == -1]:   # a leaf's box is its own primitive's: the permutation kept every record with its box
            if n["right"] >= 8:
                r = q[n["right"] - 8]
                pts = np.stack([r["Q"], r["Q"] + r["u"], r["Q"] + r["v"]] + ([r["Q"] + r["u"] + r["v"]] if r["kind"] == 0 else []))
                assert np.array_equal(n["min"], pts.min(axis=0)) and np.array_equal(n["max"], pts.max(axis=0))


def test_bounds_of_an_axis_aligned_triangle_are_padded():
    p = pkg()
    s = p.Scene()
    s.MakeTriangle((1, 2, 3), (4, 2, 3), (1, 2, 7), s.Lambertian((0.5, 0.5, 0.5)))
    s.MakeHittableList()
    w = s.getWorldPtr()
    half = F(0.0001) / F(2)
    assert list(w.bounds_min) == [1, F(2) - half, 3] and list(w.bounds_max) == [4, F(2) + half, 7]
    s.BuildBVH_TopDown()
    nodes, _, _ = s.arrays()
    assert nodes[0]["min"].tolist() == [1, F(2) - half, 3] and nodes[0]["max"].tolist() == [4, F(2) + half, 7]
    q = s.quads()[0]
    assert q["Q"].tolist() == [1, 2, 3] and q["u"].tolist() == [3, 0, 0] and q["v"].tolist() == [0, 0, 4] and q["kind"] == 1
    o = np.zeros(1, O.QUAD_DT)   # normal, D, w: what quad_finalize gives a quad of the same Q, u, v
    s2 = p.Scene()
    s2.MakeQuad((1, 2, 3), (3, 0, 0), (0, 0, 4), s2.Lambertian((0.5, 0.5, 0.5)))
    q2 = s2.MakeHittableList().quads()[0]
    for f in ("normal", "D", "w"):
        assert bits_equal(q[f], q2[f])


def test_refusals_and_their_messages():
    p = pkg()
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    for a, b, c in (((0, 0, 0), (1, 0, 0), (2, 0, 0)), ((0, 0, 0), (0, 0, 0), (0, 1, 0)), ((0, 0, 0), (1e-30, 0, 0), (0, 1e-30, 0)), ((0, 0, 0), (1e30, 0, 0), (0, 1e30, 0)),
                    ((0, 0, 0), (np.nan, 0, 0), (0, 1, 0))):
        with pytest.raises(p.capi.RtError, match="degenerate triangle") as e:
            s.MakeTriangle(a, b, c, m)
        assert e.value.code == RT_ERR_INVALID
    with pytest.raises(p.capi.RtError, match="material index 7 out of range"):
        s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 7)
    s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], F)
    with pytest.raises(p.capi.RtError, match=r"face 1: vertex index 4 out of range \(4 vertices\)"):
        s.MakeMesh(verts, [[0, 1, 2], [0, 1, 4]], m)
    assert len(s.MakeHittableList().quads()) == 1          # the failed call left the scene as it was
    assert s.MakeMesh(verts, [[0, 1, 2], [0, 1, 3], [2, 1, 0]], m) == (1, 2)   # (0, 1, 3) is a line: skipped, counted out
    s.MakeHittableList()
    assert s.n_triangles() == 2
    # a caller's own flat world: a kind above 1, and a triangle in front of a parallelogram
    w = s.getWorldPtr()
    quads = s.quads()
    n = C.c_uint32(9)
    for kinds, msg in (([0, 2, 1], "quad 1: unknown kind 2"), ([1, 0, 1], "quad 1: a parallelogram behind a triangle")):
        bad = quads.copy()
        bad["kind"] = kinds
        w.quads = bad.ctypes.data
        assert p.lib().rt_world_triangles(C.byref(w), C.byref(n)) == RT_ERR_INVALID and msg in p.lib().rt_last_error().decode() and n.value == 0
        kind, index, area, nl = (C.c_uint32 * 16)(), (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32(9)
        assert p.lib().rt_world_lights(C.byref(w), 2, kind, index, area, C.byref(nl)) == RT_ERR_INVALID and msg in p.lib().rt_last_error().decode()


def test_add_mesh_transforms_as_add_box_does():
    """a box given as 12 triangles, corner for corner: every triangle's first vertex is the Q of the box quad it halves, computed by the same arithmetic"""
    p = pkg()
    a, b, deg, off = (0, 0, 0), (165, 330, 165), 15.0, (265, 0, 295)
    box = p.Scene()
    box.MakeBox(a, b, box.Lambertian((0.7, 0.7, 0.7)), deg, off)
    box.MakeHittableList()
    quads = box.quads()
    mn, mx = np.minimum(a, b).astype(F), np.maximum(a, b).astype(F)
    dx, dy, dz = F([mx[0] - mn[0], 0, 0]), F([0, mx[1] - mn[1], 0]), F([0, 0, mx[2] - mn[2]])
    Qs = [F([mn[0], mn[1], mx[2]]), F([mx[0], mn[1], mx[2]]), F([mx[0], mn[1], mn[2]]), F([mn[0], mn[1], mn[2]]), F([mn[0], mx[1], mx[2]]), F([mn[0], mn[1], mn[2]])]
    us, vs = [dx, -dz, -dx, dz, dx, dx], [dy, dy, dy, dy, -dz, dz]
    verts, faces = [], []
    for Q, u, v in zip(Qs, us, vs):
        k = len(verts)
        verts += [Q, Q + u, Q + v, Q + u + v]
        faces += [[k, k + 1, k + 2], [k + 3, k + 2, k + 1]]
    mesh = p.Scene()
    assert mesh.MakeMesh(np.array(verts, F), faces, mesh.Lambertian((0.7, 0.7, 0.7)), 1.0, deg, off) == (0, 12)
    tris = mesh.MakeHittableList().quads()
    for k in range(6):
        assert bits_equal(tris[2 * k]["Q"], quads[k]["Q"])                          # rot_y(Q) + offset, the same expression
        np.testing.assert_allclose(tris[2 * k]["u"], quads[k]["u"], rtol=0, atol=3e-5)   # a difference of transformed points against a transformed difference
        np.testing.assert_allclose(tris[2 * k]["v"], quads[k]["v"], rtol=0, atol=3e-5)
        np.testing.assert_allclose(tris[2 * k + 1]["Q"], quads[k]["Q"] + quads[k]["u"] + quads[k]["v"], rtol=0, atol=6e-5)
    # scale first, then the rotation, then the translation
    one = p.Scene()
    one.MakeMesh(F([[1, 0, 0], [0, 1, 0], [0, 0, 1]]), [[0, 1, 2]], one.Lambertian((0.5, 0.5, 0.5)), 2.0, 90.0, (10, 20, 30))
    q = one.MakeHittableList().quads()[0]
    np.testing.assert_allclose(q["Q"], [10, 20, 28], atol=1e-5)      # (2, 0, 0) turned about y by 90 degrees is (0, 0, -2)
    np.testing.assert_allclose(q["Q"] + q["u"], [10, 22, 30], atol=1e-5)
    np.testing.assert_allclose(q["Q"] + q["v"], [12, 20, 30], atol=1e-5)


def _lights(p, world, mode):
    kind, index, area, n = (C.c_uint32 * 16)(), (C.c_uint32 * 16)(), (C.c_float * 16)(), C.c_uint32(77)
    rc = p.lib().rt_world_lights(C.byref(world), mode, kind, index, area, C.byref(n))
    return rc, n.value, list(kind)[: n.value], list(index)[: n.value], p.lib().rt_last_error().decode()


def test_light_tables_skip_a_triangle_light_and_refuse_a_world_lit_by_triangles_alone():
    p = pkg()
    s = TW.tri_room(p, lamp=True, tri_light=True)
    w = s.getWorldPtr()
    quads, mats = s.quads(), s.arrays()[2]
    emitters = [i for i in range(len(quads)) if mats["type"][quads["mat"][i]] == 4]
    assert [int(quads["kind"][i]) for i in emitters] == [0, 1]
    assert _lights(p, w, 1)[:4] == (0, 1, [0], [emitters[0]]) and _lights(p, w, 2)[:3] == (0, 2, [0, 1])
    tl = TT.lights_of(*T2.world_arrays(as_oracle_world(w)), 2)
    assert tl[1].tolist() == _lights(p, w, 2)[3]
    only = p.Scene()
    only.MakeTriangle((0, 5, 0), (2, 5, 0), (0, 5, 2), only.DiffuseLight((5, 5, 5)))
    only.MakeQuad((-5, 0, -5), (10, 0, 0), (0, 0, 10), only.Lambertian((0.5, 0.5, 0.5)))
    only.BuildBVH_TopDown()
    plain = p.Scene()
    plain.MakeQuad((-5, 0, -5), (10, 0, 0), (0, 0, 10), plain.Lambertian((0.5, 0.5, 0.5)))
    plain.BuildBVH_TopDown()
    for mode in (1, 2):   # word for word what a world without any light is told
        got, exp = _lights(p, only.getWorldPtr(), mode), _lights(p, plain.getWorldPtr(), mode)
        assert got[0] == RT_ERR_INVALID and got[4] == exp[4] and ("no quad light" if mode == 1 else "no light to sample") in got[4]


def test_the_kind_rule_on_the_twin_and_a_preset_distance():
    p = pkg()
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    s.MakeSphere((0.5, 0.5, -10), 3.0, m)
    s.MakeHittableList()
    w = as_oracle_world(s.getWorldPtr())
    eps = F(2.0 ** -23)
    rays = np.zeros((4, 7), F)
    rays[:, 0:2] = [(0.25, 0.25), (0.5, 0.5), (0.5, F(0.5) + eps), (0.75, 0.75)]
    rays[:, 2], rays[:, 5] = 1, -1
    assert TT.closest_intersection(w, rays)[2].tolist() == [1, 1, 0, 0]
    same = np.repeat(rays[:1], 3, axis=0)
    hit, t, prim, _ = TT.closest_intersection(w, same, preset=F([1.0, np.nextafter(F(1), F(2)), 0.5]))
    assert hit.tolist() == [0, 1, 0] and prim.tolist() == [-1, 1, -1] and t.tolist() == [1.0, 1.0, 0.5]   # t >= rec.distance rejects


def test_a_wall_cut_into_two_triangles_gives_the_same_expected_image():
    """The project's statistical rule, twin against twin: frame-mean luminance M with its standard error from the per-pixel sample
    variances, whole frame and the four quadrants: |M_tri - M_quad| <= 4 sqrt(SE_tri^2 + SE_quad^2); 24 x 24, depth 8, 256 against 4096 samples."""
    p = pkg()
    W = H = 24
    cam = as_oracle_camera(TW.camera(p, W, H))
    keep_t, keep_q = TW.tri_room(p, wall_as_triangles=True), TW.tri_room(p, plain=True)
    assert keep_t.n_triangles() == 2 and keep_q.n_triangles() == 0
    tri, f1 = TT.frame_samples(as_oracle_world(keep_t.getWorldPtr()), cam, W, H, 256, 8, SEED)
    quad, f2 = TT.frame_samples(as_oracle_world(keep_q.getWorldPtr()), cam, W, H, 4096, 8, SEED)
    assert f1.all() and f2.all() and np.isfinite(tri).all()

    def mean_and_se(samples, rows, cols):
        y = T.luminance(samples[rows, cols].astype(np.float64))
        return y.mean(), np.sqrt((y.var(axis=2, ddof=1) / y.shape[2]).sum()) / (y.shape[0] * y.shape[1])

    regions = {"frame": (slice(0, H), slice(0, W))}
    for qy in (0, 1):
        for qx in (0, 1):
            regions[f"quadrant {qy}{qx}"] = (slice(qy * H // 2, (qy + 1) * H // 2), slice(qx * W // 2, (qx + 1) * W // 2))
    for region, (rows, cols) in regions.items():
        m_t, se_t = mean_and_se(tri, rows, cols)
        m_q, se_q = mean_and_se(quad, rows, cols)
        print(f"{region}: triangles {m_t:.5f} +- {se_t:.5f}   quads {m_q:.5f} +- {se_q:.5f}   |diff| / bound = {abs(m_t - m_q) / (4 * np.hypot(se_t, se_q)):.3f}")
        assert m_q > 0.01 and abs(m_t - m_q) <= 4.0 * np.hypot(se_t, se_q), region


def test_the_test_room_is_followed_everywhere_and_shows_its_triangles():
    run = TW.run()
    assert run.followed and np.isfinite(run.sums).all()
    w = run.scene.getWorldPtr()
    assert run.scene.n_triangles() == 85 and w.n_quads == 92 and w.n_prims == 0
    p = pkg()
    rays = np.zeros((TW.W * TW.H, 7), F)   # primary rays through the pixel centres
    cam = run.cam
    ys, xs = np.mgrid[0:TW.H, 0:TW.W]
    sx, sy = ((xs + 0.5) / TW.W * 2 - 1).ravel().astype(F), ((ys + 0.5) / TW.H * 2 - 1).ravel().astype(F)
    rays[:, 0:3] = F(list(cam.o))
    rays[:, 3:6] = F(list(cam.w))[None] + F(list(cam.u))[None] * sx[:, None] + F(list(cam.v))[None] * sy[:, None]
    prim = TT.closest_intersection(run.world, rays)[2]
    assert (prim >= 7).mean() > 0.1 and len(np.unique(prim[prim >= 7])) > 20   # the meshes fill a good part of the view
    assert bits_equal(TW.run(as_list=True).sums, run.sums)                      # no tie between two primitives in this room: a list and a tree see the same hits


def test_every_triangle_instantiation_has_a_recipe_in_the_matrix_the_gpu_tests_run():
    """every form of stream_kernel_for()'s TRI family and of its TRI_NEE family is a key of _tri_worlds.FORMS, and nothing else is"""
    for family in ("TRI", "TRI_NEE"):
        keys = KT.family(family)
        assert len(keys) == KT.count(family) == 16 and keys == set(TW.FORMS), family   # (the reader raises on a line of the table it cannot read)
    for (world, exact, ext, big, wide), (variant, env) in TW.FORMS.items():   # the recipes say what stream_kernel_key() makes of them
        assert variant == ({0: 3, 1: 2}[exact] if world == TW.BVH else 0)
        assert env == (TW.LDS, TW.NARROW, TW.WIDE)[big + wide] if world == TW.BVH else env == (TW.NARROW if big else TW.LDS)
    assert len({TW.form_id(f) for f in TW.FORMS}) == 16


# ---- the fuzzer's worlds -------------------------------------------------------------------------------------------------------------------------------
def test_the_fuzzer_builds_its_first_fifty_worlds_on_the_host_and_no_triangles_restores_the_recorded_ones():
    """tests/golden/fuzz_worlds_first50.txt: per seed, the sha256 of the flat world (TW.flat_bytes) that tools/fuzz_campaign.py made before it knew triangles, and
    the next draw of the seed's generator after the world — the campaigns recorded under profiles/ ran those worlds, frames and cameras."""
    import hashlib
    import importlib.util
    p = pkg()
    spec = importlib.util.spec_from_file_location("fuzz_campaign", os.path.join(ROOT, "tools", "fuzz_campaign.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)   # starts nothing
    recorded = [line.split() for line in open(os.path.join(ROOT, "tests", "golden", "fuzz_worlds_first50.txt"))]
    assert [int(r[0]) for r in recorded] == list(range(50))
    with_triangles = tri_lists = meshes = 0
    for seed, digest, next_draw in recorded:
        seed = int(seed)
        s0, kinds0, builder0, big0, rng0 = fuzz.world_of_seed(p, seed, triangles=False)
        assert hashlib.sha256(TW.flat_bytes(s0)).hexdigest() == digest and int(rng0.integers(0, 1 << 30)) == int(next_draw), seed
        s1, kinds1, builder1, big1, rng1 = fuzz.world_of_seed(p, seed)
        assert (kinds1, builder1, big1) == (kinds0, builder0, big0) and int(rng1.integers(0, 1 << 30)) == int(next_draw), seed   # the frame and the camera stay too
        n = s1.n_triangles()
        assert s0.n_triangles() == 0 and (n == 0 or kinds1 >= 1)
        q0, q1 = s0.quads(), s1.quads()
        assert sorted(map(bytes, q1[q1["kind"] == 0])) == sorted(map(bytes, q0))   # the rest of the world is what it was
        assert sorted(map(bytes, s1.arrays()[1])) == sorted(map(bytes, s0.arrays()[1])) and s1.arrays()[2].tobytes() == s0.arrays()[2].tobytes()
        if n == 0:
            assert TW.flat_bytes(s1) == TW.flat_bytes(s0)
        with_triangles += n > 0
        tri_lists += n > 0 and builder1 == 3
        meshes += n > 30
    print(f"{with_triangles} of 50 worlds hold triangles, {meshes} of them a mesh, {tri_lists} are lists")
    assert with_triangles * 3 >= 50 and meshes >= 1
    assert fuzz.parse_args(["--no-triangles", "--seeds", "3"]).no_triangles and not fuzz.parse_args([]).no_triangles
