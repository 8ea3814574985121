"""Smooth shading without a GPU: the twin's pins, the kernels' own function on the host against the twin, the mathematics no kernel shares, the
scene's bookkeeping of vertex normals through everything that permutes triangles, the OBJ reader and the generators, and the ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import _smooth_twin as ST
import _smooth_worlds as SW
import _tri_twin as TT
import _tri_worlds as TW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

F = np.float32


# ---- 1. pins: with a table of zeros the twin IS _tri_twin ---------------------------------------------------------------------------------------------
def test_pin_an_all_zero_table_is_the_flat_twin_bit_for_bit():
    p = pkg()
    scene = TW.tri_room(p)
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(TW.camera(p))
    zeros = np.zeros((scene.n_triangles(), 3, 3), F)
    rays = TW.room_rays(600)
    for got, exp in zip(ST.closest_intersection_smooth(world, zeros, rays), TT.closest_intersection(world, rays)):
        assert bits_equal(np.asarray(got, F), np.asarray(exp, F))
    gids = np.repeat(np.arange(TW.W * TW.H, dtype=np.uint32), TW.SPP)
    smp = np.tile(np.arange(TW.SPP, dtype=np.uint32), TW.W * TW.H)
    lamp = TW.tri_room(p, lamp=True)
    for mode, room in ((0, world), (1, world), (2, as_oracle_world(lamp.getWorldPtr()))):
        got, ok = ST.radiance(room, zeros, cam, TW.W, TW.H, TW.DEPTH, TW.SEED, gids, smp, mode)
        exp, ok2 = TT.radiance(room, cam, TW.W, TW.H, TW.DEPTH, TW.SEED, gids, smp, mode)
        assert ok.all() and ok2.all() and bits_equal(got, exp), mismatch_report(got, exp)
    assert TT.closest_intersection is ST._flat_walk   # the substitution is undone


# ---- 2. rt_shading_normal_batch — the kernels' function on the host — equals the twin ------------------------------------------------------------------
def _random_hits(p, n, seed=5):
    """n hits on random triangles with random unit vertex normals (all three within 60 degrees of the face normal, on either side of the face)"""
    rng = np.random.default_rng(seed)
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    n_tri = 64
    for _ in range(n_tri):
        a = (rng.random(3) * 8 - 4).astype(F)
        s.MakeTriangle(a, a + (rng.standard_normal(3) * 1.5).astype(F), a + (rng.standard_normal(3) * 1.5).astype(F), m)
    s.MakeHittableList()
    quads = s.quads()
    pick = rng.integers(0, n_tri, n)
    tris = quads[pick]
    fn = tris["normal"].astype(np.float64) * rng.choice([-1.0, 1.0], n)[:, None]
    vn = fn[:, None, :] + rng.standard_normal((n, 3, 3)) * 0.6
    vn = (vn / np.linalg.norm(vn, axis=2, keepdims=True)).astype(F)
    a, b = rng.random(n), rng.random(n)
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    target = tris["Q"].astype(np.float64) + tris["u"].astype(np.float64) * a[:, None] + tris["v"].astype(np.float64) * b[:, None]
    origin = (target + rng.standard_normal((n, 3)) * 3).astype(F)
    d = (target - origin.astype(np.float64)).astype(F)
    # the hit distance as quad::hit computes it: t = (D - dot(n, o)) / dot(n, d)
    nrm = tris["normal"].astype(F)
    with np.errstate(all="ignore"):
        t = (tris["D"].astype(F) - ST.dot(nrm, origin)) / ST.dot(nrm, d)
    return tris, vn, np.concatenate([origin, d], axis=1).astype(F), t.astype(F)


def test_the_host_entry_point_equals_the_twin_on_random_hits():
    p = pkg()
    tris, vn, rays, t = _random_hits(p, 4096)
    normal, took = p.api.shading_normal_batch(tris, vn, rays, t)
    exp_n, exp_took, fb = ST.shading_normal(tris, vn, rays[:, 0:3], rays[:, 3:6], t)
    assert bits_equal(normal, exp_n), mismatch_report(normal, exp_n)
    assert (took.astype(bool) == exp_took).all()
    assert exp_took.sum() > 2000 and (fb == 2).sum() > 100   # both outcomes are exercised
    with np.errstate(all="ignore"):
        assert (ST.dot(rays[:, 3:6], normal) <= 0).all()     # the invariant: the normal faces against the ray (<= : a flat normal may be met edge-on)


def test_the_host_entry_point_equals_the_twin_on_crafted_hits():
    p = pkg()
    names, tris, vn, rays, t, expect = SW.crafted_arrays(p)
    normal, took = p.api.shading_normal_batch(tris, vn, rays, t)
    exp_n, exp_took, fb = ST.shading_normal(tris, vn, rays[:, 0:3], rays[:, 3:6], t)
    assert bits_equal(normal, exp_n), mismatch_report(normal, exp_n)
    for i, name in enumerate(names):
        assert bool(took[i]) == bool(exp_took[i]) == bool(expect[i]), name
    by = dict(zip(names, range(len(names))))
    assert fb[by["n0 == -n1 at the midpoint of ab: l2 == 0"]] == 1 and fb[by["an all-zero record"]] == 1 and fb[by["a NaN component"]] == 1
    assert fb[by["grazing, normals tilting away"]] == 2
    for k, v in (("vertex a", 0), ("vertex b", 1), ("vertex c", 2)):   # at a vertex the normal is that vertex's, up to its own normalisation
        assert np.allclose(normal[by[k]], SW.TILTED[v], atol=2e-7)
    assert normal[by["back face"]][2] < 0 and bits_equal(normal[by["back face"]], -normal[by["inside"]])
    flat = [by[k] for k in names if not expect[by[k]]]
    assert bits_equal(normal[flat], np.tile(F([0, 0, 1]), (len(flat), 1)))


# ---- 3. mathematics no kernel shares -------------------------------------------------------------------------------------------------------------------
MEASURED_F32_VS_F64 = 1.573e-7         # the largest |float32 twin - float64 rule| over the hits below, measured here on the CPU (L = 1: 1.297e-7, 2: 1.281e-7, 3: 1.573e-7)
TOLERANCE_F32_VS_F64 = 4 * MEASURED_F32_VS_F64   # times 4: hits at small l2 or grazing incidence condition worse than this sample shows


@pytest.mark.parametrize("level", [1, 2, 3])
def test_on_a_sphere_the_interpolated_normal_is_the_direction_from_the_centre(level):
    """vertices on a sphere about c with n_i = unit(v_i - c): g = hit point - c (over the radius), exactly, in real arithmetic — so the float64 rule must give
    unit(hit_p - c) to 1e-12, and the float32 twin must agree with the float64 rule within the tolerance above"""
    p = pkg()
    m = TW.mesh_io()
    v, f = m.icosphere(level)
    c, radius = np.array([0.5, -1.0, 2.0]), 1.5
    s = p.Scene()
    s.MakeMesh(v, f, s.Lambertian((0.5, 0.5, 0.5)), radius, 0.0, c, normals=m.icosphere_normals(level))
    s.MakeHittableList()
    quads, vn = s.quads(), ST.table(s.vertex_normals())
    rng = np.random.default_rng(level)
    n = 2000
    pick = rng.integers(0, len(quads), n)
    a, b = rng.random(n), rng.random(n)
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    Q, u, w_ = (quads[k][pick].astype(np.float64) for k in ("Q", "u", "v"))
    hit_p = Q + u * a[:, None] + w_ * b[:, None]
    origin = c + (hit_p - c) * 3 + rng.standard_normal((n, 3)) * 0.5      # outside, roughly radially: the outward normal faces the ray
    d = hit_p - origin
    # exact in real arithmetic: with the exact vertex normals (v_i - c) / r the float64 rule gives unit(hit_p - c)
    n_exact = [(Q - c) / radius, (Q + u - c) / radius, (Q + w_ - c) / radius]
    n64, took64, g = ST.shading_normal64(Q, u, w_, *n_exact, d, hit_p)
    assert took64.all()
    assert np.abs(g - (hit_p - c) / radius).max() < 1e-12
    assert np.abs(n64 - (hit_p - c) / np.linalg.norm(hit_p - c, axis=1, keepdims=True)).max() < 1e-12
    # the float32 twin on the scene's own records against the float64 rule on the same float32 inputs
    tris, rec = quads[pick], vn[pick]
    o32, d32 = origin.astype(F), d.astype(F)
    nrm = tris["normal"].astype(F)
    with np.errstate(all="ignore"):
        t32 = ((tris["D"].astype(F) - ST.dot(nrm, o32)) / ST.dot(nrm, d32)).astype(F)
    n32, took32, _ = ST.shading_normal(tris, rec, o32, d32, t32)
    hp32 = o32.astype(np.float64) + d32.astype(np.float64) * t32.astype(np.float64)[:, None]
    ref, took_ref, _ = ST.shading_normal64(tris["Q"], tris["u"], tris["v"], rec[:, 0], rec[:, 1], rec[:, 2], d32, hp32)
    assert took32.all() and took_ref.all()
    err = np.abs(n32.astype(np.float64) - ref).max()
    print(f"icosphere({level}): max |float32 twin - float64 rule| = {err:.3e}")
    assert err <= TOLERANCE_F32_VS_F64, err


# ---- 4. host bookkeeping -------------------------------------------------------------------------------------------------------------------------------
def _bookkeeping_scene(p, builder):
    """parallelograms, free flat triangles, a smooth mesh and a smooth triangle, then a LATE parallelogram; returns the scene and {vertex bytes: (3, 3) normals}"""
    m = TW.mesh_io()
    s = p.Scene()
    grey = s.Lambertian((0.5, 0.5, 0.5))
    s.MakeQuad((-5, 0, -5), (10, 0, 0), (0, 0, 10), grey)
    s.MakeSphere((3, 1, 3), 1.0, grey)
    s.MakeTriangle((-4, 0.1, -3), (-2, 0.1, -3.5), (-3, 2, -3), grey)
    v, f = m.icosphere(1)
    nrm = m.icosphere_normals(1)
    s.MakeMesh(v, f, grey, 1.2, 0.0, (0, 1.5, 0), normals=nrm)
    s.MakeTriangle((2, 0.1, -3), (4, 0.1, -3.5), (3, 2, -3), grey)
    tn = np.array([[0, 0.6, 0.8], [0.6, 0, 0.8], [0, 0, 1]], F)
    s.MakeTriangle((-1, 0.1, 3), (1, 0.1, 3.5), (0, 2, 3), grey, normals=tn)
    s.MakeQuad((-5, 0, -5), (10, 0, 0), (0, 6, 0), grey)   # late: it goes in front of every triangle
    getattr(s, builder)()
    expected = {}
    pts = (v * F(1.2) + F([0, 1.5, 0])).astype(F)   # rotation 0: rot_y leaves x and z as they are (c = 1, sn = 0: c * x + 0 * z)
    for face in f:
        expected[pts[face].tobytes()] = nrm[face]
    expected[np.array([(-1, 0.1, 3), (1, 0.1, 3.5), (0, 2, 3)], F).tobytes()] = tn
    return s, expected


@pytest.mark.parametrize("builder", TW.BUILDERS)
def test_record_i_belongs_to_triangle_i_of_the_flat_world(builder):
    p = pkg()
    s, expected = _bookkeeping_scene(p, builder)
    quads, vn = s.quads(), ST.table(s.vertex_normals())
    tris = quads[quads["kind"] == 1]
    assert len(vn) == len(tris) == 80 + 3 == s.n_triangles() and (quads["kind"][:2] == 0).all()
    n_smooth = 0
    for q, rec in zip(tris, vn):
        verts = np.stack([q["Q"], q["Q"] + q["u"], q["Q"] + q["v"]]).astype(F)
        key = min(expected, key=lambda k: np.abs(np.frombuffer(k, F).reshape(3, 3) - verts).max())
        if np.abs(np.frombuffer(key, F).reshape(3, 3) - verts).max() < 1e-5:   # b = Q + (b - Q) is not b to the bit
            exp = expected[key].astype(np.float64)
            exp = exp / np.linalg.norm(exp, axis=1, keepdims=True)
            assert np.abs(rec - exp).max() < 2e-7
            n_smooth += 1
        else:
            assert (rec == 0).all()   # a flat triangle has a zero record
    assert n_smooth == 81


def test_a_failed_smooth_mesh_leaves_the_scene_unchanged_and_a_flat_scene_has_no_table():
    p = pkg()
    m = TW.mesh_io()
    s, _ = _bookkeeping_scene(p, "BuildBVH_SAH")
    grey = s.Lambertian((0.1, 0.1, 0.1))
    before, table = TW.flat_bytes(s), s.vertex_normals().tobytes()
    v, f = m.tetrahedron()
    nrm = m.vertex_normals(v, f)
    for bad_normals, bad_faces, why in ((nrm, f + np.uint32(2), "normal index"), (np.concatenate([nrm[:3], np.zeros((1, 3), F)]), None, "zero length"),
                                         (np.concatenate([nrm[:3], F([[np.inf, 0, 0]])]), None, "not finite")):
        with pytest.raises(p.capi.RtError, match="rt_scene_add_mesh_smooth.*" + why.split()[0]):
            s.MakeMesh(v, f, grey, 1.0, 0.0, (0, 5, 0), normals=bad_normals, normal_faces=bad_faces)
        assert TW.flat_bytes(s) == before and s.vertex_normals().tobytes() == table
    flat = TW.tri_room(p)
    assert len(flat.vertex_normals()) == 0 and not hasattr(flat.getWorldPtr(), "vertex_normals")
    assert len(s.getWorldPtr().vertex_normals) == 83


def test_a_rotated_meshs_normals_are_the_rotation_of_the_inputs():
    p = pkg()
    m = TW.mesh_io()
    v, f = m.icosphere(0)
    s = p.Scene()
    deg = 30.0
    s.MakeMesh(v, f, s.Lambertian((0.5, 0.5, 0.5)), 2.5, deg, (1, 2, 3), normals=v * F(3))   # not unit: normalised on the host; not scaled, not translated
    s.MakeHittableList()
    vn = ST.table(s.vertex_normals())
    c, sn = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    rot = np.stack([c * v[:, 0] + sn * v[:, 2], v[:, 1], -sn * v[:, 0] + c * v[:, 2]], axis=1).astype(np.float64)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    assert np.abs(vn - rot[f.astype(np.int64)]).max() < 3e-7
    assert np.abs(np.linalg.norm(vn.astype(np.float64), axis=2) - 1).max() < 2e-7


# ---- the GPU tests' base world: what the twin says of it ---------------------------------------------------------------------------------------------
def test_the_base_world_interpolates_most_hits_and_takes_both_fallbacks():
    run = SW.run()
    info = run.info
    print(info)
    assert run.followed
    assert info["interpolated"] * 2 >= info["smooth"] > 1000
    assert info["fallback1"] >= 20 and info["fallback2"] >= 20
    assert not bits_equal(run.sums, SW.run(flat=True).sums)


# ---- 5. the OBJ reader and the generators ------------------------------------------------------------------------------------------------------------
def test_load_obj_normals_reads_vn_and_the_third_index(tmp_path):
    m = TW.mesh_io()
    text = {
        "slashes.obj": "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvn 0 1 0\nf 1//1 2//2 3//1\n",
        "full.obj": "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nvn 1 0 0\nf 1/1/2 2/1/1 3/1/2\n",
        "negative.obj": "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvn 0 1 0\nvn 1 0 0\nf -3//-1 -2//-3 -1//-2\n",
        "fan.obj": "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvn 0 0 2\nvn 0 0 3\nvn 0 0 4\nf 1//1 2//2 3//3 4//4\n",
        "plain.obj": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
    }
    for name, body in text.items():
        (tmp_path / name).write_text(body)
    v, f, n, nf = m.load_obj_normals(str(tmp_path / "slashes.obj"))
    assert f.tolist() == [[0, 1, 2]] and nf.tolist() == [[0, 1, 0]] and n.tolist() == [[0, 0, 1], [0, 1, 0]] and n.dtype == F and nf.dtype == np.uint32
    v, f, n, nf = m.load_obj_normals(str(tmp_path / "full.obj"))
    assert nf.tolist() == [[1, 0, 1]] and len(n) == 2
    v, f, n, nf = m.load_obj_normals(str(tmp_path / "negative.obj"))
    assert f.tolist() == [[0, 1, 2]] and nf.tolist() == [[2, 0, 1]]
    v, f, n, nf = m.load_obj_normals(str(tmp_path / "fan.obj"))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3]] and nf.tolist() == [[0, 1, 2], [0, 2, 3]]
    v, f, n, nf = m.load_obj_normals(str(tmp_path / "plain.obj"))
    assert n is None and nf is None and f.tolist() == [[0, 1, 2]]
    for name in text:   # load_obj keeps its signature and what it returns
        v0, f0 = m.load_obj(str(tmp_path / name))
        v1, f1, _, _ = m.load_obj_normals(str(tmp_path / name))
        assert v0.tobytes() == v1.tobytes() and f0.tobytes() == f1.tobytes()
    (tmp_path / "bad.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//2 3//1\n")
    with pytest.raises(ValueError, match="normal index"):
        m.load_obj_normals(str(tmp_path / "bad.obj"))


def test_vertex_normals_of_a_tetrahedron_and_of_an_icosphere():
    m = TW.mesh_io()
    v, f = m.tetrahedron()
    n = m.vertex_normals(v, f)
    assert n.dtype == F and np.abs(n - v).max() < 1e-6   # by symmetry: the unit positions
    v, f = m.icosphere(1)
    assert np.abs(m.vertex_normals(v, f) - v).max() < 1e-6
    assert bits_equal(m.icosphere_normals(1), v)
    assert m.vertex_normals(np.zeros((4, 3), F), np.array([[0, 1, 2]], np.uint32)).tolist() == [[0, 0, 1]] * 4   # nothing to weigh: a fixed unit vector


# ---- 6. the ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_of_the_vertex_normals():
    p = pkg()
    assert p.capi.TRI_NORMALS_DT.itemsize == 36 and p.capi.QUAD_DT.itemsize == 80
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in ("rt_scene_add_triangle_smooth", "rt_scene_add_mesh_smooth", "rt_scene_vertex_normals", "rt_shading_normal_batch", "rt_renderer_shading_normals",
                 "rt_renderer_shading_normals_info", "rt_multi_renderer_shading_normals", "rt_probe_shading_normal"):
        assert name in declared and name in p.capi.SYMBOLS and getattr(p.lib(), name).argtypes, name
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert "void SetShadingNormals(" in hpp and "rt_scene_add_mesh_smooth" in hpp and "rt_scene_add_triangle_smooth" in hpp
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])   # as the other ABI tests do: the check is built where it is missing
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_smooth")])
    out = subprocess.check_output([os.path.join(ROOT, "tests", "cpp_smooth", "smooth_abi_check")], text=True)
    assert out.strip() == "smooth ABI ok"
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp_smooth", "smooth_app")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: smooth_app" in r.stderr


def test_the_kernels_share_one_rule_and_the_parameter_blocks_keep_their_fields():
    """the rule is one RT_HD function; StreamParams and PackedSceneRef carry nothing new for it (the table rides behind the image)"""
    csrc = os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")
    funcs = open(os.path.join(csrc, "rt_device_funcs.hpp")).read()
    assert len(re.findall(r"RT_HD bool shading_normal\(", funcs)) == 1
    for name in ("rt_stream_kernel.hpp", "rt_aov_kernel.hpp", "rt_probes.hip"):
        assert "shading_normal" in open(os.path.join(csrc, name)).read(), name
    layout = open(os.path.join(csrc, "rt_layout.hpp")).read()
    stream = open(os.path.join(csrc, "rt_stream_kernel.hpp")).read()
    for block in (layout[layout.index("struct PackedSceneRef {"):layout.index("};", layout.index("struct PackedSceneRef {"))],
                  stream[stream.index("struct StreamParams {"):stream.index("};", stream.index("struct StreamParams {"))]):
        assert "normals" not in block and "vn" not in block
