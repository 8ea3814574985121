"""Smooth shading on the GPU: the probe, every kernel form a world with triangles can resolve to, the light-sampling modes, the feature pass and the
multi-GPU driver with a table of vertex normals on, against the numpy twin (tests/_smooth_twin.py, pinned by tests/test_smooth_normals_cpu.py), bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _smooth_twin as ST
import _smooth_worlds as SW
import _tri_worlds as TW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = SW.W, SW.H, SW.SPP, SW.DEPTH, SW.SEED


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def flat_world(scene):
    """the scene's flat world WITHOUT its table beside it: a renderer made from it starts flat"""
    w = scene.getWorldPtr()
    if hasattr(w, "vertex_normals"):
        del w.vertex_normals
    return w


def setenv(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- 1. the probe --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_probe_on_crafted_hits(p, as_list):
    names, tris, vn, rays6, t, expect = SW.crafted_arrays(p)
    scene = SW.crafted_world(p, as_list)
    world = scene.getWorldPtr()
    oworld = as_oracle_world(world)
    reached = 0
    for i, name in enumerate(names):   # one record per call: the world has one triangle, the case's record is its table
        rays = np.zeros((1, 7), F)
        rays[0, 0:6] = rays6[i]
        hit, normal, took = p.api.probe_shading_normal(world, vn[i:i + 1], rays)
        info = {}
        e_hit, _, e_prim, e_normal = ST.closest_intersection_smooth(oworld, vn[i:i + 1], rays, info=info)
        assert hit[0] == e_hit[0] == 1, name
        assert bits_equal(normal, e_normal), (name, normal, e_normal)
        assert int(took[0]) == info.get("interpolated", 0), name
        reached += int(e_prim[0] == 1)
        if as_list or e_prim[0] == 1:   # past a list's bounds every case reaches the triangle; a BVH leaf's box ends where the triangle ends, and aabb::intersects'
            assert e_prim[0] == 1 and bool(took[0]) == bool(expect[i]), name   # 0 / 0 on a face decides at a vertex or an edge (the twin says which way): the sphere behind
    assert as_list or reached >= 4


@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("n", [0, 1, 127, 128, 129])
def test_probe_shapes_through_the_room(p, monkeypatch, n, form):
    setenv(monkeypatch, TW.NARROW if form == "global" else TW.LDS)
    scene = SW.smooth_room(p)
    world, vn = scene.getWorldPtr(), scene.vertex_normals()
    rays = TW.room_rays(n, seed=40 + n)
    rays[n // 2:, 3:6] = (F([5, 5.2, 6.5]) + (np.random.default_rng(n).random((n - n // 2, 3), dtype=F) - F(0.5)) * F(2)) - rays[n // 2:, 0:3]   # at the smooth icosphere
    hit, normal, took = p.api.probe_shading_normal(world, vn, rays)
    if n == 0:
        assert len(hit) == 0
        return
    info = {}
    e_hit, _, e_prim, e_normal = ST.closest_intersection_smooth(as_oracle_world(world), vn, rays, info=info)
    assert bits_equal(hit.astype(F), e_hit.astype(F)) and bits_equal(normal, e_normal), mismatch_report(normal, e_normal)
    assert int(took.sum()) == info["interpolated"]
    if n >= 127:
        assert info["interpolated"] >= 10
    h0, n0, t0 = p.api.probe_shading_normal(world, None, rays)   # without a table: the flat walk
    assert not t0.any() and bits_equal(n0, ST._flat_walk(as_oracle_world(world), rays)[3])


# ---- 2. all 16 TRI keys, plain and in mode 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["plain", "nee"])
@pytest.mark.parametrize("form", list(TW.FORMS), ids=[TW.form_id(f) for f in TW.FORMS])
def test_every_triangle_instantiation_renders_the_smooth_room_as_the_twin_does(p, monkeypatch, form, mode):
    world, exact, ext, big, wide = form
    variant, env = TW.FORMS[form]
    room = {"as_list": world == TW.LIST, "lamp": True, "textured": ext == 2}
    run = SW.run(mode=mode, **room)
    keep = run.pixel_followed
    assert run.followed if ext == 1 else 0.7 < keep.mean() < 1.0
    setenv(monkeypatch, env)
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # cuts inside the frame: three passes
    scene = SW.smooth_room(p, **room)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, scene.getWorldPtr(), seed=SEED, variant=variant)
    if mode:
        r.light_sampling(mode)
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0) and r.kernel_triangles()
    assert r.shading_normals_info() == {"enabled": True, "smooth": 84}   # 80 + 4 smooth triangles; the table came with the world
    r.Render()
    img = r.DownloadRenderbuffer()
    assert bits_equal(img[keep], run.frame[keep]), mismatch_report(img[keep], run.frame[keep])
    r.refine(3)
    r.refine(5)   # uneven steps
    sums = r.refine_sums()
    assert bits_equal(sums[keep], run.sums[keep]), mismatch_report(sums[keep], run.sums[keep])
    assert bits_equal(r.DownloadRenderbuffer(), img)
    if ext == 2:   # the pixels the twin does not follow (the image-textured triangle): the same bits in every form of the same walk
        key = (world, exact, mode)
        first = _EXT2_SUMS.setdefault(key, sums)
        assert bits_equal(sums, first)
    r.close()


_EXT2_SUMS = {}   # (world, exact, mode) -> the refinement sums of the first EXT 2 form rendered: the LDS form, by FORMS' order


# ---- 3. modes 1, 4 and 16 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("mode", [1, 4, 16])
def test_light_sampling_modes_with_the_table_on(p, monkeypatch, mode, form):
    run = SW.run(mode=mode, lamp=True)
    assert run.followed
    setenv(monkeypatch, TW.NARROW if form == "global" else TW.LDS)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, run.scene.getWorldPtr(), seed=SEED)
    r.light_sampling(mode)
    assert r.light_sampling_mode() == mode and r.kernel_triangles() and r.kernel_form()["big"] == (form == "global")
    assert r.kernel_light_tree() == (mode == 16) and r.shading_normals_info()["enabled"]
    r.refine(SPP)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling(0)   # and back: the plain image with the table behind it
    r.refine(SPP)
    assert bits_equal(r.refine_sums(), SW.run(lamp=True).sums)
    r.close()


# ---- 4. zeros, off, restart ------------------------------------------------------------------------------------------------------------------------------
def test_a_table_of_zeros_is_no_table_and_turning_it_off_gives_the_flat_frame(p):
    run, flat = SW.run(), SW.run(flat=True)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, flat_world(run.scene), seed=SEED)
    assert r.shading_normals_info() == {"enabled": False, "smooth": 0}
    r.refine(SPP)
    none = r.refine_sums()
    assert bits_equal(none, flat.sums), mismatch_report(none, flat.sums)
    r.shading_normals(np.zeros((len(run.vn), 9), F))
    assert r.shading_normals_info() == {"enabled": True, "smooth": 0} and r.refine_info()["samples"] == 0   # a table change restarts the refinement
    r.refine(SPP)
    assert bits_equal(r.refine_sums(), none)
    r.shading_normals(run.vn)
    assert r.shading_normals_info() == {"enabled": True, "smooth": 84} and r.refine_info()["samples"] == 0
    r.refine(2)
    r.shading_normals(run.vn)   # the same table: nothing changes, the refinement goes on
    assert r.refine_info()["samples"] == 2
    r.refine(SPP - 2)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.shading_normals(None)
    assert r.shading_normals_info() == {"enabled": False, "smooth": 0} and r.refine_info()["samples"] == 0
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), flat.frame)
    r.close()


# ---- 5. index boundaries ------------------------------------------------------------------------------------------------------------------------------------
BW, BH, BSPP, BDEPTH = 24, 16, 4, 4   # small frames: the twin walks a list of 5300 primitives one primitive at a time


def boundary_frame(which):
    return (16, 8, 2, 3) if which == "icosphere4" else (BW, BH, BSPP, BDEPTH)


def boundary_scene(p, which, builder):
    m = TW.mesh_io()
    s = p.Scene()
    grey, red, mirror = s.Lambertian((0.6, 0.6, 0.6)), s.Lambertian((0.7, 0.2, 0.2)), s.Metal((0.8, 0.8, 0.8), 0.05)
    if which == "triangles_only":   # n_plain_quads == 0, no spheres
        s.set_background((0.6, 0.7, 0.9))
        s.MakeTriangle((-6, 0, -6), (6, 0, -6), (-6, 0, 6), grey)
        s.MakeTriangle((6, 0, 6), (-6, 0, 6), (6, 0, -6), grey, normals=[(0.1, 1, 0), (0, 1, 0.1), (-0.1, 1, 0)])
        v, f = m.icosphere(1)
        s.MakeMesh(v, f, mirror, 1.2, 0.0, (-1.5, 1.3, 0), normals=m.icosphere_normals(1))
        tv, tf = m.tetrahedron()
        s.MakeMesh(tv, tf, red, 1.3, 10.0, (1.8, 1.0, 0.5), normals=m.vertex_normals(tv, tf))
        cam = TW.boundary_camera(p, BW, BH)
    elif which == "siblings":   # one parallelogram and one smooth triangle: the two leaves of the root
        s.set_background((0.6, 0.7, 0.9))
        s.MakeQuad((-2.5, 0, 0), (2, 0, 0), (0, 2.4, 0.2), red)
        s.MakeTriangle((0.2, 0, 0), (2.8, 0, 0.2), (1.2, 2.8, 0), grey, normals=[(-0.5, 0, 1), (0.5, 0, 1), (0, 0.5, 1)])
        cam = TW.boundary_camera(p, BW, BH)
    else:
        assert which == "icosphere4"   # 5120 smooth triangles in the room: the global-memory form with nothing forced
        v, f = m.icosphere(4)
        return SW.smooth_room(p, more=lambda sc: sc.MakeMesh(v, f, sc.Lambertian((0.8, 0.4, 0.3)), 1.1, 0.0, (7.5, 7.0, 5.5), normals=m.icosphere_normals(4)),
                              as_list=builder == "MakeHittableList"), TW.camera(p, *boundary_frame(which)[:2])
    getattr(s, builder)()
    return s, cam


@functools.lru_cache(maxsize=None)
def boundary_sums(which, as_list):
    p = pkg()
    s, cam = boundary_scene(p, which, "MakeHittableList" if as_list else "BuildBVH_SAH")
    w, h, spp, depth = boundary_frame(which)
    samples, followed = ST.frame_samples(as_oracle_world(s.getWorldPtr()), s.vertex_normals(), as_oracle_camera(cam), w, h, spp, depth, SEED)
    assert followed.all()
    return ST.in_order_sums(samples)


@pytest.mark.parametrize("walk", ["exact", "fast", "list"])
@pytest.mark.parametrize("which", ["triangles_only", "siblings", "icosphere4"])
def test_index_boundaries(p, which, walk):
    as_list = walk == "list"
    s, cam = boundary_scene(p, which, "MakeHittableList" if as_list else "BuildBVH_SAH")
    quads = s.quads()
    if which == "triangles_only":
        assert (quads["kind"] == 1).all() and s.getWorldPtr().n_prims == 0
    if which == "siblings" and not as_list:
        assert TW.sibling_leaves(s) == [(0, 1)] or TW.sibling_leaves(s) == [(1, 0)]
    w, h, spp, depth = boundary_frame(which)
    r = p.Renderer.MakeRenderer(w, h, spp, depth, cam, s.getWorldPtr(), seed=SEED, variant=0 if as_list else (2 if walk == "exact" else 3))
    form = r.kernel_form()
    assert r.kernel_triangles() and r.shading_normals_info()["enabled"] and form["exact"] == (walk != "fast")
    if which == "icosphere4":
        assert form["big"] == 1   # beyond the LDS by itself
    r.refine(spp)
    exp = boundary_sums(which, as_list)
    assert bits_equal(r.refine_sums(), exp), mismatch_report(r.refine_sums(), exp)
    r.close()


# ---- 6. feature buffers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_feature_buffers_hold_the_shading_normal(p, as_list):
    run = SW.run(as_list=as_list)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, run.scene.getWorldPtr(), seed=SEED)
    r.enable_aov()
    r.refine(1)
    r.refine(SPP - 1)
    got = r.aov_sums()
    exp = ST.first_hit_sums(run.world, run.vn, as_oracle_camera(run.cam), W, H, SPP, SEED)
    assert bits_equal(got[..., 0:4], exp[..., 0:4]), mismatch_report(got[..., 0:4], exp[..., 0:4])
    den = r.denoise()
    assert np.isfinite(den).all()
    r.shading_normals(None)
    r.refine(SPP)
    flat = r.aov_sums()
    assert bits_equal(got[..., 3:8], flat[..., 3:8])          # depth, albedo and coverage do not know the table
    assert not bits_equal(got[..., 0:3], flat[..., 0:3])      # the normal does
    r.close()


# ---- 7. ranks ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 3])
def test_ranks_through_the_memcpy_transport(p, monkeypatch, ranks):
    run = SW.run()
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, run.scene.getWorldPtr(), ranks, seed=SEED)
    m.Render()
    img = m.DownloadRenderbuffer()
    assert bits_equal(img, run.frame), mismatch_report(img, run.frame)
    m.shading_normals(None)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), SW.run(flat=True).frame)
    m.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point_and_leave_the_renderer_flat(p):
    run, flat = SW.run(), SW.run(flat=True)
    vn = ST.table(run.vn).reshape(-1, 9)
    nan, one_zero = vn.copy(), vn.copy()
    nan[5, 4] = np.nan
    smooth_row = int(np.nonzero((vn != 0).any(axis=1))[0][0])
    one_zero[smooth_row, 3:6] = 0
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, flat_world(run.scene), seed=SEED)
    for bad in (vn[:-1], np.concatenate([vn, vn[:1]]), nan, one_zero):
        with pytest.raises(p.capi.RtError, match="rt_renderer_shading_normals") as e:
            r.shading_normals(bad)
        assert e.value.code == 1   # RT_ERR_INVALID
    assert not r.shading_normals_info()["enabled"]
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), flat.frame)
    r.close()
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, flat_world(run.scene), seed=SEED, variant=1)
    with pytest.raises(p.capi.RtError, match="rt_renderer_shading_normals.*variant 1") as e:
        r.shading_normals(vn)
    assert e.value.code == 1
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), flat.frame)
    r.close()
    for traversal in (1, 2):
        s = SW.smooth_room(p, traversal=traversal)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, flat_world(s), seed=SEED)
        with pytest.raises(p.capi.RtError, match="rt_renderer_shading_normals.*traversal") as e:
            r.shading_normals(s.vertex_normals())
        assert e.value.code == 1
        r.close()
        with pytest.raises(p.capi.RtError, match="rt_renderer_shading_normals"):   # Renderer pushes the scene's table at creation: the refusal surfaces there
            p.Renderer.MakeRenderer(W, H, SPP, DEPTH, run.cam, s.getWorldPtr(), seed=SEED)


# ---- 9. what it is for -------------------------------------------------------------------------------------------------------------------------------------
def test_a_smooth_icosphere_looks_more_like_the_sphere_than_the_flat_one(p):
    """mean |normal AOV - the analytic sphere's| over the pixels both cover fully: smaller for the smooth mesh than for the flat one (an ordering, not a threshold)"""
    m = TW.mesh_io()
    v, f = m.icosphere(3)
    c, radius, w, h, spp = (0, 1.5, 0), 1.5, 64, 64, 4
    cam = p.PinholeCamera((0, 1.5, 6), (0, 1.5, 0), (0, 1, 0), 35.0, 1.0)
    out = {}
    for name in ("sphere", "flat", "smooth"):
        s = p.Scene()
        blue = s.Lambertian((0.3, 0.5, 0.8))
        s.set_background((0.6, 0.7, 0.9))
        s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), s.Lambertian((0.6, 0.6, 0.6)))
        if name == "sphere":
            s.MakeSphere(c, radius, blue)
        else:
            s.MakeMesh(v, f, blue, radius, 0.0, c, normals=m.icosphere_normals(3) if name == "smooth" else None)
        s.BuildBVH_SAH()
        r = p.Renderer.MakeRenderer(w, h, spp, 4, cam, s.getWorldPtr(), seed=SEED)
        r.enable_aov()
        r.refine(spp)
        a = r.aov()
        out[name] = (a["normal"], a["depth"])
        r.close()
    # pixels whose every sample meets the object in all three frames: nearer than the floor behind it (depth is in units of the primary ray's length)
    on = np.ones((h, w), bool)
    for name in out:
        n = out[name][0]
        on &= np.abs(np.linalg.norm(n, axis=2) - 1) < 0.05   # a pixel that mixes floor and object has a shorter mean normal
        on &= n[..., 2] > 0.2                                   # facing the camera: the object, not the floor
    assert on.sum() > 300
    d_flat = float(np.abs(out["flat"][0][on] - out["sphere"][0][on]).mean())
    d_smooth = float(np.abs(out["smooth"][0][on] - out["sphere"][0][on]).mean())
    print(f"normal AOV against the analytic sphere over {int(on.sum())} pixels: flat icosphere(3) {d_flat:.5f}, smooth icosphere(3) {d_smooth:.5f}")
    assert d_smooth < d_flat


# ---- 10. beyond the twin: glass ----------------------------------------------------------------------------------------------------------------------------
def test_a_glass_smooth_icosphere_has_the_same_bits_in_every_form_and_walk(p, monkeypatch):
    m = TW.mesh_io()
    v, f = m.icosphere(1)

    def glass(s):
        s.MakeMesh(v, f, s.Dielectric((1, 1, 1), 1.5), 1.4, 0.0, (5, 4.2, 4.5), normals=m.icosphere_normals(1))
    frames = []
    for env in (TW.LDS, TW.NARROW):
        for variant in (2, 3):
            setenv(monkeypatch, env)
            s = SW.smooth_room(p, more=glass)
            r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, SW.camera(p), s.getWorldPtr(), seed=SEED, variant=variant)
            form = r.kernel_form()
            assert form["big"] == (env is TW.NARROW) and form["exact"] == (variant == 2) and r.shading_normals_info()["smooth"] == 164
            r.refine(SPP)
            frames.append(r.refine_sums())
            r.close()
    for other in frames[1:]:
        assert bits_equal(frames[0], other)
    assert np.isfinite(frames[0]).all() and not bits_equal(frames[0], SW.run().sums)


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_app_renders_the_frame_python_renders(p):
    def fnv1a(data):
        h = 1469598103934665603
        for b in data:
            h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
        return h
    w, h, spp, depth = 40, 24, 4, 5
    d = os.path.join(ROOT, "tests", "cpp_smooth")
    out = subprocess.check_output([os.path.join(d, "smooth_app"), str(w), str(h), str(spp), str(depth)], text=True, timeout=120)
    s = p.Scene()
    white, blue = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.3, 0.5, 0.8))
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), white)
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    f = np.array([0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5], np.uint32).reshape(-1, 3)
    s.MakeMesh(v, f, blue, 1.5, 20.0, (0, 1.8, 0), normals=v)
    s.MakeTriangle((-3, 0.1, -2), (-1.5, 0.1, -2.5), (-2.5, 2, -2), white, normals=[(0, 0.3, 1), (0.3, 0, 1), (-0.3, 0, 1)])
    s.set_background((0.6, 0.7, 0.9))
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(w, h, spp, depth, p.PinholeCamera((0.5, 2.5, 7), (0, 1.5, 0), (0, 1, 0), 50.0, w / h), s.getWorldPtr(), seed=1984)
    assert r.shading_normals_info() == {"enabled": True, "smooth": 9}
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.close()
    assert out.strip() == f"smooth {w}x{h} spp={spp} depth={depth} fnv={fnv1a(frame.tobytes()):016x}"


def test_render_tool_smooth_writes_the_api_frame_as_png(p, tmp_path):
    import json
    import sys
    out = tmp_path / "smooth.png"
    args = ["--scene", "cornell_box", "--width", "32", "--height", "32", "--spp", "4", "--depth", "8", "--mesh", "icosphere:2", "--mesh-scale", "80",
            "--mesh-rotate-y", "10", "--mesh-translate", "278,278,200", "--mesh-material", "metal", "--smooth", "--out", str(out)]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py")] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert lines[0] == {"mesh": "icosphere:2", "triangles": 320, "skipped_degenerate": 0}
    m = TW.mesh_io()
    frames = {}
    for smooth in (False, True):
        s = p.Scene.cornell_box()
        s.MakeMesh(*m.icosphere(2), s.Metal((0.8, 0.85, 0.88), 0.0), 80.0, 10.0, (278, 278, 200), normals=m.icosphere_normals(2) if smooth else None)
        s.BuildBVH_TopDown()
        r = p.Renderer.MakeRenderer(32, 32, 4, 8, p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0), s.getWorldPtr(), seed=1984)
        assert r.shading_normals_info()["enabled"] == smooth
        r.Render()
        frames[smooth] = r.DownloadRenderbuffer()
        r.close()
    from ray_tracing_v06_amd import image_io
    expected = tmp_path / "api.png"
    image_io.write_png(str(expected), frames[True])
    assert out.read_bytes() == expected.read_bytes() and not bits_equal(frames[True], frames[False])
