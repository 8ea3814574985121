"""Texture coordinates on the GPU: the probe, the eight TRI && EXT 2 kernel keys, the light-sampling modes, ranks, the table beside the
vertex normals, refusals and restarts, with a table of texture coordinates on.  Every comparison is bit for bit: against the numpy twin
(tests/_uv_twin.py, pinned by tests/test_texture_coords_cpu.py), against the oracle where a stand-in world exists, and between forms where nothing absolute does."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _smooth_twin as ST
import _tri_worlds as TW
import _uv_twin as UT
import _uv_worlds as UW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = UW.W, UW.H, UW.SPP, UW.DEPTH, UW.SEED
EXT2 = UW.EXT2_FORMS
EXT2_IDS = [TW.form_id(f) for f in EXT2]


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def bare_world(scene, keep=()):
    """the scene's flat world without the tables beside it (but those named in keep): a renderer made from it starts without them"""
    w = scene.getWorldPtr()
    for name in ("vertex_normals", "texture_coords"):
        if name not in keep and hasattr(w, name):
            delattr(w, name)
    return w


def setenv(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def renderer(p, scene, form, world=None, w=W, h=H, spp=SPP, depth=DEPTH, cam=None):
    variant, _ = TW.FORMS[form]
    r = p.Renderer.MakeRenderer(w, h, spp, depth, cam if cam is not None else UW.camera(p), world if world is not None else scene.getWorldPtr(), seed=SEED, variant=variant)
    assert r.kernel_form() == TW.kernel_form_of(form) and r.kernel_triangles()
    return r


def frame_of(r):
    r.Render()
    return r.DownloadRenderbuffer()


# ---- 8. the probe ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_probe_equals_the_twin_on_the_rooms_rays(p, monkeypatch, as_list, form):
    setenv(monkeypatch, TW.NARROW if form == "global" else TW.LDS)
    scene = UW.uv_room(p, as_list=as_list)
    world, uv = scene.getWorldPtr(), scene.texture_coords()
    tab = UT.table(uv)
    n = 257
    rays = TW.room_rays(n, seed=23)
    rays[n // 2:, 3:6] = (F(UW.SPHERE_AT["translate"]) + (np.random.default_rng(2).random((n - n // 2, 3), dtype=F) - F(0.5)) * F(2.6)) - rays[n // 2:, 0:3]   # at the sphere
    extra = np.zeros((2, 7), F)   # the index boundaries: one ray each at the centroid of the FIRST triangle of the flat world (qi == n_plain_quads) and of the LAST
    quads = scene.quads()
    tris = quads[quads["kind"] == 1]
    for k, q in enumerate((tris[0], tris[-1])):
        c = q["Q"] + (q["u"] + q["v"]) / F(3)
        extra[k, 0:3] = c + q["normal"] * F(0.05)
        extra[k, 3:6] = -q["normal"]
    rays = np.concatenate([rays, extra])
    hit, got = p.api.probe_tri_uv(world, uv, rays)
    e_hit, _, e_prim, want = UT.closest_intersection_uv(as_oracle_world(world), uv, rays)
    assert bits_equal(hit.astype(F), e_hit.astype(F)) and bits_equal(got, want), mismatch_report(got, want)
    first_tri = world.n_prims + world.n_quads - len(tab)
    assert e_prim[-2] == first_tri and e_prim[-1] == world.n_prims + world.n_quads - 1   # both boundary triangles were met
    on_sphere = (e_hit != 0) & (e_prim >= first_tri) & (tab[np.maximum(e_prim - first_tri, 0)] != UT.IDENTITY).any(axis=(1, 2))
    assert on_sphere.sum() >= 30 and ((got[on_sphere] < 0) | (got[on_sphere] > 1)).any()
    h0, planar = p.api.probe_tri_uv(world, None, rays)   # without a table: the planar coordinates everywhere
    assert bits_equal(planar, UT.closest_intersection_uv(as_oracle_world(world), None, rays)[3])
    assert len(p.api.probe_tri_uv(world, uv, np.zeros((0, 7), F))[0]) == 0


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_probe_on_crafted_hits_and_a_parallelogram_in_front(p, as_list):
    names, _, uv, rays6, _ = UW.crafted_arrays(p)
    for with_quad in (False, True):
        scene = UW.crafted_world(p, as_list, with_quad=with_quad)
        world = scene.getWorldPtr()
        oworld = as_oracle_world(world)
        on_quad = on_tri = 0
        for i, name in enumerate(names):   # one record per call: the world has one triangle, the case's record is its table
            rays = np.zeros((1, 7), F)
            rays[0, 0:6] = rays6[i]
            hit, got = p.api.probe_tri_uv(world, uv[i:i + 1], rays)
            e_hit, _, e_prim, want = UT.closest_intersection_uv(oworld, uv[i:i + 1], rays)
            assert hit[0] == e_hit[0] == 1 and bits_equal(got, want), (name, got, want)
            if with_quad and rays6[i, 0] >= 1:   # behind the parallelogram: ITS planar coordinates (x - 0.75) / 1.75, (y + 0.5) / 3, whatever the record says
                assert e_prim[0] == world.n_prims and bits_equal(got, UT.closest_intersection_uv(oworld, None, rays)[3]), name
                on_quad += 1
            on_tri += int(e_prim[0] == world.n_prims + world.n_quads - 1)
        assert on_tri >= (5 if with_quad else 15) and on_quad == (15 if with_quad else 0)


# ---- 9. identity == off == oracle -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_frame(as_list, which):
    p = pkg()
    scene = {"textured": lambda: TW.tri_room(p, textured=True, as_list=as_list), "stand_in": lambda: UW.palette_room(p, stand_in=True, as_list=as_list)}[which]()
    frame, _ = O.render(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(UW.camera(p)), W, H, SPP, DEPTH, SEED)
    frame.setflags(write=False)
    return frame


@pytest.mark.parametrize("form", EXT2, ids=EXT2_IDS)
def test_identity_table_is_no_table_is_the_oracle(p, monkeypatch, form):
    as_list = form[0] == TW.LIST
    setenv(monkeypatch, TW.FORMS[form][1])
    scene = TW.tri_room(p, textured=True, as_list=as_list)
    assert len(scene.texture_coords()) == 0
    r = renderer(p, scene, form)
    assert r.texture_coords_info() == {"enabled": False, "mapped": 0}
    none = frame_of(r)
    r.texture_coords(np.broadcast_to(UT.IDENTITY, (scene.n_triangles(), 3, 2)))
    assert r.texture_coords_info() == {"enabled": True, "mapped": 0}
    ident = frame_of(r)
    r.texture_coords(None)
    assert r.texture_coords_info() == {"enabled": False, "mapped": 0}
    off = frame_of(r)
    r.close()
    want = oracle_frame(as_list, "textured")
    assert bits_equal(none, want), mismatch_report(none, want)
    assert bits_equal(ident, none) and bits_equal(off, none)


# ---- 10. constant-UV faces == a stand-in world, against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", EXT2, ids=EXT2_IDS)
def test_constant_uv_faces_render_as_the_stand_in_world_does(p, monkeypatch, form):
    as_list = form[0] == TW.LIST
    setenv(monkeypatch, TW.FORMS[form][1])
    scene = UW.palette_room(p, as_list=as_list)
    r = renderer(p, scene, form)
    assert r.texture_coords_info() == {"enabled": True, "mapped": 20}   # the table came with the world
    assert r.light_sampling_mode() == 0
    got = frame_of(r)
    r.texture_coords(None)
    planar = frame_of(r)
    r.close()
    want = oracle_frame(as_list, "stand_in")
    assert bits_equal(got, want), mismatch_report(got, want)
    assert not bits_equal(planar, want)   # without the table every face shows the same corner of the palette


# ---- 11. general UVs, held absolutely ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def open_pair_expected(as_list):
    p = pkg()
    scene = UW.open_pair(p, as_list=as_list)
    samples, decided = UT.first_hit_frame(as_oracle_world(scene.getWorldPtr()), scene.texture_coords(), UW.pair_image(), as_oracle_camera(UW.camera(p)), W, H, SPP, SEED)
    return samples, decided


@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_general_coordinates_give_the_first_hits_texel(p, monkeypatch, as_list, form):
    setenv(monkeypatch, TW.NARROW if form == "global" else TW.LDS)
    samples, decided = open_pair_expected(as_list)
    assert decided.all(), f"the twin cannot decide {int((~decided).sum())} samples"   # a failure, never a skip
    scene = UW.open_pair(p, as_list=as_list)
    r = p.Renderer.MakeRenderer(W, H, SPP, 2, UW.camera(p), scene.getWorldPtr(), seed=SEED)
    k = r.kernel_form()
    assert k["ext"] == 2 and k["big"] == (form == "global") and r.kernel_triangles() and r.texture_coords_info() == {"enabled": True, "mapped": 2}
    got = frame_of(r)
    r.close()
    want = UT.resolve(UT.in_order_sums(samples), SPP)
    assert bits_equal(got, want), mismatch_report(got, want)
    texels = np.unique(samples.reshape(-1, 3), axis=0)
    assert len(texels) >= 12   # most of the 15 texels, the white background and maybe a failed scatter's black


# ---- 12. consistency where nothing absolute exists --------------------------------------------------------------------------------------------------------
_ROOM_SUMS = {}   # as_list -> the refinement sums of the first form rendered


@pytest.mark.parametrize("form", EXT2, ids=EXT2_IDS)
def test_every_key_and_uneven_steps_give_one_frame_of_the_uv_room(p, monkeypatch, form):
    as_list = form[0] == TW.LIST
    setenv(monkeypatch, TW.FORMS[form][1])
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # cuts inside the frame: three passes
    scene = UW.uv_room(p, as_list=as_list)
    r = renderer(p, scene, form)
    assert r.texture_coords_info() == {"enabled": True, "mapped": 48}
    img = frame_of(r)
    r.refine(3)
    r.refine(5)   # uneven steps
    sums = r.refine_sums()
    assert bits_equal(r.DownloadRenderbuffer(), img)
    first = _ROOM_SUMS.setdefault(as_list, sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)
    r.texture_coords(None)
    r.refine(SPP)
    assert not bits_equal(r.refine_sums(), sums)   # the sphere is in view: its coordinates show
    r.close()
    if len(_ROOM_SUMS) == 2:   # no tie between two primitives in this room: a list and a tree see the same hits
        assert bits_equal(_ROOM_SUMS[False], _ROOM_SUMS[True])


@pytest.mark.parametrize("ranks", [2, 3])
def test_ranks_through_the_memcpy_transport(p, monkeypatch, ranks):
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    scene = UW.uv_room(p)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, UW.camera(p), scene.getWorldPtr(), seed=SEED)
    one = frame_of(r)
    r.texture_coords(None)
    planar = frame_of(r)
    r.close()
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, UW.camera(p), scene.getWorldPtr(), ranks, seed=SEED)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), one)
    m.texture_coords(None)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), planar) and not bits_equal(planar, one)
    with pytest.raises(p.capi.RtError, match="rt_renderer_texture_coords"):
        m.texture_coords(np.zeros((3, 6), F))   # refused before any rank changes
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), planar)
    m.close()


@pytest.mark.parametrize("mode", [1, 2, 4, 16])
def test_light_sampling_modes_read_the_table_in_both_forms(p, monkeypatch, mode):
    frames = []
    for env in (TW.LDS, TW.NARROW):
        setenv(monkeypatch, env)
        scene = UW.uv_room(p, lamp=True, tri_light=True)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, UW.camera(p), scene.getWorldPtr(), seed=SEED)
        r.light_sampling(mode)
        assert r.light_sampling_mode() == mode and r.kernel_form()["big"] == (env is TW.NARROW) and r.kernel_form()["nee"] == 1
        assert r.texture_coords_info()["enabled"]
        r.refine(SPP)
        with_table = r.refine_sums()
        r.texture_coords(None)
        r.refine(SPP)
        without = r.refine_sums()
        r.texture_coords(scene.texture_coords())   # on again while the mode is on: the mode's image gets its tail back
        r.refine(SPP)
        assert bits_equal(r.refine_sums(), with_table) and not bits_equal(without, with_table)
        r.close()
        frames.append(with_table)
    assert bits_equal(frames[0], frames[1]), mismatch_report(frames[0], frames[1])


# ---- 13. with normals --------------------------------------------------------------------------------------------------------------------------------------
def test_both_tables_and_each_alone(p):
    scene = UW.uv_room(p, normals=True, lamp=True)
    vn, uv = scene.vertex_normals(), scene.texture_coords()
    assert len(vn) == len(uv) == scene.n_triangles()
    cam = UW.camera(p)

    def fresh(keep):
        return p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, bare_world(scene, keep), seed=SEED)
    only_uv, only_vn, neither = fresh(("texture_coords",)), fresh(("vertex_normals",)), fresh(())
    assert only_uv.texture_coords_info()["enabled"] and not only_uv.shading_normals_info()["enabled"]
    assert only_vn.shading_normals_info()["enabled"] and not only_vn.texture_coords_info()["enabled"]
    f_uv, f_vn, f_none = frame_of(only_uv), frame_of(only_vn), frame_of(neither)
    both = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
    assert both.shading_normals_info()["enabled"] and both.texture_coords_info() == {"enabled": True, "mapped": 48}
    f_both = frame_of(both)
    assert len({f.tobytes() for f in (f_uv, f_vn, f_none, f_both)}) == 4
    both.shading_normals(None)                       # normals off: the UV frame as it is without normals
    assert both.texture_coords_info()["enabled"] and bits_equal(frame_of(both), f_uv)
    both.shading_normals(vn)
    assert bits_equal(frame_of(both), f_both)
    both.texture_coords(None)                        # UVs off: the frame of the normals alone
    assert both.shading_normals_info()["enabled"] and bits_equal(frame_of(both), f_vn)
    both.shading_normals(None)
    assert bits_equal(frame_of(both), f_none)
    both.texture_coords(uv)                          # the other order of switching on
    both.shading_normals(vn)
    assert bits_equal(frame_of(both), f_both)
    # a light-sampling mode enabled AFTER both tables reads both; so does one enabled before them
    both.light_sampling(2)
    nee_both = frame_of(both)
    late = fresh(())
    late.light_sampling(2)
    nee_none = frame_of(late)
    late.shading_normals(vn)
    late.texture_coords(uv)
    assert bits_equal(frame_of(late), nee_both) and not bits_equal(nee_none, nee_both)
    late.shading_normals(None)
    only_uv.light_sampling(2)
    assert bits_equal(frame_of(late), frame_of(only_uv))
    for r in (only_uv, only_vn, neither, both, late):
        r.close()


def test_constant_uv_faces_with_normals_are_the_smooth_twin_of_an_ext1_stand_in(p):
    """item 10's argument with the vertex normals on: the image world (EXT 2, both tables) against _smooth_twin's frame of the stand-in (EXT 1, normals only),
    which the twin follows in full; then UVs off leaves section 21's frame of the same world: the oracle does not know normals, the planar lookup is its own"""
    scene = UW.palette_room(p, normals=True, textured=False)
    stand = UW.palette_room(p, stand_in=True, normals=True, textured=False)
    cam = UW.camera(p)
    samples, followed = ST.frame_samples(as_oracle_world(stand.getWorldPtr()), stand.vertex_normals(), as_oracle_camera(cam), W, H, SPP, DEPTH, SEED)
    assert followed.all()
    want = ST.resolve(ST.in_order_sums(samples), SPP)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
    assert r.kernel_form()["ext"] == 2 and r.shading_normals_info()["smooth"] == 20 and r.texture_coords_info()["mapped"] == 20
    got = frame_of(r)
    r.close()
    assert bits_equal(got, want), mismatch_report(got, want)
    s = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, stand.getWorldPtr(), seed=SEED)
    assert s.kernel_form()["ext"] == 1
    assert bits_equal(frame_of(s), want)
    s.close()


# ---- 14. no image material -----------------------------------------------------------------------------------------------------------------------------------
def test_a_table_on_a_world_that_never_reads_it_changes_no_bit(p):
    forms = []
    for build in (lambda: UW.uv_room(p, image=False), lambda: TW.tri_room(p)):   # an EXT 2 world whose image is on a parallelogram; an EXT 1 world
        scene = build()
        n = scene.n_triangles()
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, UW.camera(p), bare_world(scene), seed=SEED)
        form = r.kernel_form()
        forms.append(form["ext"])
        before = frame_of(r)
        r.texture_coords(UW.random_uvs(3 * n, seed=3).reshape(n, 6))
        assert r.texture_coords_info() == {"enabled": True, "mapped": n} and r.kernel_form() == form   # the kernel it launched
        assert bits_equal(frame_of(r), before)
        r.close()
    assert forms == [2, 1]
    want, _ = O.render(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(UW.camera(p)), W, H, SPP, DEPTH, SEED)
    assert bits_equal(before, want)


# ---- 15. refusals and restarts -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point_and_leave_the_renderer_as_it_was(p):
    scene = UW.uv_room(p)
    uv = UT.table(scene.texture_coords()).reshape(-1, 6)
    cam = UW.camera(p)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, bare_world(scene), seed=SEED)
    planar = frame_of(r)
    nan = uv.copy()
    nan[7, 2] = np.nan
    for bad in (uv[:-1], np.concatenate([uv, uv[:1]]), nan):   # a wrong n twice, a NaN
        with pytest.raises(p.capi.RtError, match="rt_renderer_texture_coords") as e:
            r.texture_coords(bad)
        assert e.value.code == 1   # RT_ERR_INVALID
    assert not r.texture_coords_info()["enabled"] and bits_equal(frame_of(r), planar)
    r.close()
    spheres = p.Scene.book1_final(SEED)   # variants 5 and 6 render no world with triangles: they refuse a table on the variant alone, before its size is looked at
    for variant, word, world, table in ((1, "variant 1", bare_world(scene), uv), (5, "variant 5", spheres.getWorldPtr(), uv[:1]), (6, "variant 6", spheres.getWorldPtr(), uv[:1])):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, world, seed=SEED, variant=variant)
        with pytest.raises(p.capi.RtError, match="rt_renderer_texture_coords.*" + word) as e:
            r.texture_coords(table)
        assert e.value.code == 1 and not r.texture_coords_info()["enabled"]
        r.close()
    for traversal in (1, 2):   # queue, wide4
        s = UW.uv_room(p, traversal=traversal)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, bare_world(s), seed=SEED)
        with pytest.raises(p.capi.RtError, match="rt_renderer_texture_coords.*traversal") as e:
            r.texture_coords(s.texture_coords())
        assert e.value.code == 1
        r.close()
        with pytest.raises(p.capi.RtError, match="rt_renderer_texture_coords"):   # Renderer pushes the scene's table at creation: the refusal surfaces there
            p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED)


def test_the_same_table_keeps_the_refinement_and_a_changed_one_restarts_it(p):
    scene = UW.uv_room(p)
    uv = UT.table(scene.texture_coords()).reshape(-1, 6)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, UW.camera(p), scene.getWorldPtr(), seed=SEED)
    r.refine(SPP)
    whole = r.refine_sums()
    r.texture_coords(uv.copy())   # the same table again, right after creation pushed it
    assert r.refine_info()["samples"] == SPP
    r.texture_coords(None)
    assert r.refine_info()["samples"] == 0
    r.texture_coords(None)   # off twice: nothing
    r.texture_coords(uv)
    r.refine(2)
    r.texture_coords(uv)
    assert r.refine_info()["samples"] == 2
    r.refine(SPP - 2)
    assert bits_equal(r.refine_sums(), whole)
    other = uv.copy()
    other[len(other) - 1, 0] += F(0.25)
    r.texture_coords(other)
    assert r.refine_info()["samples"] == 0 and r.texture_coords_info() == {"enabled": True, "mapped": 48}
    r.close()


# ---- 16. the C++ mirror ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_app_renders_the_frame_python_renders(p):
    def fnv1a(data):
        h = 1469598103934665603
        for b in data:
            h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
        return h
    w, h, spp, depth = 40, 24, 4, 5
    out = subprocess.check_output([os.path.join(ROOT, "tests", "cpp_uv", "uv_app"), str(w), str(h), str(spp), str(depth)], text=True, timeout=120)
    from ray_tracing_v06_amd import image_io
    s = p.Scene()
    s.set_image(image_io.read_ppm(os.path.join(ROOT, "tests", "golden", "uv_atlas_8x4.ppm")))   # the image the program computes
    white, image = s.Lambertian((0.73, 0.73, 0.73)), s.ImageTexture()
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), white)
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    t = np.array([[0, 0.5], [1, 0.5], [0.5, 1.25], [0.5, -0.25], [0.25, 0.5], [0.75, 0.5]], F)
    f = np.array([0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5], np.uint32).reshape(-1, 3)
    s.MakeMesh(v, f, image, 1.5, 20.0, (0, 1.8, 0), normals=v, uvs=t)
    s.MakeTriangle((-3, 0.1, -2), (-1.5, 0.1, -2.5), (-2.5, 2, -2), image, uvs=[(0.1, 0.1), (0.9, 0.2), (0.4, 0.95)])
    s.set_background((0.6, 0.7, 0.9))
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(w, h, spp, depth, p.PinholeCamera((0.5, 2.5, 7), (0, 1.5, 0), (0, 1, 0), 50.0, w / h), s.getWorldPtr(), seed=1984)
    assert r.texture_coords_info() == {"enabled": True, "mapped": 9} and r.shading_normals_info() == {"enabled": True, "smooth": 8}
    frame = frame_of(r)
    r.close()
    assert out.strip() == f"uv {w}x{h} spp={spp} depth={depth} fnv={fnv1a(frame.tobytes()):016x}"


def test_render_tool_textures_an_obj_mesh_and_refuses_one_without_coordinates(p, tmp_path):
    import sys
    golden = os.path.join(ROOT, "tests", "golden")
    out = tmp_path / "cube.png"
    args = ["--scene", "cornell_box", "--width", "32", "--height", "32", "--spp", "4", "--depth", "8", "--mesh-scale", "160", "--mesh-rotate-y", "25",
            "--mesh-translate", "200,0,150", "--texture", os.path.join(golden, "uv_atlas_8x4.png")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py")] + args + ["--mesh", os.path.join(golden, "uv_cube.obj"), "--out", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    from ray_tracing_v06_amd import image_io, mesh_io
    s = p.Scene.cornell_box()
    s.set_image(image_io.read_png(os.path.join(golden, "uv_atlas_8x4.png")))
    v, f, t, tf = mesh_io.load_obj_uvs(os.path.join(golden, "uv_cube.obj"))
    s.MakeMesh(v, f, s.ImageTexture(), 160.0, 25.0, (200, 0, 150), uvs=t, uv_faces=tf)
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(32, 32, 4, 8, p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0), s.getWorldPtr(), seed=1984)
    assert r.texture_coords_info() == {"enabled": True, "mapped": 12}
    expected = tmp_path / "api.png"
    image_io.write_png(str(expected), frame_of(r))
    r.close()
    assert out.read_bytes() == expected.read_bytes()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py")] + args + ["--mesh", os.path.join(golden, "uv_cube_incomplete.obj"), "--out", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "no complete set of texture coordinates" in res.stderr
