"""Normal maps on the GPU: the device probe against the host batch, all sixteen kernel forms — eight plain, eight under mode 48 — against the
whole-sample twin, flat maps and strength 0 against the renderer without a table, sessions, the feature pass, ranks and refusals.  Every comparison is bit for bit:
with the numpy twin (tests/_nmap_twin.py, pinned by tests/test_normal_maps_cpu.py), which follows EVERY sample of the test room, or with the renderer's own frame
on the kernels it had before.  Frames are 24 x 16 at 8 spp and depth 6."""
import numpy as np
import pytest

import _aov_tex_twin as AT
import _nmap_twin as NT
import _nmap_worlds as NW
import _tri_worlds as TW
from _common import as_oracle_camera, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = NW.W, NW.H, NW.SPP, NW.DEPTH, NW.SEED
FORMS = list(NW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, NW.ENV_TREE]
LDS_FAST = (TW.BVH, 0, 2, 0, 0)


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def setenv(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def renderer(p, scene, form=LDS_FAST, mode=0, spp=SPP, mapped=True):
    """a renderer of `scene` on the recipe of `form` (the caller has set its environment) that states the kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, NW.camera(p), scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_normal_map() == mapped and r.normal_maps_info() == {"enabled": mapped, "mapped": 4 if mapped else 0}
    if mapped:
        assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
        assert r.kernel_triangles() and r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, NT.VT.resolve(sums, spp))
    return sums


# ---- 1. the rule on the device ----------------------------------------------------------------------------------------------------------------------------
def test_the_probe_is_the_host_batch_bit_for_bit(p):
    tab, cases = NW.table(), NW.random_cases()
    aimed_tab, aimed, expected = NW.aimed_cases()
    for t, c in ((NW.api_table(tab), cases), (NW.api_table(aimed_tab), aimed)):
        host_n, host_path = NW.run_cases(p.api.normal_map_batch, t, c)
        dev_n, dev_path = NW.run_cases(p.api.probe_normal_map, t, c)
        assert (dev_path == host_path).all(), np.nonzero(dev_path != host_path)[0][:5]
        assert bits_equal(dev_n, host_n), mismatch_report(dev_n, host_n)
    assert dev_path.tolist() == expected.tolist()   # the aimed cases leave the rule on the device by every way out, as on the host


# ---- 2. the sixteen forms -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_sums():
    return {}


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_is_the_twin(p, monkeypatch, first_sums, form, mode):
    """All 16 NMAP keys, each reached by its recipe on the test room — a checker floor, a mapped Lambertian sphere, a mapped fuzzy-metal sphere, a mapped
    parallelogram wall, an image-textured uv_sphere mesh with vertex normals, coordinates and a map, a quad light — under a constant background (plain) or the sky
    map (mode 48): the sums equal the whole-sample twin's on every pixel, and differ from the same room's without the table."""
    run = NW.run(bool(mode), as_list=form[0] == TW.LIST)
    assert run.followed.all()                                              # the twin leaves no sample out
    assert run.info["replaced"] > 300 and run.info["facing"] > 10          # ... and bent normals on the way, and met the facing test
    assert not bits_equal(run.samples, run.unmapped)
    setenv(monkeypatch, TW.FORMS[form][1])
    r = renderer(p, run.scene, form, mode)
    sums = sums_of(r)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(sums.sum(axis=(0, 1)), run.sums.sum(axis=(0, 1)))   # the frame sums
    first = first_sums.setdefault(mode, sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)
    r.normal_maps(None)   # the same renderer without the table: another frame, on the kernel it had
    assert not r.kernel_normal_map()
    without = sums_of(r)
    r.close()
    assert not bits_equal(without, sums)
    assert bits_equal(without, NT.VT.in_order_sums(run.unmapped)), mismatch_report(without, NT.VT.in_order_sums(run.unmapped))


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_flat_maps_and_strength_zero_are_the_renderer_without_a_table(p, monkeypatch, form, mode):
    """on each of the sixteen keys: flat maps at the room's strengths, and the room's maps at strength 0, give the bits the existing kernels give with the table off"""
    setenv(monkeypatch, TW.FORMS[form][1])
    as_list = form[0] == TW.LIST
    frames = []
    for kw in (dict(flat=True), dict(strength=0.0)):
        scene = NW.room(p, env=bool(mode), as_list=as_list, **kw)
        r = renderer(p, scene, form, mode)
        frames.append(sums_of(r))
        r.normal_maps(None)
        assert not r.kernel_normal_map() and r.kernel_form()["ext"] == 2
        frames.append(sums_of(r))
        r.close()
    assert bits_equal(frames[0], frames[1]), mismatch_report(frames[0], frames[1])
    assert bits_equal(frames[2], frames[3]), mismatch_report(frames[2], frames[3])


def test_a_world_of_spheres_alone_takes_a_map(p, monkeypatch):
    """no quad, no triangle, no image material: the world's own kernels are the reference's feature set's; with a flat map the NMAP form gives their bits, with a
    map another frame"""
    setenv(monkeypatch, TW.LDS)
    frames = {}
    for name, img in (("flat", NW.XW.constant(4, 4, (128, 128, 255))), ("bumps", NW.bumps())):
        s = p.Scene()
        ground, ball, metal = s.Lambertian((0.5, 0.5, 0.5)), s.Lambertian((0.7, 0.3, 0.3)), s.Metal((0.8, 0.8, 0.8), 0.2)
        s.MakeSphere((5, -100, 6), 100.0, ground)
        s.MakeSphere((3.5, 1.0, 6), 1.0, ball)
        s.MakeSphere((6.5, 1.0, 6), 1.0, metal)
        s.set_image(img)
        s.image_sampling(0, "repeat", "bilinear")
        for m in (ground, ball, metal):
            s.set_normal_map(m, 0, 1.0)
        s.BuildBVH_SAH()
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, NW.camera(p), s.getWorldPtr(), seed=SEED)
        assert r.kernel_normal_map() and r.normal_maps_info() == {"enabled": True, "mapped": 3}
        frames[name] = sums_of(r)
        r.normal_maps(None)
        frames[name + " off"] = sums_of(r)
        r.close()
    assert bits_equal(frames["flat"], frames["flat off"]) and bits_equal(frames["flat off"], frames["bumps off"])
    assert not bits_equal(frames["bumps"], frames["bumps off"])


# ---- 3. sessions ------------------------------------------------------------------------------------------------------------------------------------------------
def test_uneven_steps_and_the_table_on_off_on(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = NW.run(False)
    r = renderer(p, run.scene)
    for n in (1, 4, 3):
        r.refine(n)
    stepped = r.refine_sums()
    assert bits_equal(stepped, run.sums), mismatch_report(stepped, run.sums)
    table = run.scene.normal_maps()
    r.normal_maps(table)   # unchanged: a no-op that keeps the refinement
    assert r.refine_info()["samples"] == SPP
    r.normal_maps(None)
    assert r.refine_info()["samples"] == 0 and not r.kernel_normal_map()
    off = sums_of(r)
    r.normal_maps(table)
    assert r.refine_info()["samples"] == 0 and r.kernel_normal_map()
    on = sums_of(r)
    r.close()
    assert bits_equal(on, run.sums) and not bits_equal(off, on)


# ---- 4. the feature pass ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [True, False], ids=["vertex-normals", "flat"])
@pytest.mark.parametrize("as_list", [False, True], ids=["stack", "list"])
def test_the_feature_pass_carries_the_mapped_normal(p, monkeypatch, as_list, smooth):
    setenv(monkeypatch, TW.LDS)
    scene = NW.room(p, as_list=as_list, smooth=smooth)
    world = NW.as_oracle_world(scene.getWorldPtr())
    vn, uv, nmaps, table = scene.vertex_normals(), scene.texture_coords(), scene.normal_maps(), NW.room_table()
    assert bool(len(vn)) == smooth
    info = {}
    want = {}
    for name, maps in (("mapped", nmaps), ("unmapped", None)):
        trace, _ = NT.walk_of(vn if smooth else None, uv, maps, table, info)
        want[name] = AT.sums(world, as_oracle_camera(NW.camera(p)), W, H, SPP, SEED, True, uv=uv, table=table, trace=trace)[0]
    assert info["replaced"] > 100 and not bits_equal(want["mapped"][..., 0:3], want["unmapped"][..., 0:3])
    assert bits_equal(want["mapped"][..., 3:8], want["unmapped"][..., 3:8])   # albedo, depth and hits are unchanged
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, NW.camera(p), scene.getWorldPtr(), seed=SEED)
    with pytest.raises(p.capi.RtError, match="RT_AOV_TEXTURED") as e:
        r.enable_aov()
    assert e.value.code == 1
    r.enable_aov(textured=True)
    r.refine(SPP)
    got = r.aov_sums()
    assert bits_equal(got, want["mapped"]), mismatch_report(got, want["mapped"])
    r.normal_maps(None)
    r.refine(SPP)
    got = r.aov_sums()
    r.close()
    assert bits_equal(got, want["unmapped"]), mismatch_report(got, want["unmapped"])


# ---- 5. ranks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    run = NW.run(False)
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, NW.camera(p), run.scene.getWorldPtr(), 2, seed=SEED)
    assert m.normal_maps_info() == {"enabled": True, "mapped": 4}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.close()
    assert bits_equal(frame, run.frame), mismatch_report(frame, run.frame)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_renderer_usable(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = NW.run(False)
    table = run.scene.normal_maps()
    world = run.scene.getWorldPtr()
    del world.normal_maps   # a renderer without the table, to give it to
    cam = NW.camera(p)

    def refused(make, why, give=lambda r: r.normal_maps(table)):
        r = make()
        with pytest.raises(p.capi.RtError, match=why) as e:
            give(r)
        assert e.value.code == 1 and not r.kernel_normal_map()
        r.Render()   # ... and is as usable as it was
        r.close()

    for mode in (1, 2, 4, 16):
        def lit(mode=mode):
            r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, world, seed=SEED)
            r.light_sampling(mode)
            return r
        refused(lit, f"light-sampling mode {mode} is on")
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, run.scene.getWorldPtr(), seed=SEED)   # ... and the other way round
    for mode in (1, 2, 4, 16, 32):
        with pytest.raises(p.capi.RtError, match=f"light-sampling mode {mode} has no kernel that reads one") as e:
            r.light_sampling(mode)
        assert e.value.code == 1 and r.light_sampling_mode() == 0 and r.kernel_normal_map()
    on_a_light = table.copy()
    on_a_light[int(np.nonzero(run.scene.arrays()[2]["type"] == 4)[0][0])] = (1, 1, 1.0, 0)
    negative = table.copy()
    negative["strength"][np.nonzero(negative["on"])[0][0]] = -1.0
    for bad, why in ((table[:-1], "records for a world of"), (on_a_light, "takes no normal map"), (negative, "strength")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.normal_maps(bad)
        assert e.value.code == 1 and r.kernel_normal_map()   # the table it had stays
    r.textures(None)   # the entries the maps name are gone: refused before any kernel, as an image material without an entry is
    with pytest.raises(p.capi.RtError, match="normal map of the world names image|image material of the world names image") as e:
        r.Render()
    assert e.value.code == 1
    r.textures(run.scene.textures())
    sums = sums_of(r)
    r.close()
    assert bits_equal(sums, run.sums)
    def walked(traversal=None, tree=False):   # a floor and two balls, walked another way; the table comes by hand
        s = p.Scene()
        grey = s.Lambertian((0.5, 0.5, 0.5))
        one, two = s.MakeSphere((3.5, 1.0, 6), 1.0, grey), s.MakeSphere((6.5, 1.0, 6), 1.0, s.Metal((0.8, 0.8, 0.8), 0.2))
        if tree:
            s.set_world_node_tree(s.bvh_node(p.Scene.prim_ref(one), p.Scene.prim_ref(two)))
        else:
            s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), grey)
            s.set_traversal(traversal)
            s.BuildBVH_SAH()
        return p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED)
    by_hand = np.zeros(2, p.capi.NORMAL_MAP_DT)
    by_hand[0] = (1, 0, 1.0, 0)
    for make, why in ((lambda: walked(1), "queue or wide4"), (lambda: walked(2), "queue or wide4"), (lambda: walked(tree=True), "bvh_node tree")):
        refused(make, why, give=lambda r: r.normal_maps(by_hand))


def test_the_baseline_kernel_the_ray_exchange_and_the_tolerance_mode_refuse_a_table(p, monkeypatch):
    """kernel variants 5 and 6 take worlds of the reference's feature set only: spheres under the sky gradient, here with a table given by hand; variant 1 too"""
    setenv(monkeypatch, TW.LDS)
    s = p.Scene.book1_final(SEED)   # a BVH of spheres in the LDS
    table = np.zeros(s.getWorldPtr().n_materials, p.capi.NORMAL_MAP_DT)
    table[0] = (1, 0, 1.0, 0)       # the ground, a Lambertian
    assert s.arrays()[2]["type"][0] == 0
    cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
    for variant in (1, 5, 6):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED, variant=variant)
        why = "the baseline kernel \\(variant 1\\) reads no normal-map table" if variant == 1 else f"kernel variant {variant} reads no texture table and no normal-map table"
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.normal_maps(table)
        assert e.value.code == 1 and not r.kernel_normal_map()
        r.Render()
        r.close()
