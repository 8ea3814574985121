"""Microfacet surfaces on the GPU: the device probe against the host batch, all sixteen kernel forms — eight plain, eight under mode 48 — against the
whole-sample twin, a table of records that are all off against the kernels the renderer had, sessions, mode 48 around the table, ranks, the feature pass and the
refusals.  Every comparison is bit for bit: with the numpy twin (tests/_mfac_twin.py, pinned by tests/test_microfacets_cpu.py), which follows EVERY sample of
the test room, or with the renderer's own frame.  Frames are 24 x 16 at 8 spp and depth 6."""
import numpy as np
import pytest

import _mfac_twin as MT
import _mfac_worlds as MW
import _nmap_worlds as NW
import _tri_worlds as TW
from _common import bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = MW.W, MW.H, MW.SPP, MW.DEPTH, MW.SEED
FORMS = list(MW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, MW.ENV_TREE]
LDS_FAST = (TW.BVH, 0, 2, 0, 0)
RECORDS = 5   # the floor, the two conductors, the shell, the mesh


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


def renderer(p, scene, form=LDS_FAST, mode=0, spp=SPP, recorded=True):
    """a renderer of `scene` on the recipe of `form` (the caller has set its environment) that states the kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, MW.camera(p), scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_microfacet() == recorded and r.microfacets_info() == {"enabled": recorded, "records": RECORDS if recorded else 0}
    if recorded:
        assert not r.kernel_normal_map()   # one family answers: the MFAC forms read the normal-map table too
        assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
        assert r.kernel_triangles() and r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, MT.resolve(sums, spp))
    return sums


# ---- 1. the rule on the device ----------------------------------------------------------------------------------------------------------------------------
def test_the_probe_is_the_host_batch_bit_for_bit(p):
    aimed, expected = MW.aimed_cases()
    for cases in (MW.random_cases(), aimed):
        host = MW.run_cases(p.api.microfacet_batch, cases)
        dev = MW.run_cases(p.api.probe_microfacet, cases)
        for d, h, name in zip(dev, host, ("direction", "weight", "way", "draws")):
            if d.dtype == np.uint32:
                assert (d == h).all(), (name, np.nonzero(d != h)[0][:5])
            else:
                assert bits_equal(d, h), (name, mismatch_report(d, h))
    assert set(dev[2].tolist()) == set(MT.WAYS)   # the aimed cases leave the rule on the device by every way out, as on the host
    assert all(e == 0 or e == w for e, w in zip(expected, dev[2]))


# ---- 2. the sixteen forms -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_sums():
    return {}


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_is_the_twin(p, monkeypatch, first_sums, form, mode):
    """All 16 MFAC keys, each reached by its recipe on the test room — a coated checker floor, a rough-conductor sphere and triangle, a coated image-textured mesh
    under a roughness map and a normal map, a metal without a record, a glass ball, a quad light, all inside a coated shell — under a constant background
    (plain) or the sky map (mode 48): the sums equal the whole-sample twin's on every pixel; with the records all off, and with the table taken away, they equal
    the twin's without records."""
    run = MW.run(bool(mode), as_list=form[0] == TW.LIST)
    st = run.stats
    assert run.followed.all()                                              # the twin leaves no sample out
    assert st["specular"] > 0 and st["base"] > 0 and st["absorbed"] > 0 and st["backside"] > 0 and st["mapped"] > 0 and st["glass"] > 0, st   # ... and took every way out
    assert not bits_equal(run.samples, run.unrecorded)
    setenv(monkeypatch, TW.FORMS[form][1])
    r = renderer(p, run.scene, form, mode)
    sums = sums_of(r)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(sums.sum(axis=(0, 1)), run.sums.sum(axis=(0, 1)))   # the frame sums
    first = first_sums.setdefault(mode, sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)
    unrecorded = MT.in_order_sums(run.unrecorded)
    off = np.zeros(len(run.scene.microfacets()), p.capi.MICROFACET_DT)
    r.microfacets(off)     # the same kernel, no record on: the frame of the room without records
    assert r.kernel_microfacet() and r.microfacets_info() == {"enabled": True, "records": 0}
    all_off = sums_of(r)
    assert bits_equal(all_off, unrecorded), mismatch_report(all_off, unrecorded)
    r.microfacets(None)    # ... and without the table, on the normal-map kernel the renderer had: the same frame again
    assert not r.kernel_microfacet() and r.kernel_normal_map()
    without = sums_of(r)
    r.close()
    assert bits_equal(without, unrecorded), mismatch_report(without, unrecorded)
    assert not bits_equal(without, sums)


def test_a_world_without_textures_takes_constant_records(p, monkeypatch):
    """no image, no texture table, no normal map: a microfacet table of constant records works alone; all off, it gives the world's own kernel's bits"""
    setenv(monkeypatch, TW.LDS)
    s = simple(p)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, MW.camera(p), s.getWorldPtr(), seed=SEED)
    assert r.kernel_microfacet() and r.microfacets_info() == {"enabled": True, "records": 3} and not r.textures_info()["enabled"]
    on = sums_of(r)
    r.microfacets(np.zeros(3, p.capi.MICROFACET_DT))
    all_off = sums_of(r)
    r.microfacets(None)
    assert not r.kernel_microfacet() and r.kernel_form()["ext"] == 1
    off = sums_of(r)
    r.close()
    assert bits_equal(all_off, off), mismatch_report(all_off, off)
    assert not bits_equal(on, off)


def simple(p, records=True):
    """a floor and two balls on the world's own EXT 1 kernel: coats on the Lambertians, a conductor on the metal"""
    s = p.Scene()
    floor, ball, metal = s.Lambertian((0.5, 0.5, 0.5)), s.Lambertian((0.7, 0.3, 0.3)), s.Metal((0.9, 0.7, 0.4), 0.2)
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), floor)
    s.MakeSphere((3.5, 1.0, 6), 1.0, ball)
    s.MakeSphere((6.5, 1.0, 6), 1.0, metal)
    if records:
        s.set_microfacet(floor, 0.2, 0.3).set_microfacet(ball, 0.6).set_microfacet(metal, 0.35)
    s.set_background(MW.BACKGROUND)
    s.BuildBVH_SAH()
    return s


# ---- 3. the normal-map family is what it was ----------------------------------------------------------------------------------------------------------------------
def test_a_normal_map_table_alone_still_runs_its_own_family(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = NW.run(False)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, NW.camera(p), run.scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[LDS_FAST][0])
    assert r.kernel_normal_map() and not r.kernel_microfacet() and r.microfacets_info() == {"enabled": False, "records": 0}
    sums = sums_of(r)
    r.close()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)


# ---- 4. sessions ------------------------------------------------------------------------------------------------------------------------------------------------
def test_uneven_steps_and_the_table_on_off_on(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = MW.run(False)
    r = renderer(p, run.scene)
    for n in (1, 4, 3):
        r.refine(n)
    stepped = r.refine_sums()
    assert bits_equal(stepped, run.sums), mismatch_report(stepped, run.sums)
    table = run.scene.microfacets()
    r.microfacets(table)   # unchanged: a no-op that keeps the refinement
    assert r.refine_info()["samples"] == SPP
    r.microfacets(None)
    assert r.refine_info()["samples"] == 0 and not r.kernel_microfacet()
    off = sums_of(r)
    r.microfacets(table)
    assert r.refine_info()["samples"] == 0 and r.kernel_microfacet()
    on = sums_of(r)
    r.close()
    assert bits_equal(on, run.sums) and not bits_equal(off, on)


def test_mode_48_on_and_off_around_the_table(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = MW.run(True)
    table = run.scene.microfacets()
    world = run.scene.getWorldPtr()
    del world.microfacets   # a renderer without the table, to give it to
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, MW.camera(p), world, seed=SEED, variant=TW.FORMS[LDS_FAST][0])
    r.light_sampling(48)
    assert not r.kernel_microfacet() and r.kernel_normal_map()
    r.microfacets(table)   # the mode first, then the table
    assert r.kernel_microfacet() and r.kernel_env_light() and r.kernel_light_tree()
    sampled = sums_of(r)
    assert bits_equal(sampled, run.sums), mismatch_report(sampled, run.sums)
    r.light_sampling(0)    # the mode off under the table: the plain MFAC form
    assert r.kernel_microfacet() and not r.kernel_env_light()
    plain = sums_of(r)
    r.light_sampling(48)   # ... and on again
    again = sums_of(r)
    r.close()
    assert bits_equal(again, run.sums) and not bits_equal(plain, sampled)
    fresh = renderer(p, run.scene)   # the table from creation, no mode: the same plain frame
    want = sums_of(fresh)
    fresh.close()
    assert bits_equal(plain, want), mismatch_report(plain, want)


# ---- 5. ranks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    run = MW.run(False)
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, MW.camera(p), run.scene.getWorldPtr(), 2, seed=SEED)
    assert m.microfacets_info() == {"enabled": True, "records": RECORDS}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.close()
    assert bits_equal(frame, run.frame), mismatch_report(frame, run.frame)


# ---- 6. the feature pass ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_feature_pass_does_not_read_the_table(p, monkeypatch):
    """textured mode on the room, plain mode on a world it accepts: the feature sums with the table on are the sums with it off; the plain pass refuses the room
    for its normal maps with and without the table, as it did"""
    setenv(monkeypatch, TW.LDS)
    for scene, textured in ((MW.run(False).scene, True), (simple(p), False)):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, MW.camera(p), scene.getWorldPtr(), seed=SEED)
        assert r.kernel_microfacet()
        if textured:
            with pytest.raises(p.capi.RtError, match="RT_AOV_TEXTURED") as e:
                r.enable_aov()
            assert e.value.code == 1
        r.enable_aov(textured=textured)
        r.refine(SPP)
        on = r.aov_sums()
        r.microfacets(None)
        if textured:
            with pytest.raises(p.capi.RtError, match="RT_AOV_TEXTURED"):
                r.enable_aov()
        r.refine(SPP)
        off = r.aov_sums()
        r.close()
        assert bits_equal(on, off), mismatch_report(on, off)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_renderer_usable(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = MW.run(False)
    table = run.scene.microfacets()
    world = run.scene.getWorldPtr()
    del world.microfacets   # a renderer without the table, to give it to
    cam = MW.camera(p)

    def refused(make, why, give=lambda r: r.microfacets(table)):
        r = make()
        with pytest.raises(p.capi.RtError, match=why) as e:
            give(r)
        assert e.value.code == 1 and not r.kernel_microfacet()
        r.Render()   # ... and is as usable as it was
        r.close()

    for mode in (1, 2, 4, 16):
        def lit(mode=mode):
            r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, world, seed=SEED)
            r.normal_maps(None)   # (the room's normal map refuses these modes too)
            r.light_sampling(mode)
            return r
        refused(lit, f"light-sampling mode {mode} is on")
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, run.scene.getWorldPtr(), seed=SEED)   # ... and the other way round
    r.normal_maps(None)
    for mode in (1, 2, 4, 16, 32):
        with pytest.raises(p.capi.RtError, match=f"microfacet table, and light-sampling mode {mode} has no kernel that reads one") as e:
            r.light_sampling(mode)
        assert e.value.code == 1 and r.light_sampling_mode() == 0 and r.kernel_microfacet()
    r.normal_maps(run.scene.normal_maps())
    mats = run.scene.arrays()[2]["type"]
    on_a_light, on_glass = table.copy(), table.copy()
    on_a_light[int(np.nonzero(mats == 4)[0][0])] = (1, 0, 0.5, 0.04)
    on_glass[int(np.nonzero(mats == 2)[0][0])] = (1, 0, 0.5, 0.04)
    first = int(np.nonzero(table["on"])[0][0])
    rough, nan, spec, kind, image = (table.copy() for _ in range(5))
    rough["roughness"][first], nan["roughness"][first], spec["specular"][first], kind["on"][first] = 1.5, np.nan, -0.25, 3
    image["on"][first], image["image"][first] = 2, 256
    for bad, why in ((table[:-1], "records for a world of"), (on_a_light, "takes no microfacet record"), (on_glass, "takes no microfacet record"), (rough, "roughness"),
                     (nan, "roughness"), (spec, "specular"), (kind, "on is 0"), (image, "image index")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.microfacets(bad)
        assert e.value.code == 1 and r.kernel_microfacet() and r.microfacets_info()["records"] == RECORDS   # the table it had stays
    r.textures(None)   # the entry the roughness map names is gone: refused before any kernel, as a normal map without an entry is
    with pytest.raises(p.capi.RtError, match="roughness map of the world names image|normal map of the world names image|image material of the world names image") as e:
        r.Render()
    assert e.value.code == 1
    r.normal_maps(None)
    with pytest.raises(p.capi.RtError, match="roughness map of the world names image|image material of the world names image") as e:
        r.Render()
    assert e.value.code == 1
    r.textures(run.scene.textures())
    r.normal_maps(run.scene.normal_maps())
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
    by_hand = np.zeros(2, p.capi.MICROFACET_DT)
    by_hand[0] = (1, 0, 0.5, 0.04)
    for make, why in ((lambda: walked(1), "queue or wide4"), (lambda: walked(2), "queue or wide4"), (lambda: walked(tree=True), "bvh_node tree")):
        refused(make, why, give=lambda r: r.microfacets(by_hand))


def test_the_baseline_kernel_the_ray_exchange_and_the_tolerance_mode_refuse_a_table(p, monkeypatch):
    """kernel variants 5 and 6 take worlds of the reference's feature set only: spheres under the sky gradient, here with a table given by hand; variant 1 too"""
    setenv(monkeypatch, TW.LDS)
    s = p.Scene.book1_final(SEED)   # a BVH of spheres in the LDS
    table = np.zeros(s.getWorldPtr().n_materials, p.capi.MICROFACET_DT)
    table[0] = (1, 0, 0.5, 0.04)    # the ground, a Lambertian
    assert s.arrays()[2]["type"][0] == 0
    cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
    for variant in (1, 5, 6):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED, variant=variant)
        why = "the baseline kernel \\(variant 1\\) reads no microfacet table" if variant == 1 else f"kernel variant {variant} reads no microfacet table"
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.microfacets(table)
        assert e.value.code == 1 and not r.kernel_microfacet()
        r.Render()
        r.close()
