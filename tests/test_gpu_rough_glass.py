"""Rough glass on the GPU: the device probe against the host batch, all sixteen MFAC kernel forms — eight plain, eight under mode 48 — against
the whole-sample twin on a room with a frosted ball and a frosted, mapped pane, the glass records off against §29's frames, sessions, ranks, the feature pass
and the refusals.  Every comparison is bit for bit: with the numpy twin (tests/_rglass_twin.py, pinned by tests/test_rough_glass_cpu.py), which follows EVERY
sample of the room, or with the renderer's own frame.  Frames are 24 x 16 at 8 spp and depth 6."""
import numpy as np
import pytest

import _rglass_twin as GT
import _rglass_worlds as GW
import _tri_worlds as TW
from _common import bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = GW.W, GW.H, GW.SPP, GW.DEPTH, GW.SEED
FORMS = list(GW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, GW.ENV_TREE]
LDS_FAST = (TW.BVH, 0, 2, 0, 0)
RECORDS = 7   # §29's five, the frosted ball, the pane


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


def renderer(p, scene, form=LDS_FAST, mode=0, spp=SPP):
    """a renderer of `scene` on the recipe of `form` (the caller has set its environment) that states the kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, GW.camera(p), scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_microfacet() and r.microfacets_info() == {"enabled": True, "records": RECORDS} and not r.kernel_normal_map()
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
    assert r.kernel_triangles() and r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, GT.resolve(sums, spp))
    return sums


# ---- 1. the rule on the device ----------------------------------------------------------------------------------------------------------------------------
def test_the_probe_is_the_host_batch_bit_for_bit(p):
    aimed, expected, _ = GW.aimed_cases()
    for cases in (GW.random_cases(), aimed):
        host = GW.run_cases(p.api.rough_glass_batch, cases)
        dev = GW.run_cases(p.api.probe_rough_glass, cases)
        for d, h, name in zip(dev, host, ("direction", "weight", "way", "draws")):
            if d.dtype == np.uint32:
                assert (d == h).all(), (name, np.nonzero(d != h)[0][:5])
            else:
                assert bits_equal(d, h), (name, mismatch_report(d, h))
    assert set(dev[2].tolist()) == set(GT.WAYS)   # the aimed cases leave the rule on the device by every way out, as on the host
    assert all(e == 0 or e == w for e, w in zip(expected, dev[2]))


# ---- 2. the sixteen forms -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_sums():
    return {}


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_is_the_twin(p, monkeypatch, first_sums, form, mode):
    """All 16 MFAC keys, each reached by its recipe, on §29's room with a frosted ball and a frosted pane under the roughness map: the sums equal the whole-sample
    twin's on every pixel; with the glass records off they equal the twin's without them (which is §29's twin's); with the table taken away, the normal-map
    kernel's frame is the twin's without any record."""
    run = GW.run(bool(mode), as_list=form[0] == TW.LIST)
    st = run.stats
    assert run.followed.all()                                              # the twin leaves no sample out
    for key in ("rg_reflected", "rg_transmitted", "rg_absorbed", "rg_total", "rg_back", "rg_mapped", "glass", "recorded"):
        assert st[key] > 0, (key, st)
    setenv(monkeypatch, TW.FORMS[form][1])
    r = renderer(p, run.scene, form, mode)
    sums = sums_of(r)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(sums.sum(axis=(0, 1)), run.sums.sum(axis=(0, 1)))   # the frame sums
    first = first_sums.setdefault(mode, sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)
    r.microfacets(run.mfacs_clear)   # the same kernel, the glass clear: the frame of the room without glass records
    assert r.kernel_microfacet() and r.microfacets_info() == {"enabled": True, "records": RECORDS - 2}
    clear = sums_of(r)
    assert bits_equal(clear, run.clear_sums), mismatch_report(clear, run.clear_sums)
    assert not bits_equal(clear, sums)
    r.microfacets(None)    # ... and without the table, on the normal-map kernel the renderer had: the frame without any record
    assert not r.kernel_microfacet() and r.kernel_normal_map()
    without = sums_of(r)
    r.close()
    bare, followed = GT.frame_samples(*run.args, None, run.table, **run.lights)
    assert followed.all() and bits_equal(without, GT.in_order_sums(bare)), mismatch_report(without, GT.in_order_sums(bare))


def simple(p):
    """a floor, a frosted ball and a clear one on the world's own EXT 1 kernel: no image, no texture table"""
    s = p.Scene()
    floor, frosted, clear = s.Lambertian((0.5, 0.5, 0.5)), s.Dielectric((1, 1, 1), 1.5), s.Dielectric((1, 1, 1), 1.5)
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), floor)
    s.MakeSphere((3.5, 1.0, 6), 1.0, frosted)
    s.MakeSphere((6.5, 1.0, 6), 1.0, clear)
    s.set_rough_glass(frosted, 0.5)
    s.set_background(GW.BACKGROUND)
    s.BuildBVH_SAH()
    return s


def test_a_world_without_textures_takes_a_glass_record(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    s = simple(p)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, GW.camera(p), s.getWorldPtr(), seed=SEED)
    assert r.kernel_microfacet() and r.microfacets_info() == {"enabled": True, "records": 1} and not r.textures_info()["enabled"]
    on = sums_of(r)
    r.microfacets(np.zeros(3, p.capi.MICROFACET_DT))
    all_off = sums_of(r)
    r.microfacets(None)
    assert not r.kernel_microfacet()
    off = sums_of(r)
    r.close()
    assert bits_equal(all_off, off), mismatch_report(all_off, off)
    assert not bits_equal(on, off)


# ---- 3. sessions ------------------------------------------------------------------------------------------------------------------------------------------------
def test_uneven_steps_and_the_table_on_off_on(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = GW.run(False)
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
    r.microfacets(None)
    off_again = sums_of(r)
    r.microfacets(table)
    on_again = sums_of(r)
    r.close()
    assert bits_equal(on, run.sums) and bits_equal(on_again, on) and bits_equal(off_again, off) and not bits_equal(off, on)


# ---- 4. ranks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    run = GW.run(False)
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, GW.camera(p), run.scene.getWorldPtr(), 2, seed=SEED)
    assert m.microfacets_info() == {"enabled": True, "records": RECORDS}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.close()
    assert bits_equal(frame, run.frame), mismatch_report(frame, run.frame)


# ---- 5. the feature pass ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_feature_pass_does_not_read_the_table(p, monkeypatch):
    """textured mode on the room, plain mode on a world it accepts: the feature sums with the table on are the sums with it off"""
    setenv(monkeypatch, TW.LDS)
    for scene, textured in ((GW.run(False).scene, True), (simple(p), False)):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, GW.camera(p), scene.getWorldPtr(), seed=SEED)
        assert r.kernel_microfacet()
        r.enable_aov(textured=textured)
        r.refine(SPP)
        on = r.aov_sums()
        r.microfacets(None)
        r.refine(SPP)
        off = r.aov_sums()
        r.close()
        assert bits_equal(on, off), mismatch_report(on, off)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_and_the_kernel_as_they_were(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = GW.run(False)
    table = run.scene.microfacets()
    mats = run.scene.arrays()[2]["type"]
    r = renderer(p, run.scene)
    form = r.kernel_form()
    glass = [int(i) for i in np.nonzero(mats == 2)[0]]
    frosted = [i for i in glass if table["on"][i] == GT.GLASS][0]
    clear = [i for i in glass if table["on"][i] == 0][0]
    lam, metal, light = (int(np.nonzero(mats == t)[0][0]) for t in (0, 1, 4))
    bad = []
    for at, why in ((lam, "belongs on a dielectric alone"), (metal, "belongs on a dielectric alone"), (light, "belongs on a dielectric alone")):
        for kind in (GT.GLASS, GT.GLASS_MAPPED):
            t = table.copy()
            t[at] = (kind, 0, 0.5, 0.0)
            bad.append((t, why))
    for kind, why in ((1, "takes no microfacet record"), (2, "takes no microfacet record"), (3, "on is 0"), (5, "on is 0"), (7, "on is 0")):   # today's words
        t = table.copy()
        t[clear] = (kind, 0, 0.5, 0.04)
        bad.append((t, why))
    t = table.copy()
    t[lam] = (3, 0, 0.5, 0.04)
    bad.append((t, "on is 0"))
    rough, nan, spec, image = (table.copy() for _ in range(4))
    rough["roughness"][frosted], nan["roughness"][frosted], spec["specular"][frosted] = 1.5, np.nan, 0.04
    image[frosted] = (GT.GLASS_MAPPED, 256, 0.5, 0.0)
    bad += [(rough, "rough-glass record's roughness"), (nan, "rough-glass record's roughness"), (spec, "reads no specular"), (image, "rough-glass record's image index"),
            (table[:-1], "records for a world of")]
    for t, why in bad:
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.microfacets(t)
        assert e.value.code == 1 and r.kernel_microfacet() and r.kernel_form() == form and r.microfacets_info() == {"enabled": True, "records": RECORDS}
    r.normal_maps(None)   # (the room's normal map refuses these modes too, and first)
    for mode in (1, 2, 4, 16, 32):   # §29's refusals cover a table with glass records unchanged
        with pytest.raises(p.capi.RtError, match=f"microfacet table, and light-sampling mode {mode} has no kernel that reads one") as e:
            r.light_sampling(mode)
        assert e.value.code == 1 and r.light_sampling_mode() == 0 and r.kernel_microfacet()
    only_pane = np.zeros(len(table), p.capi.MICROFACET_DT)   # a mapped glass record alone needs its entry at launch, as the other mapped kind does
    pane = [i for i in glass if table["on"][i] == GT.GLASS_MAPPED][0]
    only_pane[pane] = table[pane]
    r.microfacets(only_pane)
    r.textures(None)
    with pytest.raises(p.capi.RtError, match="roughness map of the world names image|image material of the world names image") as e:
        r.Render()
    assert e.value.code == 1
    r.textures(run.scene.textures())
    r.normal_maps(run.scene.normal_maps())
    r.microfacets(table)
    sums = sums_of(r)   # ... and the renderer is as usable as it was
    r.close()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    s = p.Scene.book1_final(SEED)   # variants 1, 5 and 6 refuse a glass record as they refuse any
    types = s.arrays()[2]["type"]
    by_hand = np.zeros(len(types), p.capi.MICROFACET_DT)
    by_hand[int(np.nonzero(types == 2)[0][0])] = (GT.GLASS, 0, 0.5, 0.0)
    cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
    for variant in (1, 5, 6):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED, variant=variant)
        with pytest.raises(p.capi.RtError, match="reads no microfacet table") as e:
            r.microfacets(by_hand)
        assert e.value.code == 1 and not r.kernel_microfacet()
        r.close()
