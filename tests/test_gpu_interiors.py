"""Solid glass on the GPU: the device probes against the host batches, all sixteen INTR kernel forms — eight plain, eight under mode 48 — against
the whole-sample twins on a room of glass of every kind, seen from outside and from inside the glass box; every sigma zeroed against the facing-only twin, every
record off against the MFAC kernel's frame, the table taken away; sessions, ranks, the feature pass and the refusals.  Every comparison is bit for bit: with the
numpy twins (tests/_interior_twin.py, pinned by tests/test_interiors_cpu.py), which follow EVERY sample of the room, or with the renderer's own frame.  Frames are
24 x 16 at 8 spp and depth 8."""
import numpy as np
import pytest

import _interior_twin as IT
import _interior_worlds as IW
import _tri_worlds as TW
from _common import bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = IW.W, IW.H, IW.SPP, IW.DEPTH, IW.SEED
FORMS = list(IW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, IW.ENV_TREE]
VIEWS = [IW.OUTSIDE, IW.INSIDE]
LDS_FAST = (TW.BVH, 0, 2, 0, 0)
RECORDS = IW.RECORDS


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


def renderer(p, scene, form=LDS_FAST, mode=0, view=IW.OUTSIDE, spp=SPP):
    """a renderer of `scene` on the recipe of `form` (the caller has set its environment) that states the kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, IW.camera(p, view), scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_interior() and r.interiors_info() == {"enabled": True, "records": RECORDS}
    assert r.kernel_microfacet() and r.microfacets_info() == {"enabled": True, "records": 1} and not r.kernel_normal_map()
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
    assert r.kernel_triangles() and r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, IT.resolve(sums, spp))
    return sums


# ---- 1. the rule on the device ----------------------------------------------------------------------------------------------------------------------------
def test_the_probes_are_the_host_batches_bit_for_bit(p):
    aimed, expected = IW.aimed_cases()
    for cases in (IW.random_cases(), aimed):
        host = IW.run_cases(p.api.interior_batch, cases)
        dev = IW.run_cases(p.api.probe_interior, cases)
        for d, h, name in zip(dev, host, ("back", "eta", "T")):
            if d.dtype == np.uint32:
                assert (d == h).all(), (name, np.nonzero(d != h)[0][:5])
            else:
                assert bits_equal(d, h), (name, mismatch_report(d, h))
    assert (dev[0] == expected).all()
    x = IW.expf_samples(1 << 18)
    dev, host = p.api.probe_expf(x), p.api.expf_batch(x)
    assert bits_equal(dev, host), mismatch_report(dev, host)
    edge = p.api.probe_expf(np.array([0.0, -0.0, np.nan, -np.inf, -87.0, -1e30], F))
    assert edge[0] == 1 and edge[1] == 1 and (edge[2:] == 0).all()


# ---- 2. the sixteen forms -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_sums():
    return {}


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_is_the_twin(p, monkeypatch, first_sums, form, mode):
    """All 16 INTR keys, each reached by its recipe, on the room, from outside and from inside the glass box: the sums equal the whole-sample twin's on every
    pixel and those of the other forms; with every sigma zeroed they equal the facing-only twin's, the unedited loop of _path_twin over the wrapped walk; with
    every record off they are the MFAC kernel's frame of the room, which is _rglass_twin's; with the table taken away the renderer has the kernel and the frame
    it had before there was one."""
    setenv(monkeypatch, TW.FORMS[form][1])
    for view in VIEWS:
        run = IW.run(bool(mode), form[0] == TW.LIST, view)
        assert run.followed.all() and run.facing_followed.all() and run.off_followed.all()   # the twins leave no sample out
        assert all(v > 0 for v in run.stats.values()), run.stats
        r = renderer(p, run.scene, form, mode, view)
        sums = sums_of(r)
        assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
        assert bits_equal(sums.sum(axis=(0, 1)), run.sums.sum(axis=(0, 1)))   # the frame sums
        first = first_sums.setdefault((mode, view), sums)
        assert bits_equal(sums, first), mismatch_report(sums, first)
        r.interiors(IW.no_tint(run.interiors))   # the same kernel, no absorption: the facing alone
        assert r.kernel_interior() and r.interiors_info() == {"enabled": True, "records": RECORDS}
        facing = sums_of(r)
        assert bits_equal(facing, run.facing_sums), mismatch_report(facing, run.facing_sums)
        assert not bits_equal(facing, sums)
        r.interiors(IW.all_off(run.interiors))   # the same kernel, every record off
        assert r.kernel_interior() and r.interiors_info() == {"enabled": True, "records": 0}
        off = sums_of(r)
        assert bits_equal(off, run.off_sums), mismatch_report(off, run.off_sums)
        r.interiors(None)   # ... and without the table, on the MFAC kernel the renderer had: the same frame, bit for bit
        assert not r.kernel_interior() and r.kernel_microfacet() and not r.interiors_info()["enabled"]
        assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0)
        without = sums_of(r)
        r.close()
        assert bits_equal(without, off), mismatch_report(without, off)
        assert not bits_equal(off, facing)


def simple(p, frosted=False, traversal=0, record=True):
    """a floor, a tinted glass box and a clear ball on the world's own EXT 1 kernel: no image, no texture table and — unless frosted — no microfacet table"""
    s = p.Scene()
    floor, box, ball = s.Lambertian((0.5, 0.5, 0.5)), s.Dielectric((1, 1, 1), 1.5), s.Dielectric((1, 1, 1), 1.5)
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), floor)
    s.MakeBox((3.0, 0.2, 5.0), (5.0, 2.2, 7.0), box, rotate_y=15.0)
    s.MakeSphere((6.8, 1.0, 6), 1.0, ball)
    if record:
        s.set_interior(box, color=(0.4, 0.8, 0.6), at=1.0)
    if frosted:
        s.set_rough_glass(ball, 0.5)
    s.set_background(IW.BACKGROUND)
    s.set_traversal(traversal)
    s.BuildBVH_SAH()
    return s


def test_a_world_without_textures_or_microfacets_takes_an_interior_table(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    s = simple(p)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, IW.camera(p), s.getWorldPtr(), seed=SEED)
    assert r.kernel_interior() and r.interiors_info() == {"enabled": True, "records": 1}
    assert not r.textures_info()["enabled"] and not r.microfacets_info()["enabled"] and not r.normal_maps_info()["enabled"]
    on = sums_of(r)
    r.interiors(np.zeros(3, p.capi.INTERIOR_DT))
    all_off = sums_of(r)
    r.interiors(None)
    assert not r.kernel_interior() and not r.kernel_microfacet()
    off = sums_of(r)
    r.close()
    assert bits_equal(all_off, off), mismatch_report(all_off, off)
    assert not bits_equal(on, off)


# ---- 3. sessions ------------------------------------------------------------------------------------------------------------------------------------------------
def test_uneven_steps_the_table_on_off_on_and_mode_48_around_it(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run, env_run = IW.run(False), IW.run(True)
    r = renderer(p, run.scene)
    for n in (1, 4, 3):
        r.refine(n)
    stepped = r.refine_sums()
    assert bits_equal(stepped, run.sums), mismatch_report(stepped, run.sums)
    table = run.scene.interiors()
    r.interiors(table)   # unchanged: a no-op that keeps the refinement
    assert r.refine_info()["samples"] == SPP
    r.interiors(None)
    assert r.refine_info()["samples"] == 0 and not r.kernel_interior() and r.kernel_microfacet()
    off = sums_of(r)
    r.interiors(table)
    assert r.refine_info()["samples"] == 0 and r.kernel_interior()
    on = sums_of(r)
    r.interiors(None)
    off_again = sums_of(r)
    r.interiors(table)
    on_again = sums_of(r)
    r.close()
    assert bits_equal(on, run.sums) and bits_equal(on_again, on) and bits_equal(off_again, off) and bits_equal(off, run.off_sums)
    r = renderer(p, env_run.scene)   # mode 48 on and off around the table, and the table on and off under mode 48
    plain = sums_of(r)
    r.light_sampling(48)
    assert r.kernel_interior() and r.kernel_env_light() and r.kernel_light_tree()
    sampled = sums_of(r)
    assert bits_equal(sampled, env_run.sums), mismatch_report(sampled, env_run.sums)
    r.interiors(None)
    assert not r.kernel_interior() and r.kernel_env_light()
    sampled_off = sums_of(r)
    assert bits_equal(sampled_off, env_run.off_sums), mismatch_report(sampled_off, env_run.off_sums)
    r.interiors(env_run.scene.interiors())
    assert bits_equal(sums_of(r), sampled)
    r.light_sampling(0)
    assert r.kernel_interior() and not r.kernel_env_light()
    assert bits_equal(sums_of(r), plain)
    r.close()
    assert not bits_equal(plain, sampled)


# ---- 4. ranks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    run = IW.run(False)
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, IW.camera(p), run.scene.getWorldPtr(), 2, seed=SEED)
    assert m.microfacets_info() == {"enabled": True, "records": 1}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.interiors(None)
    m.Render()
    off = m.DownloadRenderbuffer()
    m.close()
    assert bits_equal(frame, run.frame), mismatch_report(frame, run.frame)
    assert bits_equal(off, IT.resolve(run.off_sums, SPP))


# ---- 5. the feature pass ------------------------------------------------------------------------------------------------------------------------------------------
def test_both_feature_modes_give_the_bits_they_give_without_the_table(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    for scene, textured in ((IW.run(False).scene, True), (simple(p), False)):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, IW.camera(p), scene.getWorldPtr(), seed=SEED)
        assert r.kernel_interior()
        r.enable_aov(textured=textured)
        r.refine(SPP)
        on = r.aov_sums()
        r.interiors(None)
        r.refine(SPP)
        off = r.aov_sums()
        r.close()
        assert bits_equal(on, off), mismatch_report(on, off)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_and_the_kernel_as_they_were(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = IW.run(False)
    table = run.scene.interiors()
    mats = run.scene.arrays()[2]["type"]
    r = renderer(p, run.scene)
    form = r.kernel_form()
    glass = [int(i) for i in np.nonzero(mats == 2)[0]]
    solid = [i for i in glass if table["on"][i] == 1][0]
    lam, metal, light = (int(np.nonzero(mats == t)[0][0]) for t in (0, 1, 4))
    bad = []
    for at in (lam, metal, light):
        t = table.copy()
        t[at] = (1, (0.1, 0.1, 0.1))
        bad.append((t, "belongs on a dielectric alone"))
    for kind in (2, 3, 7):
        t = table.copy()
        t["on"][solid] = kind
        bad.append((t, "on is 0"))
    for value in (-0.5, np.nan, np.inf):
        t = table.copy()
        t["sigma"][solid, 1] = value
        bad.append((t, "absorption coefficient"))
    bad += [(table[:-1], "records for a world of"), (np.concatenate([table, table[:1]]), "records for a world of")]
    for t, why in bad:
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.interiors(t)
        assert e.value.code == 1 and r.kernel_interior() and r.kernel_form() == form and r.interiors_info() == {"enabled": True, "records": RECORDS}
    for mode in (1, 2, 4, 16, 32):   # §29's refusals, from the side of the mode
        with pytest.raises(p.capi.RtError, match=f"light-sampling mode {mode} has no kernel that reads one") as e:
            r.light_sampling(mode)
        assert e.value.code == 1 and r.light_sampling_mode() == 0 and r.kernel_interior()
    sums = sums_of(r)   # ... and the renderer is as usable as it was
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    r.close()

    def refused(make, why, give, mode=0):
        """a renderer without the table refuses it: code 1, no interior kernel, no table, the mode it had, and as usable as it was"""
        r = make()
        with pytest.raises(p.capi.RtError, match=why) as e:
            give(r)
        assert e.value.code == 1 and not r.kernel_interior() and r.interiors_info() == {"enabled": False, "records": 0} and r.light_sampling_mode() == mode
        r.Render()
        r.close()

    # ... and from the side of the table: each mode that is on refuses it — 1, 2, 4 and 16 on the room, 32 on the room under the sky map
    for mode in (1, 2, 4, 16, 32):
        scene = (IW.run(True) if mode == 32 else run).scene
        world = scene.getWorldPtr()
        del world.interiors, world.microfacets   # a renderer without either table (the frosted record refuses these modes too), to give the table to

        def lit(mode=mode, world=world):
            r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, IW.camera(p), world, seed=SEED)
            r.light_sampling(mode)
            assert r.light_sampling_mode() == mode
            return r
        refused(lit, f"light-sampling mode {mode} is on, which has no kernel that reads an interior table", lambda r, scene=scene: r.interiors(scene.interiors()), mode)
    s = p.Scene.book1_final(SEED)   # variants 1, 5 and 6 refuse a table as they refuse §29's
    types = s.arrays()[2]["type"]
    by_hand = np.zeros(len(types), p.capi.INTERIOR_DT)
    by_hand[int(np.nonzero(types == 2)[0][0])] = (1, (0.5, 0.5, 0.5))
    cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
    for variant in (1, 5, 6):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED, variant=variant)
        with pytest.raises(p.capi.RtError, match="reads no interior table") as e:
            r.interiors(by_hand)
        assert e.value.code == 1 and not r.kernel_interior()
        r.close()
    t = np.zeros(3, p.capi.INTERIOR_DT)
    t[1] = (1, (0.5, 0.5, 0.5))
    for traversal in (1, 2):   # the queue and wide4 walks
        s = simple(p, traversal=traversal, record=False)
        refused(lambda s=s: p.Renderer.MakeRenderer(W, H, SPP, DEPTH, IW.camera(p), s.getWorldPtr(), seed=SEED), "queue or wide4", lambda r: r.interiors(t))
    s = p.Scene()   # a bvh_node tree: two balls, the second of glass; the table comes by hand
    one, two = s.MakeSphere((3.5, 1.0, 6), 1.0, s.Lambertian((0.5, 0.5, 0.5))), s.MakeSphere((6.5, 1.0, 6), 1.0, s.Dielectric((1, 1, 1), 1.5))
    s.set_world_node_tree(s.bvh_node(p.Scene.prim_ref(one), p.Scene.prim_ref(two)))
    by_hand = np.zeros(2, p.capi.INTERIOR_DT)
    by_hand[1] = (1, (0.5, 0.5, 0.5))
    refused(lambda: p.Renderer.MakeRenderer(W, H, SPP, DEPTH, IW.camera(p), s.getWorldPtr(), seed=SEED), "a bvh_node tree renders on a walk that reads no interior table",
            lambda r: r.interiors(by_hand))
