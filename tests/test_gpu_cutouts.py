"""Alpha cutouts on the GPU: the device probe against the host batch, all sixteen CUT kernel forms — eight plain, eight under mode 48 — against
the whole-sample twin on a room of masked surfaces; the frame against the same world without the table; opaque masks against the renderer without a table, an
empty mask against the world without the surface; the table's edges, sessions, ranks and the refusals.  Every comparison is bit for bit: with the numpy twin
(tests/_cutout_twin.py, pinned by tests/test_cutouts_cpu.py), which follows EVERY sample of the room, or with the renderer's own frame.  Frames are 24 x 16 at
8 spp and depth 8."""
import numpy as np
import pytest

import _cutout_worlds as CW
import _env_tree_twin as VT
import _tri_worlds as TW
from _common import bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = CW.W, CW.H, CW.SPP, CW.DEPTH, CW.SEED
FORMS = list(CW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, CW.ENV_TREE]
LDS_FAST = (TW.BVH, 0, 2, 0, 0)
GLOBAL_FAST = (TW.BVH, 0, 2, 1, 1)
RECORDS = CW.RECORDS


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


def form_of(form, mode, cut=True):
    """what kernel_form() reports: the CUT forms are EXT 2 forms, whatever the world; without a table the room, which has no textured material, is an EXT 1 world
    under its constant background and an EXT 2 world under the sky map (the rooms of mode 48)"""
    return dict(TW.kernel_form_of(form, nee=1 if mode else 0), ext=2 if cut or mode else 1)


def renderer(p, scene, form=LDS_FAST, mode=0, world=None, cut=True, records=RECORDS):
    """a renderer of `scene` on the recipe of `form` (the caller has set its environment) that states the kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, CW.camera(p), scene.getWorldPtr() if world is None else world, seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_cutout() == cut and r.cutouts_info() == {"enabled": cut, "records": records if cut else 0}
    assert r.kernel_interior() == cut and r.kernel_microfacet() == cut and r.textures_info()["enabled"]
    assert r.kernel_form() == form_of(form, mode, cut), r.kernel_form()
    assert r.kernel_triangles() and r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def without_table(scene):
    world = scene.getWorldPtr()
    del world.cutouts
    return world


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, VT.resolve(sums, spp))
    return sums


# ---- 1. the rule on the device ----------------------------------------------------------------------------------------------------------------------------
def test_the_probe_is_the_host_batch_bit_for_bit(p):
    table, records = p.api.texture_table(CW.case_table()), CW.case_records()
    for name, quads, uv, rays, t, material in CW.batches():
        host = p.api.cutout_batch(table, quads, uv, rays, t, records, material)
        dev = p.api.probe_cutout(table, quads, uv, rays, t, records, material)
        assert (dev[0] == host[0]).all(), (name, np.nonzero(dev[0] != host[0])[0][:5])
        assert bits_equal(dev[1], host[1]), (name, mismatch_report(dev[1], host[1]))
        assert bits_equal(dev[2], host[2]), (name, mismatch_report(dev[2], host[2]))
        assert 0 < host[0].sum() < len(t)


# ---- 2. the sixteen forms -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_sums():
    return {}


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_is_the_twin(p, monkeypatch, first_sums, form, mode):
    """All 16 CUT keys, each reached by its recipe, on the room: the sums equal the whole-sample twin's on every pixel and those of the other forms; with the
    table taken away the renderer has the kernel it had before there was one and renders the twin's frame of the room with whole cards."""
    setenv(monkeypatch, TW.FORMS[form][1])
    run = CW.run(bool(mode), form[0] == TW.LIST)
    assert run.followed.all() and run.off_followed.all()   # the twin leaves no sample out
    r = renderer(p, run.scene, form, mode)
    sums = sums_of(r)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(sums.sum(axis=(0, 1)), run.sums.sum(axis=(0, 1)))   # the frame sums
    first = first_sums.setdefault(mode, sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)
    r.cutouts(None)
    assert not r.kernel_cutout() and not r.kernel_interior() and not r.kernel_microfacet() and not r.cutouts_info()["enabled"]
    assert r.kernel_form() == form_of(form, mode, cut=False)
    off = sums_of(r)
    r.close()
    assert bits_equal(off, run.off_sums), mismatch_report(off, run.off_sums)


def test_the_frame_differs_from_the_world_without_the_table(p, monkeypatch):
    """what the feature is for: holes are seen through.  Without the rule a card is a solid rectangle, and this fails."""
    setenv(monkeypatch, TW.LDS)
    run = CW.run(False)
    r = renderer(p, run.scene)
    on = sums_of(r)
    r.close()
    r = renderer(p, run.scene, world=without_table(run.scene), cut=False)
    off = sums_of(r)
    r.close()
    differ = (on.view(np.uint32) != off.view(np.uint32)).any(axis=2)
    assert differ.sum() > 100, differ.sum()
    assert bits_equal(off, run.off_sums) and bits_equal(on, run.sums)


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", [LDS_FAST, GLOBAL_FAST], ids=["lds", "global"])
def test_every_kind_of_record_live_beside_the_masks(p, monkeypatch, form, mode):
    """what `CUT` implies `INTR` is for: masked cards beside a solid-glass box with an interior record, a rough conductor and a coated card that is masked too,
    in one launch on a sub-header whose three lanes are all live — against the one loop of _path_twin with the cutout walk as its trace; with every sigma zero
    against the road of the wrapped walk (_interior_twin.solid_walk); without the cutout table on the INTR form, against the loop with _tri_twin's walk"""
    import _interior_worlds as IW
    setenv(monkeypatch, TW.FORMS[form][1])
    run = CW.run(bool(mode), live=True)
    assert run.followed.all() and run.off_followed.all() and run.facing_followed.all()
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, CW.camera(p), run.scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_cutout() and r.kernel_interior() and r.kernel_microfacet() and r.kernel_form() == form_of(form, mode)
    assert r.cutouts_info() == {"enabled": True, "records": RECORDS} and r.interiors_info() == {"enabled": True, "records": 1}
    assert r.microfacets_info() == {"enabled": True, "records": 2}
    sums = sums_of(r)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    r.interiors(IW.no_tint(run.scene.interiors()))
    assert r.kernel_cutout()
    facing = sums_of(r)
    assert bits_equal(facing, run.facing_sums), mismatch_report(facing, run.facing_sums)
    r.interiors(run.scene.interiors())
    r.cutouts(None)
    assert not r.kernel_cutout() and r.kernel_interior() and r.kernel_microfacet()
    off = sums_of(r)
    r.close()
    assert bits_equal(off, run.off_sums), mismatch_report(off, run.off_sums)
    assert not bits_equal(sums, off) and not bits_equal(sums, facing)


# ---- 3. masks that decide nothing, and masks that decide everything --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", [LDS_FAST, GLOBAL_FAST], ids=["lds", "global"])
def test_an_opaque_mask_on_every_material_changes_no_bit(p, monkeypatch, form, mode):
    """the CUT form with a lookup at every candidate against the kernel the renderer runs without a table, which the older suites hold to the oracle"""
    setenv(monkeypatch, TW.FORMS[form][1])
    scene = CW.room(p, env=bool(mode), records=False)
    r = renderer(p, scene, form, mode, cut=False)
    plain = sums_of(r)
    table = CW.all_of(p, scene, scene.names["images"]["white"])
    r.cutouts(table)
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": int((table["on"] != 0).sum())}
    opaque = sums_of(r)
    r.cutouts(np.zeros(len(table), p.capi.CUTOUT_DT))   # ... and with every record off
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": 0}
    all_off = sums_of(r)
    r.close()
    assert bits_equal(opaque, plain), mismatch_report(opaque, plain)
    assert bits_equal(all_off, plain), mismatch_report(all_off, plain)


def test_an_empty_mask_on_a_list_world_is_the_world_without_the_surface(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    form = (TW.LIST, 1, 2, 0, 0)
    scene = CW.room(p, as_list=True, records=False)
    scene.set_cutout(scene.names["fence"], scene.names["images"]["black"])
    r = renderer(p, scene, form, records=1)
    masked = sums_of(r)
    r.close()
    r = renderer(p, CW.room(p, as_list=True, fence=False, records=False), form, cut=False)
    absent = sums_of(r)
    r.close()
    assert bits_equal(masked, absent), mismatch_report(masked, absent)


# ---- 4. the table's edges ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_last_record_of_the_coordinates_and_a_world_without_any(p, monkeypatch):
    """in the list world the card's second triangle is the world's last, so its coordinates are the last record of the table; without coordinates the world has
    no table at all"""
    setenv(monkeypatch, TW.LDS)
    run = CW.run(False, True)
    uv = run.scene.texture_coords()
    assert len(uv) == run.scene.n_triangles() == 3 and (uv[-1]["t2"] == (0, 2)).all() and run.stats["rejected_tri_uv"] >= 100
    r = renderer(p, run.scene, (TW.LIST, 1, 2, 0, 0))
    sums = sums_of(r)
    r.close()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    bare = CW.run(False, uvs=False)
    assert len(bare.scene.texture_coords()) == 0 and bare.followed.all() and bare.stats["rejected_tri_uv"] == 0 and bare.stats["rejected_tri_plain"] >= 100
    r = renderer(p, bare.scene)
    assert not r.texture_coords_info()["enabled"]
    sums = sums_of(r)
    r.close()
    assert bits_equal(sums, bare.sums), mismatch_report(sums, bare.sums)
    assert not bits_equal(bare.sums, run.sums)


# ---- 5. sessions and ranks ----------------------------------------------------------------------------------------------------------------------------------------
def test_uneven_steps_and_the_table_off_on_off(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = CW.run(False)
    r = renderer(p, run.scene)
    for n in (1, 4, 3):
        r.refine(n)
    stepped = r.refine_sums()
    assert bits_equal(stepped, run.sums), mismatch_report(stepped, run.sums)
    table = run.scene.cutouts()
    r.cutouts(table)   # unchanged: a no-op that keeps the refinement
    assert r.refine_info()["samples"] == SPP
    r.cutouts(None)
    assert r.refine_info()["samples"] == 0 and not r.kernel_cutout()
    off = sums_of(r)
    r.cutouts(table)
    assert r.refine_info()["samples"] == 0 and r.kernel_cutout()
    on = sums_of(r)
    r.cutouts(None)
    off_again = sums_of(r)
    r.close()
    assert bits_equal(on, run.sums) and bits_equal(off, run.off_sums) and bits_equal(off_again, off)


def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    run = CW.run(False)
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, CW.camera(p), run.scene.getWorldPtr(), 2, seed=SEED)
    assert m.cutouts_info() == {"enabled": True, "records": RECORDS}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.cutouts(None)
    m.Render()
    off = m.DownloadRenderbuffer()
    m.close()
    assert bits_equal(frame, run.frame), mismatch_report(frame, run.frame)
    assert bits_equal(off, VT.resolve(run.off_sums, SPP))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_the_kernel_and_the_next_frame_as_they_were(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = CW.run(False)
    table, names = run.scene.cutouts(), run.scene.names
    r = renderer(p, run.scene)
    form = r.kernel_form()

    def still_on():
        return r.kernel_cutout() and r.kernel_form() == form and r.cutouts_info() == {"enabled": True, "records": RECORDS}
    bad = []
    t = table.copy()
    t[names["light"]] = (1, 1, 0.5, 0)
    bad.append((t, "a light or a medium takes no cutout"))
    for kind in (2, 7):
        t = table.copy()
        t["on"][names["fence"]] = kind
        bad.append((t, "on is 0"))
    for value in (-0.5, 1.5, np.nan, np.inf):
        t = table.copy()
        t["cutoff"][names["card"]] = value
        bad.append((t, "a cutoff must be finite and in"))
    t = table.copy()
    t["image"][names["card"]] = 256
    bad.append((t, "an image index lies in"))
    bad += [(table[:-1], "records for a world of"), (np.concatenate([table, table[:1]]), "records for a world of")]
    for t, why in bad:
        with pytest.raises(p.capi.RtError, match=why) as e:
            r.cutouts(t)
        assert e.value.code == 1 and still_on()
    for mode in (1, 2, 4, 16, 32):   # from the side of the mode
        with pytest.raises(p.capi.RtError, match=f"cutout table, and light-sampling mode {mode} has no kernel that reads one") as e:
            r.light_sampling(mode)
        assert e.value.code == 1 and r.light_sampling_mode() == 0 and still_on()
    for textured in (False, True):   # the feature pass does not know the rule
        with pytest.raises(p.capi.RtError, match="the feature pass does not know the cutout rule") as e:
            r.enable_aov(textured=textured)
        assert e.value.code == 1 and still_on()
    t = table.copy()
    t[names["glass"]] = (1, 1, 0.5, 0)
    interiors = np.zeros(len(table), p.capi.INTERIOR_DT)
    interiors[names["glass"]] = (1, (0.1, 0.1, 0.1))
    r.cutouts(t)   # a cutout on glass is a cutout; then the interior record is refused, and with the interior record on the cutout is
    with pytest.raises(p.capi.RtError, match="a holed solid has no inside"):
        r.interiors(interiors)
    assert not r.interiors_info()["enabled"]
    r.cutouts(table)
    r.interiors(interiors)
    with pytest.raises(p.capi.RtError, match="a holed solid has no inside"):
        r.cutouts(t)
    r.interiors(None)
    assert still_on()
    # launch-time: a texture table that has lost the entry a record names is found before any kernel runs, and leaves everything as it was
    records, texels = run.scene.textures()
    short = (records[:2].copy(), texels[:int(records[2]["first"])].copy())
    r.refine(2)
    r.textures(short)
    with pytest.raises(p.capi.RtError, match="a cutout record of the world names image") as e:
        r.refine(1)
    assert e.value.code == 1 and still_on()
    r.textures((records, texels))
    sums = sums_of(r)   # ... and the renderer is as usable as it was
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    r.close()

    def refused(make, why, give, mode=0):
        """a renderer without the table refuses it: code 1, no cutout kernel, no table, the mode it had, and as usable as it was"""
        r = make()
        with pytest.raises(p.capi.RtError, match=why) as e:
            give(r)
        assert e.value.code == 1 and not r.kernel_cutout() and r.cutouts_info() == {"enabled": False, "records": 0} and r.light_sampling_mode() == mode
        r.Render()
        r.close()

    def bare(scene=run.scene, **kw):
        return p.Renderer.MakeRenderer(W, H, SPP, DEPTH, CW.camera(p), without_table(scene), seed=SEED, **kw)
    for mode in (1, 2, 4, 16, 32):   # each mode that is on refuses the table — 32 on the room under the sky map
        scene = (CW.run(True) if mode == 32 else run).scene

        def lit(mode=mode, scene=scene):
            r = bare(scene)
            r.light_sampling(mode)
            return r
        refused(lit, f"light-sampling mode {mode} is on, which has no kernel that reads a cutout table", lambda r, scene=scene: r.cutouts(scene.cutouts()), mode)
    for textured in (False, True):
        def featured(textured=textured):
            r = bare()
            r.enable_aov(textured=textured)
            return r
        refused(featured, "feature buffers are on, and the feature pass does not know the cutout rule", lambda r: r.cutouts(table))

    def untextured():
        r = bare()
        r.textures(None)
        return r
    r = untextured()   # (without its table the room cannot launch at all: the refusal alone is checked)
    with pytest.raises(p.capi.RtError, match="no texture table to take a mask from") as e:
        r.cutouts(table)
    assert e.value.code == 1 and not r.kernel_cutout() and not r.cutouts_info()["enabled"]
    r.close()
    for variant in (1, 5, 6):
        s = p.Scene.book1_final(SEED)
        by_hand = np.zeros(len(s.arrays()[2]), p.capi.CUTOUT_DT)
        by_hand[0] = (1, 0, 0.5, 0)
        cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED, variant=variant)
        with pytest.raises(p.capi.RtError, match="reads no cutout table") as e:
            r.cutouts(by_hand)
        assert e.value.code == 1 and not r.kernel_cutout()
        r.close()

    def walked(traversal):
        s = p.Scene()
        s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s.Lambertian((0.5, 0.5, 0.5)))
        s.MakeSphere((0, 1, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))
        s.set_background(CW.BACKGROUND)
        s.set_traversal(traversal)
        s.BuildBVH_SAH()
        return s
    t2 = np.zeros(2, p.capi.CUTOUT_DT)
    t2[0] = (1, 1, 0.5, 0)
    for traversal in (1, 2):   # the queue and wide4 walks
        s = walked(traversal)
        refused(lambda s=s: p.Renderer.MakeRenderer(W, H, SPP, DEPTH, CW.camera(p), s.getWorldPtr(), seed=SEED), "queue or wide4", lambda r: r.cutouts(t2))
    s = p.Scene()   # a bvh_node tree
    one, two = s.MakeSphere((-1.5, 1.0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5))), s.MakeSphere((1.5, 1.0, 0), 1.0, s.Metal((0.8, 0.8, 0.8), 0.1))
    s.set_world_node_tree(s.bvh_node(p.Scene.prim_ref(one), p.Scene.prim_ref(two)))
    refused(lambda: p.Renderer.MakeRenderer(W, H, SPP, DEPTH, CW.camera(p), s.getWorldPtr(), seed=SEED), "a bvh_node tree renders on a walk that reads no cutout table",
            lambda r: r.cutouts(t2))
