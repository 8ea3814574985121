"""The cutout kernels and the full feature pass in the live room, on the GPU: all sixteen CUT instantiations of render_kernel_stream render the
masked room of tests/_live_worlds.py — masked surfaces with a moving sphere, a sphere of medium and the solid tinted box behind their holes, a leaf of image
material under vertex normals, a normal map and the alpha of its own picture, every rider of the tail live at once — under the three cameras, and are compared
with the composed whole-sample twin (the rule in the leaf phase, then smooth normal and map at the hit the walk kept), which follows EVERY sample: in-order
refinement sums and frames, bit for bit on every pixel.  Mode RT_AOV_FULL runs in the same room under the three cameras against the extended feature twin.
Frames are 24 x 16 at 8 spp and depth 8.  Mode 48 refuses a world with a constant medium, so its room has none."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _interior_twin as IT
import _live_worlds as LW
import _tri_worlds as TW
from _common import ROOT, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = LW.W, LW.H, LW.SPP, LW.DEPTH, LW.SEED
FORMS = list(LW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
MODES = [0, LW.ENV_TREE]
MODE_IDS = ["plain", "mode48"]
LDS_FAST, GLOBAL_FAST = (TW.BVH, 0, 2, 0, 0), (TW.BVH, 0, 2, 1, 0)
LIST_LDS, LIST_GLOBAL = (TW.LIST, 1, 2, 0, 0), (TW.LIST, 1, 2, 1, 1)
CUT_RECORDS, MFAC_RECORDS = 5, 6   # the leaf, the grain, the steel, the tiles and the opaque bronze; the plain room's four coats and conductors, the grain and the steel


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


def renderer(p, tw, kind, form=LDS_FAST, mode=0, spp=SPP, scene=None):
    """a renderer of the masked room on the recipe of `form` (the caller has set its environment), under camera `kind`, that states the CUT kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, tw.cams[kind], (scene or tw.scene).getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": CUT_RECORDS}
    assert r.kernel_interior() and r.kernel_microfacet() and r.textures_info()["enabled"] and r.normal_maps_info()["enabled"]
    assert r.interiors_info() == {"enabled": True, "records": 1} and r.microfacets_info() == {"enabled": True, "records": MFAC_RECORDS}
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
    assert r.kernel_triangles() and r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, IT.resolve(sums, spp))
    return sums


def push(r, table):
    nmaps, mfacs, interiors, cutouts = table
    r.normal_maps(nmaps)
    r.microfacets(mfacs)
    r.interiors(interiors)
    r.cutouts(cutouts)


def against_the_twin(r, tw, kind, variant, first_sums, key):
    """the renderer's sums under the tables of `variant` equal the twin's cached frame, and those of every form before it that rendered the same key"""
    f = tw.frame(variant, kind)
    assert f.followed.all()
    push(r, LW.tables_of(tw.table, variant))
    sums = sums_of(r)
    assert bits_equal(sums, f.sums), (variant, kind, mismatch_report(sums, f.sums))
    assert bits_equal(sums.sum(axis=(0, 1)), f.sums.sum(axis=(0, 1)))
    first = first_sums.setdefault(key + (variant, kind), sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)
    return sums


@pytest.fixture(scope="module")
def first_sums():
    return {}


# ---- 1. the sixteen CUT keys ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_cut_instantiation_is_the_twin_in_the_live_room(p, monkeypatch, first_sums, form, mode):
    """One shape of kernel, plain or under mode 48, under the camera its index picks: the CUT key with every table on; the same key with every cutout record
    off; the INTR key with the cutout table taken away; the CUT key with every sigma zero.  Each equals the twin on every pixel and the other forms of its
    world and camera, and the four frames differ pairwise where the twin's differ."""
    setenv(monkeypatch, TW.FORMS[form][1])
    kind = LW.CAMERAS[FORMS.index(form) % 3]
    tw = LW.run(bool(mode), form[0] == TW.LIST, None, True)
    key = (mode, form[0])
    r = renderer(p, tw, kind, form, mode)
    got = {LW.ALL: against_the_twin(r, tw, kind, LW.ALL, first_sums, key)}
    got[LW.CUTOUTS_OFF] = against_the_twin(r, tw, kind, LW.CUTOUTS_OFF, first_sums, key)
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": 0} and r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0)
    got[LW.NO_CUTOUTS] = against_the_twin(r, tw, kind, LW.NO_CUTOUTS, first_sums, key)
    assert not r.kernel_cutout() and r.kernel_interior() and r.kernel_microfacet() and not r.cutouts_info()["enabled"]
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0)
    got[LW.SIGMA_ZERO] = against_the_twin(r, tw, kind, LW.SIGMA_ZERO, first_sums, key)
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": CUT_RECORDS}
    r.close()
    assert bits_equal(got[LW.CUTOUTS_OFF], got[LW.NO_CUTOUTS])   # a table of records that are off decides nothing
    for a in LW.CUT_VARIANTS:
        for b in LW.CUT_VARIANTS:
            assert bits_equal(got[a], got[b]) == bits_equal(tw.frame(a, kind).sums, tw.frame(b, kind).sums), (a, b)
    assert not bits_equal(got[LW.ALL], got[LW.NO_CUTOUTS]) and not bits_equal(got[LW.ALL], got[LW.SIGMA_ZERO])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", LW.CAMERAS)
@pytest.mark.parametrize("form", [LDS_FAST, GLOBAL_FAST], ids=["lds", "global"])
def test_an_lds_and_a_global_memory_form_under_all_three_cameras(p, monkeypatch, first_sums, form, kind, mode):
    setenv(monkeypatch, TW.FORMS[form][1])
    tw = LW.run(bool(mode), False, None, True)
    r = renderer(p, tw, kind, form, mode)
    against_the_twin(r, tw, kind, LW.ALL, first_sums, (mode, form[0]))
    r.close()


# ---- 2. sessions and ranks -----------------------------------------------------------------------------------------------------------------------------------
def test_uneven_refinement_steps_are_the_twins_first_sample_frames(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    tw = LW.run(False, False, None, True)
    for kind in ("motion", "defocus"):
        head, ok_head = tw.samples(kind, spp=3)
        tail, ok_tail = tw.samples(kind, spp=5, first_sample=3)
        assert ok_head.all() and ok_tail.all()
        both = np.concatenate([head, tail], axis=2)
        assert bits_equal(both, tw.frame(LW.ALL, kind).samples)
        r = renderer(p, tw, kind)
        r.refine(3)
        first = r.refine_sums()
        assert bits_equal(first, IT.in_order_sums(head)), mismatch_report(first, IT.in_order_sums(head))
        r.refine(5)
        stepped = r.refine_sums()
        r.close()
        assert bits_equal(stepped, IT.in_order_sums(both)), mismatch_report(stepped, IT.in_order_sums(both))


def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    tw = LW.run(False, False, None, True)
    f = tw.frame(LW.ALL, "defocus")
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, tw.cams["defocus"], tw.scene.getWorldPtr(), 2, seed=SEED)
    assert m.cutouts_info() == {"enabled": True, "records": CUT_RECORDS} and m.microfacets_info() == {"enabled": True, "records": MFAC_RECORDS}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.close()
    assert f.followed.all() and bits_equal(frame, f.frame), mismatch_report(frame, f.frame)


# ---- 3. masks that decide nothing, and a mask that decides everything: GPU against GPU ------------------------------------------------------------------------
def test_an_opaque_mask_on_every_material_changes_no_bit_under_the_motion_camera_with_media(p, monkeypatch):
    import _cutout_worlds as CW
    setenv(monkeypatch, TW.LDS)
    tw = LW.run(False, False, None, True)
    r = renderer(p, tw, "motion")
    r.cutouts(None)
    bare = sums_of(r)
    table = CW.all_of(p, tw.scene, tw.scene.names["images"]["white"])
    table[np.nonzero(tw.table[2]["on"])[0]] = (0, 0, 0.0, 0)   # a material with an interior record takes no cutout: a holed solid has no inside
    r.cutouts(table)
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": int((table["on"] != 0).sum())} and (table["on"] != 0).sum() > CUT_RECORDS
    opaque = sums_of(r)
    r.close()
    assert bits_equal(opaque, bare), mismatch_report(opaque, bare)
    assert bits_equal(bare, tw.frame(LW.NO_CUTOUTS, "motion").sums)


def test_a_black_mask_on_the_leaf_is_the_room_built_without_it(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    tw = LW.run(False, False, None, True)
    frames = []
    for args in (dict(leaf_mask="black"), dict(leaf=False)):
        scene = LW.room(p, masks=True, **args)
        r = renderer(p, tw, "motion", scene=scene)
        frames.append(sums_of(r))
        r.close()
    assert bits_equal(frames[0], frames[1]), mismatch_report(frames[0], frames[1])
    assert not bits_equal(frames[0], tw.frame(LW.ALL, "motion").sums)


# ---- 4. mode RT_AOV_FULL in the room ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LW.CAMERAS)
@pytest.mark.parametrize("form", [LDS_FAST, GLOBAL_FAST, LIST_LDS, LIST_GLOBAL], ids=["stack-lds", "stack-global", "list-lds", "list-global"])
def test_the_full_feature_pass_is_the_feature_twin_in_the_live_room(p, monkeypatch, form, kind):
    """aov_kernel_full beside the CUT kernel, in the plain room with its media, moving spheres, vertex normals, live normal-map table and masks: the feature sums
    equal the extended feature twin (whose walk starts each sample's stream where the camera's draws left it) on every pixel, the colour sums beside them equal
    the colour twin; the first-hit features read neither the interior nor the microfacet table; the normal-map table moves the normal sums and nothing else."""
    setenv(monkeypatch, TW.FORMS[form][1])
    as_list = form[0] == TW.LIST
    tw = LW.run(False, as_list, None, True)
    r = renderer(p, tw, kind, form)
    r.enable_aov(full=True)
    assert r.aov_mode() == "full" and r.kernel_cutout()
    r.refine(SPP)
    aov, sums = r.aov_sums(), r.refine_sums()
    want = LW.features(as_list, kind)
    assert bits_equal(aov, want), (kind, mismatch_report(aov, want))
    f = tw.frame(LW.ALL, kind)
    assert f.followed.all() and bits_equal(sums, f.sums), mismatch_report(sums, f.sums)
    if kind == "pinhole" and form == LDS_FAST:   # the filter on these buffers
        import test_gpu_denoise as DN
        dp = p.Renderer.denoise_params()
        got = r.denoise()
        want_frame = DN.twin_denoise(sums, aov, SPP, SPP, dp.iterations, dp.sigma_depth, dp.sigma_lum, dp.demodulate)
        assert bits_equal(got, want_frame), mismatch_report(got, want_frame)
    r.interiors(None)
    r.refine(SPP)
    no_interiors = r.aov_sums()
    r.microfacets(None)
    r.refine(SPP)
    no_records = r.aov_sums()
    assert bits_equal(aov, no_interiors) and bits_equal(aov, no_records), mismatch_report(aov, no_records)
    r.normal_maps(None)
    r.refine(SPP)
    flat = r.aov_sums()
    r.close()
    want_flat = LW.features(as_list, kind, LW.NMAPS_OFF)
    assert bits_equal(flat, want_flat), mismatch_report(flat, want_flat)
    assert bits_equal(flat[..., 3:], aov[..., 3:]) and not bits_equal(flat[..., :3], aov[..., :3])


# ---- 5. random worlds ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fuzz_campaign_runs_five_live_worlds_under_masks_and_the_twin_follows_every_sample(p):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_campaign.py"), "--seeds", "5", "--cutouts", "--live", "--aov-full"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    done = [line for line in res.stdout.splitlines() if line.startswith("DONE: 5 worlds, 0 failures")]
    assert done and "'live_cutout_worlds': 5" in done[0] and "'live_cutout_kernels':" in done[0] and "'live_cutout_not_followed': 0" in done[0], res.stdout[-2000:]
    print(done[0])
