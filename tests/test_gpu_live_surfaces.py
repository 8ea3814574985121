"""Live surface records beside media, noise, moving spheres and the three cameras, on the GPU: all sixteen INTR, sixteen MFAC and sixteen NMAP
instantiations of render_kernel_stream render the room of tests/_live_worlds.py with every record live and are compared with the extended whole-sample twin
(tests/_path_twin.py with `media`; pinned to the CPU oracle by tests/test_path_twin_oracle_cpu.py), which follows EVERY sample: in-order refinement sums and frames,
bit for bit on every pixel.  Frames are 24 x 16 at 8 spp and depth 8.  Mode 48 refuses a world with a constant medium, so its room has none."""
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
LDS_FAST, GLOBAL_FAST = (TW.BVH, 0, 2, 0, 0), (TW.BVH, 0, 2, 1, 0)


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


def renderer(p, tw, kind, form=LDS_FAST, mode=0, spp=SPP):
    """a renderer of the room on the recipe of `form` (the caller has set its environment), under camera `kind`, that states the INTR kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, tw.cams[kind], tw.scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_interior() and r.kernel_microfacet() and not r.kernel_normal_map() and r.normal_maps_info()["enabled"]   # a family's query names its own key
    assert r.interiors_info() == {"enabled": True, "records": 1} and r.microfacets_info() == {"enabled": True, "records": 4}
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
    assert r.kernel_env_light() == (mode == 48) and r.kernel_light_tree() == (mode == 48)
    return r


def sums_of(r, spp=SPP):
    r.refine(spp)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    assert bits_equal(frame, IT.resolve(sums, spp))
    return sums


def push(r, table):
    nmaps, mfacs, interiors = table
    r.normal_maps(nmaps)
    r.microfacets(mfacs)
    r.interiors(interiors)


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


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_of_the_three_families_is_the_twin(p, monkeypatch, first_sums, form, mode):
    """One shape of kernel, plain or under mode 48, under the camera its index picks: the INTR key with every table on; the same kernel with every sigma zero (the
    facing alone) and with every record off, the three tables still present; the MFAC key with the interior table taken away; the NMAP key with the microfacet
    table taken away too.  Forty-eight instantiations in all, each equal to the twin on every pixel and to the other forms of its world and camera."""
    setenv(monkeypatch, TW.FORMS[form][1])
    kind = LW.CAMERAS[FORMS.index(form) % 3]
    tw = LW.run(bool(mode), form[0] == TW.LIST)
    key = (mode, form[0])
    r = renderer(p, tw, kind, form, mode)
    full = against_the_twin(r, tw, kind, LW.ALL, first_sums, key)
    facing = against_the_twin(r, tw, kind, LW.SIGMA_ZERO, first_sums, key)
    assert r.kernel_interior() and not bits_equal(facing, full)
    off = against_the_twin(r, tw, kind, LW.RECORDS_OFF, first_sums, key)
    assert r.kernel_interior() and r.kernel_microfacet() and r.normal_maps_info()["enabled"] and r.interiors_info() == {"enabled": True, "records": 0}
    assert not bits_equal(off, full)
    mfac = against_the_twin(r, tw, kind, LW.NO_INTERIORS, first_sums, key)
    assert not r.kernel_interior() and r.kernel_microfacet() and not r.kernel_normal_map() and r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0)
    nmap = against_the_twin(r, tw, kind, LW.NO_MICROFACETS, first_sums, key)
    assert not r.kernel_interior() and not r.kernel_microfacet() and r.kernel_normal_map() and r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0)
    r.close()
    assert not bits_equal(mfac, full) and not bits_equal(nmap, mfac)


@pytest.mark.parametrize("mode", MODES, ids=["plain", "mode48"])
@pytest.mark.parametrize("kind", LW.CAMERAS)
@pytest.mark.parametrize("form", [LDS_FAST, GLOBAL_FAST], ids=["lds", "global"])
def test_an_lds_and_a_global_memory_form_under_all_three_cameras(p, monkeypatch, first_sums, form, kind, mode):
    setenv(monkeypatch, TW.FORMS[form][1])
    tw = LW.run(bool(mode))
    r = renderer(p, tw, kind, form, mode)
    against_the_twin(r, tw, kind, LW.ALL, first_sums, (mode, form[0]))
    r.close()


def test_uneven_refinement_steps_are_the_twins_first_sample_frames(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    tw = LW.run(False)
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
    tw = LW.run(False)
    f = tw.frame(LW.ALL, "motion")
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, tw.cams["motion"], tw.scene.getWorldPtr(), 2, seed=SEED)
    assert m.microfacets_info() == {"enabled": True, "records": 4}
    m.Render()
    frame = m.DownloadRenderbuffer()
    m.close()
    assert f.followed.all() and bits_equal(frame, f.frame), mismatch_report(frame, f.frame)


def test_the_feature_pass_refuses_the_medium_and_runs_on_the_room_without_it(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    tw = LW.run(False)
    r = renderer(p, tw, "pinhole")
    form = r.kernel_form()
    for textured in (False, True):   # both modes refuse the room: the plain one its normal-map table before anything else, the textured one its medium
        with pytest.raises(p.capi.RtError, match="RT_MAT_ISOTROPIC" if textured else "normal-map table") as e:
            r.enable_aov(textured=textured)
        assert e.value.code == 1 and r.kernel_form() == form and r.kernel_interior() and r.kernel_microfacet() and r.normal_maps_info()["enabled"]
        assert r.interiors_info() == {"enabled": True, "records": 1} and r.microfacets_info() == {"enabled": True, "records": 4}
    sums = sums_of(r)   # ... and the renderer is as usable as it was
    assert bits_equal(sums, tw.frame(LW.ALL, "pinhole").sums)
    r.enable_aov(full=True)   # the third mode follows the medium: it admits the room as it is, and gives the feature twin's sums
    assert r.aov_mode() == "full" and r.kernel_form() == form and r.kernel_interior() and r.kernel_microfacet() and r.normal_maps_info()["enabled"]
    r.refine(SPP)
    full, sums = r.aov_sums(), r.refine_sums()
    r.close()
    want = LW.feature_sums(tw, "pinhole")
    assert bits_equal(full, want), mismatch_report(full, want)
    assert bits_equal(sums, tw.frame(LW.ALL, "pinhole").sums)
    dry = LW.run(False, medium=False)
    r = renderer(p, dry, "pinhole")
    with pytest.raises(p.capi.RtError, match="normal-map table") as e:   # the plain mode refuses the room, medium or none: the textured mode is the one it admits
        r.enable_aov(textured=False)
    assert e.value.code == 1 and r.kernel_interior()
    r.enable_aov(textured=True)
    r.refine(SPP)
    on, sums = r.aov_sums(), r.refine_sums()
    assert bits_equal(sums, dry.frame(LW.ALL, "pinhole").sums)   # the beauty frame beside the features is the twin's
    r.interiors(None)
    r.refine(SPP)
    no_interiors = r.aov_sums()
    r.microfacets(None)
    r.refine(SPP)
    no_records = r.aov_sums()
    r.close()
    assert bits_equal(on, no_interiors) and bits_equal(on, no_records), mismatch_report(on, no_records)   # first-hit features read neither table


def test_the_fuzz_campaign_runs_ten_live_worlds_and_the_twin_follows_every_sample(p):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_campaign.py"), "--seeds", "10", "--surfaces", "--live"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    done = [line for line in res.stdout.splitlines() if line.startswith("DONE: 10 worlds, 0 failures")]
    assert done and "'live_worlds': 10" in done[0] and "'live_kernels':" in done[0] and "'live_not_followed': 0" in done[0], res.stdout[-2000:]
    print(done[0])
