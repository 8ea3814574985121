"""The masked live room without a GPU: without records it is the CPU oracle's; the composed walk — the cutout rule in the leaf phase, then smooth
normal and normal map at the hit the walk kept — with no rule to apply is the walk; an empty mask is the surface removed; the twin follows EVERY sample and the
paths take what the room was built for (counted, printed and held to a bar); three deliberately wrong twins each give another frame; the host's rule function gives
what the twin computed on candidates taken from the room's paths; the feature twin of mode RT_AOV_FULL knows the normal map and the cameras' draws; and the twin's
frames are the digests of profiles/twin_digests_live_cutouts.txt."""
import os

import numpy as np
import pytest

import _aov_full_twin as AF
import _aov_tex_twin as AT
import _cutout_twin as CT
import _cutout_worlds as CW
import _live_worlds as LW
import _nmap_twin as NT
import _nmap_worlds as NW
import _path_twin as PT
import _tex_twin as XT
import _tri_twin as TT
import _uv_twin as UT
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg
from test_live_surfaces_cpu import draw_for_the_accepted_test_alone
from test_path_twin_oracle_cpu import oracle_samples
from test_surfaces_cpu import Recorder

F = np.float32
MODES = [False, True]
MODE_IDS = ["plain", "mode48"]
LISTS = [False, True]
LIST_IDS = ["bvh", "list"]


@pytest.fixture(scope="module")
def p():
    return pkg()


def masked(mode48, as_list=False):
    return LW.run(mode48, as_list, None, True)


def values_that_differ(a, b):
    """the number of pixel values (a pixel's red, green or blue) in which two frames of in-order sums differ in any bit"""
    a, b = np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32)
    return int((a != b)[..., 0:3].sum())


# ---- 1. the room and the walk ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("kind", LW.CAMERAS)
def test_the_masked_room_without_records_is_the_oracles(p, kind, as_list):
    """Every record table absent: the whole-sample twin over _tri_twin's walk equals the CPU oracle bit for bit, every sample followed.  The oracle knows the
    world's one image, clamped and unfiltered, whatever entry a material names — so that is the table this twin run is given."""
    scene = LW.room(p, masks=True, as_list=as_list)
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(LW.camera(p, kind))
    tex = (None, [(AT.world_image(scene.getWorldPtr()), XT.CLAMP, XT.NEAREST)] * len(scene.textures()[0]))
    got, followed = PT.radiance(world, cam, LW.W, LW.H, LW.DEPTH, LW.SEED, *PT.keys(LW.W, LW.H, LW.SPP), TT.closest_intersection, glass=True, media=True, tex=tex)
    want = oracle_samples(world, cam, LW.W, LW.H, LW.SPP, LW.DEPTH, LW.SEED)
    assert followed.all() and bits_equal(got, want), mismatch_report(got, want)


@pytest.mark.parametrize("kind", LW.CAMERAS)
@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_the_composed_walk_with_no_rule_to_apply_is_the_walk(p, mode48, kind):
    """every record off, and an all-white mask on every material that takes one: the samples of _nmap_twin.walk_of without `base`"""
    tw = masked(mode48)
    plain, ok = tw.samples(kind, plain_walk=True)
    assert ok.all() and bits_equal(tw.frame(LW.CUTOUTS_OFF, kind).samples, plain) and bits_equal(tw.frame(LW.NO_CUTOUTS, kind).samples, plain)
    white = CW.all_of(p, tw.scene, tw.scene.names["images"]["white"])
    white[np.nonzero(tw.table[2]["on"])[0]] = (0, 0, 0.0, 0)   # (solid glass takes no cutout)
    stats = {}
    opaque, ok = tw.samples(kind, tw.table[:3] + (white,), stats=stats)
    assert ok.all() and bits_equal(opaque, plain), mismatch_report(opaque, plain)
    assert stats["tested"] > 1000 and stats["rejected"] == 0
    assert not bits_equal(tw.frame(LW.ALL, kind).samples, plain)


@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_a_black_mask_on_the_leaf_is_the_room_without_the_leaf(mode48):
    black, absent = LW.Twin(mode48, masks=True, leaf_mask="black"), LW.Twin(mode48, masks=True, leaf=False)
    for kind in ("motion", "defocus"):
        a, ok_a = black.samples(kind)
        b, ok_b = absent.samples(kind)
        assert ok_a.all() and ok_b.all() and bits_equal(a, b), mismatch_report(a, b)
        assert not bits_equal(a, masked(mode48).frame(LW.ALL, kind).samples)


# ---- 2. counters and conditions --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("kind", LW.CAMERAS)
@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_every_sample_is_followed_and_every_counter_reaches_the_bar(mode48, kind, as_list):
    """No sample is excused, under every table variant the GPU test renders; and every counter that can occur in the frame is at least LW.AT_LEAST in it.  What
    cannot occur is zero: a sphere that has moved without the motion camera, a light pick without mode 48, a medium's draw without a medium — and a medium's
    draw after a rejection in a list, where every sphere is tested before the first parallelogram."""
    tw = masked(mode48, as_list)
    for variant in LW.CUT_VARIANTS:
        assert tw.frame(variant, kind).followed.all(), variant
    stats = tw.frame(LW.ALL, kind).stats
    counts = {name: int(stats.get(name, 0)) for name in LW.CUT_COUNTERS}
    print(f"masked live room {'mode 48' if mode48 else 'plain'} {'list' if as_list else 'bvh'} {kind}: {counts}")
    for name in LW.CUT_COUNTERS:
        if LW.can_occur(name, mode48, kind, as_list=as_list):
            assert counts[name] >= LW.AT_LEAST, (name, counts[name])
        else:
            assert counts[name] == 0, (name, counts[name])
    assert counts["mask_uv_is_shade_uv"] == counts["kept_image_masked"]   # README: a mask from a picture's alpha agrees with its colour texel for texel
    assert counts["kept_mapped_masked"] >= counts["kept_image_masked"] and counts["kept_smooth_masked"] >= counts["kept_image_masked"]
    assert (stats.get("medium_draws", 0) > 0) == (not mode48)


@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_the_masked_checker_behind_the_frosted_ball_is_met_by_deep_rays_alone(mode48, monkeypatch):
    """no ray from the camera reaches the parallelogram behind the ball — the ball hides it —, and the rule still decides on it: on rays that went through the
    rough glass or came from elsewhere in the room"""
    tw = masked(mode48)
    tiles, eye = tw.scene.names["tiles"], np.asarray(tw.eye, F)
    for kind in ("pinhole", "motion"):
        rec = Recorder(CT.keeps)
        monkeypatch.setattr(CT, "keeps", rec)
        tw.samples(kind)
        monkeypatch.undo()
        on_tiles = [(np.asarray(args[7]) == tiles, args[3], out[0]) for args, out, _ in rec.calls]
        candidates = sum(int(m.sum()) for m, _, _ in on_tiles)
        rejected = sum(int((keep[m] == 0).sum()) for m, _, keep in on_tiles)
        from_the_eye = sum(int((m & (o == eye).all(axis=1)).sum()) for m, o, _ in on_tiles)
        print(f"masked live room {'mode 48' if mode48 else 'plain'} {kind}: the checker behind the ball: {candidates} candidates, {rejected} rejected, {from_the_eye} from the eye")
        assert candidates >= LW.AT_LEAST and 0 < rejected < candidates and from_the_eye == 0


# ---- 3. the room would notice ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_three_wrong_twins_each_give_another_frame(mode48):
    """a rejected candidate that is not taken back (its distance stays in the record, so the walk prunes what lies behind the hole); the leaf's mask read at the
    planar coordinates instead of its record's; and — in the plain room, which has media — a medium that draws only for the test that accepts.  Each moves more
    than 100 pixel values of the frame the GPU tests compare kernels with."""
    tw = masked(mode48)
    out = {}
    for kind in LW.CAMERAS:
        right = tw.frame(LW.ALL, kind).sums
        for wrong in (CT.NOT_TAKEN_BACK, CT.MASK_AT_PLANAR):
            samples, _ = tw.samples(kind, wrong=wrong)
            out[kind, wrong] = values_that_differ(right, LW.IT.in_order_sums(np.nan_to_num(samples)))
        if not mode48:
            samples, ok = tw.samples(kind, stats={"after_medium": draw_for_the_accepted_test_alone})
            assert ok.all()
            out[kind, "a medium draws for the accepted test alone"] = values_that_differ(right, LW.IT.in_order_sums(samples))
    print(f"masked live room {'mode 48' if mode48 else 'plain'}, pixel values of {LW.W * LW.H * 3} that a wrong twin moves: {out}")
    assert all(v > 100 for v in out.values()), out


# ---- 4. the host rule --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_rule_gives_what_the_twin_computed_on_256_candidates_of_each_source(p, monkeypatch):
    """The twin's run of the room under the motion camera with _cutout_twin.keeps recorded; 256 of the candidates of each source of coordinates — a parallelogram's
    planar ones, a triangle's record, a triangle's identity record — go to rt_cutout_batch, the function the kernels share, and come back as the twin had them."""
    rec = Recorder(CT.keeps)
    monkeypatch.setattr(CT, "keeps", rec)
    tw = masked(False)
    fresh, _ = tw.samples("motion")
    monkeypatch.undo()
    assert bits_equal(fresh, tw.frame(LW.ALL, "motion").samples)
    given = p.api.texture_table(NW.api_table(tw.textures))
    cases = {"parallelogram": [], "triangle, coordinates": [], "triangle, identity": []}
    for (table, quads, uv, o, d, t, records, material), out, _ in rec.calls:
        if uv is None:
            assert (quads["kind"] == 0).all()
            name, uv = "parallelogram", np.zeros((len(t), 3, 2), F)
        else:
            assert (quads["kind"] == 1).all()
            identity = (np.asarray(uv) == UT.IDENTITY).all(axis=(1, 2))
            for which, name in ((identity, "triangle, identity"), (~identity, "triangle, coordinates")):
                if which.any() and not which.all():
                    cases[name].append((quads[which], np.asarray(uv)[which], o[which], d[which], t[which], material[which], tuple(x[which] for x in out)))
            if identity.any() and not identity.all():
                continue
            name = "triangle, identity" if identity.all() else "triangle, coordinates"
        cases[name].append((quads, np.asarray(uv), o, d, t, material, out))
    counts = {}
    for name, calls in cases.items():
        quads, uv, o, d, t, material = (np.concatenate([c[i] for c in calls]) for i in range(6))
        want = [np.concatenate([c[6][i] for c in calls]) for i in range(3)]
        counts[name] = len(t)
        at = np.sort(np.random.default_rng(36).choice(len(t), 256, replace=False))
        rays = np.ascontiguousarray(np.concatenate([o[at], d[at]], axis=1), F)
        keep, tuv, value = p.api.cutout_batch(given, quads[at], None if name == "parallelogram" else np.ascontiguousarray(uv[at], F), rays, np.ascontiguousarray(t[at], F),
                                              tw.table[3], material[at].astype(np.uint32))
        assert (keep == want[0][at]).all(), name
        assert bits_equal(tuv, want[1][at]) and bits_equal(value, want[2][at]), (name, mismatch_report(value, want[2][at]))
        assert 0 < keep.sum() < 256, name
    print(f"host rule on the masked live room: candidates {counts}")


# ---- 5. the feature twin -----------------------------------------------------------------------------------------------------------------------------------------
def noise_of(world):
    import _noise_twin as NZ
    tab = NZ.tables(world)
    return lambda albedo, scale, pts: NZ.value(tab, np.asarray(albedo, F), F(scale), pts)


@pytest.mark.parametrize("kind", LW.CAMERAS)
def test_the_feature_twin_with_every_map_off_is_the_feature_twin_without_the_argument(kind):
    tw = masked(False)
    off = tw.table[0].copy()
    off["on"] = 0
    args = dict(uv=tw.uv, cutouts=tw.table[3], table=tw.textures, noise=noise_of(tw.world), vn=tw.vn)
    cam = as_oracle_camera(tw.cams[kind])
    before = AF.sums(tw.world, cam, LW.W, LW.H, LW.SPP, LW.SEED, **args)
    after = AF.sums(tw.world, cam, LW.W, LW.H, LW.SPP, LW.SEED, nmaps=off, **args)
    assert bits_equal(after, before) and bits_equal(before, LW.features(False, kind, LW.NMAPS_OFF))
    mapped = LW.features(False, kind)
    assert bits_equal(mapped[..., 3:], before[..., 3:]) and values_that_differ(mapped, before) > 100   # the map moves the normal sums alone


def test_on_the_dry_room_without_masks_it_is_the_textured_modes_twin_with_the_normal_map_rule():
    """no medium and no mask, the pinhole camera: mode 2's twin is mode 1's (_aov_tex_twin.sums over _nmap_twin.walk_of, as tests/test_gpu_normal_maps.py
    composes them), which the GPU suite holds aov_kernel_nmap to"""
    dry = LW.run(False, medium=False)
    cam = as_oracle_camera(dry.cams["pinhole"])
    trace, _ = NT.walk_of(dry.vn, dry.uv, dry.table[0], dry.textures)
    want = AT.sums(dry.world, cam, LW.W, LW.H, LW.SPP, LW.SEED, True, uv=dry.uv, table=dry.textures, noise=noise_of(dry.world), trace=lambda w, rays: trace(w, rays))[0]
    got = LW.feature_sums(dry, "pinhole")
    assert bits_equal(got, want), mismatch_report(got, want)


def test_a_walk_that_starts_from_a_fresh_stream_under_the_defocus_camera_differs_in_the_fog():
    """what `prim_rng` is for: the walk draws where the camera's draws left the sample's stream — behind the jitter and the two lens draws.  A twin whose walk
    starts from a fresh state gives other first hits where a medium drew, and the same everywhere else."""
    tw = masked(False)
    stats = AF.new_stats()
    right = LW.feature_sums(tw, "defocus", stats=stats)
    assert bits_equal(right, LW.features(False, "defocus")) and stats["medium_draws"] >= 100 and stats["fog_hits"] >= LW.AT_LEAST and stats["through_fog"] >= LW.AT_LEAST
    wrong = LW.feature_sums(tw, "defocus", fresh_rng=True)
    moved = (right.view(np.uint32) != wrong.view(np.uint32)).any(axis=2)
    print(f"masked live room, defocus: a fresh stream moves {int(moved.sum())} of {LW.W * LW.H} pixels of the feature sums; {stats['medium_draws']} medium draws")
    assert moved.sum() >= 10
    dry = LW.Twin(False, medium=False, masks=True)   # without media nothing draws in the walk, and where the stream stands decides nothing
    assert bits_equal(LW.feature_sums(dry, "defocus"), LW.feature_sums(dry, "defocus", fresh_rng=True))


# ---- 6. the reference does not move unnoticed ----------------------------------------------------------------------------------------------------------------------
def test_the_twins_frames_are_the_committed_digests():
    with open(os.path.join(ROOT, "profiles", "twin_digests_live_cutouts.txt")) as f:
        committed = f.read().splitlines()
    now = LW.digest_lines()
    assert len(now) == 60 and [line for line in now if line not in committed] == [] and len(committed) == len(now)
