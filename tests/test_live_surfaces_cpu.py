"""The room of the live-surface tests without a GPU: the extended twin follows EVERY sample of it under the three cameras, plain and under mode 48;
the paths take the combinations the room was built for (counted and printed); the frame is sensitive to the records, the camera, the time and the order of a
medium's draw; and the host's rule functions give what the twin computed on 256 hits of each rule taken from the room's paths."""
import numpy as np
import pytest

import _interior_twin as IT
import _live_worlds as LW
import _nmap_twin as NT
import _nmap_worlds as NW
import _rglass_twin as GT
from _common import bits_equal, mismatch_report, pkg
from test_surfaces_cpu import Recorder, WithoutTable, gathered

F = np.float32
MODES = [False, True]
MODE_IDS = ["plain", "mode48"]


@pytest.fixture(scope="module")
def p():
    return pkg()


def pixels_that_differ(a, b):
    """the number of pixels on which two frames of samples differ in any bit"""
    a, b = np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32)
    return int((a != b).any(axis=(2, 3)).sum())


@pytest.mark.parametrize("kind", LW.CAMERAS)
@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_every_sample_is_followed_and_the_paths_take_what_the_room_was_built_for(mode48, kind):
    """No sample is excused: followed.all() under every table variant the GPU test renders.  The counters: a recorded hit on a noise material; a mapped-normal hit
    on a moving sphere at a time above 0.25 (the motion camera's alone: the other two trace at time 0); a records' rule run on a path that had drawn for a medium;
    a medium scatter inside the frosted ball right after a rough transmission; a charged interior hit; an inside segment that ended on the medium, which the rule
    leaves uncharged.  Mode 48 refuses a world with a medium, so its room has none: there the light halves are counted in the medium counters' place."""
    tw = LW.run(mode48)
    for variant in LW.VARIANTS:
        assert tw.frame(variant, kind).followed.all(), variant
    stats = tw.frame(LW.ALL, kind).stats
    names = LW.COUNTERS_48 if mode48 else LW.COUNTERS
    counts = {name: int(np.sum(stats.get(name, 0))) for name in names}
    print(f"live room {'mode 48' if mode48 else 'plain'} {kind}: {counts}")
    for name in names:
        if name == "mapped_moving" and kind != "motion":
            assert counts[name] == 0
        else:
            assert counts[name] > 0, name
    assert (stats.get("medium_draws", 0) > 0) == (not mode48)


@pytest.mark.parametrize("mode48", MODES, ids=MODE_IDS)
def test_the_room_is_sensitive_to_records_camera_and_time(mode48):
    tw = LW.run(mode48)
    out = {}
    for kind in LW.CAMERAS:
        out[f"records off, {kind}"] = pixels_that_differ(tw.frame(LW.ALL, kind).samples, tw.frame(LW.RECORDS_OFF, kind).samples)
    for a, b in (("pinhole", "defocus"), ("pinhole", "motion"), ("defocus", "motion")):
        out[f"cameras swapped, {a} / {b}"] = pixels_that_differ(tw.frame(LW.ALL, a).samples, tw.frame(LW.ALL, b).samples)
    still, ok = tw.samples("motion", time0=True)
    assert ok.all()
    out["time zeroed, motion"] = pixels_that_differ(tw.frame(LW.ALL, "motion").samples, still)
    print(f"live room {'mode 48' if mode48 else 'plain'}, pixels of {LW.W * LW.H} that differ: {out}")
    assert all(v >= 1 for v in out.values()), out


def draw_for_the_accepted_test_alone(tape, rows, accepted):
    """The deliberately WRONG order this work is about: a medium test that finds a non-empty interval but does not accept gives its uniform back, so that only an
    accepted test has drawn.  The kernels and the oracle draw once per non-empty interval, whatever becomes of the test."""
    tape.cur[rows[~accepted]] -= 1


@pytest.mark.parametrize("kind", LW.CAMERAS)
def test_a_twin_that_draws_for_the_accepted_medium_test_alone_gives_another_frame(kind):
    tw = LW.run(False)
    right = tw.frame(LW.ALL, kind)
    stats = {"after_medium": draw_for_the_accepted_test_alone}
    wrong, ok = tw.samples(kind, stats=stats)
    n = pixels_that_differ(right.samples, wrong)
    print(f"live room plain {kind}: the wrong draw order changes {n} of {LW.W * LW.H} pixels ({stats['medium_draws'] - stats['medium_hits']} uniforms given back)")
    assert ok.all() and n >= 1


def test_the_host_rules_give_what_the_twin_computed_on_256_hits_of_each_rule(p, monkeypatch):
    """The twin's run of the room under the motion camera with its rule functions recorded; 256 of the hits of each rule go to rt_normal_map_batch,
    rt_microfacet_batch, rt_rough_glass_batch and rt_interior_batch, the functions the kernels share, and come back as the twin had them, bit for bit."""
    nmap, mfac, glass, solid = Recorder(NT.case), Recorder(GT.mfac_scatter, 5), Recorder(GT.faced, 4), Recorder(IT.interior_hit)
    monkeypatch.setattr(NT, "case", nmap)
    monkeypatch.setattr(GT, "mfac_scatter", mfac)
    monkeypatch.setattr(GT, "faced", glass)
    monkeypatch.setattr(IT, "interior_hit", solid)
    tw = LW.run(False)
    fresh, _ = tw.samples("motion")
    monkeypatch.undo()
    assert bits_equal(fresh, tw.frame(LW.ALL, "motion").samples)
    table = NW.api_table(tw.textures)

    (surface, a, b, tri, normal, ray_d, u, v, index, strength), (want_n, want_path), _, n = gathered(WithoutTable(nmap), 10, 2, cover=1)
    got_n, got_path = p.api.normal_map_batch(table, surface, a, b, tri, normal, ray_d, u, v, index, strength)
    assert bits_equal(got_n, want_n) and (got_path == want_path).all(), mismatch_report(got_n, want_n)
    assert (surface == NT.SPHERE).all() and n >= 256
    print(f"host rules on the live room: normal map {n} hits", end="")

    (normal, ray_d, rough, f0, coat), (want_w, want_f, want_way), words, n = gathered(mfac, 5, 3, cover=2)
    got = p.api.microfacet_batch(normal, ray_d, rough, f0, coat.astype(np.uint32), words)
    assert bits_equal(got[0], want_w) and bits_equal(got[1], want_f) and (got[2] == want_way).all(), mismatch_report(got[0], want_w)
    assert (got[3] == [len(k) for k in words]).all() and coat.any() and not coat.all() and n >= 256
    print(f", microfacet {n}", end="")

    (facing, eta, ray_d, rough), (want_w, want_g, want_way), words, n = gathered(glass, 4, 3, cover=2)
    behind = eta == F(1.5)                       # the frosted ball's index: 1.5 from inside, 1 / 1.5 from outside
    assert (behind | (eta == F(1) / F(1.5))).all() and behind.any() and not behind.all()
    got = p.api.rough_glass_batch(np.where(behind[:, None], -facing, facing), ray_d, rough, np.full(len(eta), 1.5, F), words)
    assert bits_equal(got[0], want_w) and bits_equal(got[1], want_g) and (got[2] == want_way).all(), mismatch_report(got[0], want_w)
    assert (got[3] == [len(k) for k in words]).all() and n >= 256
    print(f", rough glass {n}", end="")

    (back, ray_d, t, ior, sigma), (want_eta, want_T), _, n = gathered(solid, 5, 2)
    back = back.astype(bool)
    stored = np.where(back[:, None], ray_d, -ray_d).astype(F)   # a stored normal on the side of the ray the twin's facing says: the batch takes its own decision from it
    got_back, got_eta, got_T = p.api.interior_batch(stored, stored, ray_d, t, ior, sigma, np.zeros(len(t), np.uint32))
    assert (got_back.astype(bool) == back).all() and bits_equal(got_eta, want_eta) and bits_equal(got_T, want_T), mismatch_report(got_T, want_T)
    assert back.any() and not back.all() and (sigma[back] > 0).any() and n >= 256
    print(f", interior {n}")


def test_the_light_table_of_mode_48_refuses_the_room_with_its_media(p):
    """Why the room under mode 48 has no medium: mode 48's table is mode 16's, and the host refuses to build it for a world with a constant medium — whose hit test
    draws from the path's stream — so no kernel ever picks a light half after a medium's draw.  The room without its media is accepted."""
    with pytest.raises(p.capi.RtError, match="RT_MAT_ISOTROPIC") as e:
        LW.room(p, env=True, medium=True).light_tree()
    assert e.value.code == 1
    nodes, cdf = LW.run(True).scene.light_tree()
    assert len(cdf) >= 1
