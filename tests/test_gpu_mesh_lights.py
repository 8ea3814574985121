"""Triangle and mesh lights in light sampling on the GPU (mode 4): the 16 TRI && NEE instantiations, given a table that holds a triangle light,
against the numpy twin of a whole sample (tests/_mesh_light_twin.py, pinned by tests/test_mesh_lights_cpu.py), bit for bit — every key of _tri_worlds.FORMS on a
room with a quad, a sphere and a triangle light; a closed emissive mesh; the table at its limit; the clamped index; that modes 0, 1 and 2 are what they were;
what switching does; two ranks; the feature buffers; and the expectation against plain path tracing."""
import ctypes as C

import numpy as np
import pytest

import _mesh_light_twin as MT
import _mesh_light_worlds as MW
import _tri_twin as TT
import _tri_worlds as TW
from _common import as_oracle_camera, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu

ENV_KEYS = ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP")


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read when the renderer is made


def make(p, run, mode=4, variant=0):
    r = p.Renderer.MakeRenderer(run.W, run.H, run.spp, run.depth, run.cam, run.scene.getWorldPtr(), seed=run.seed, variant=variant)
    if mode:
        r.light_sampling(mode)
    return r


def test_mode_4_is_accepted_on_a_triangle_lit_room_and_reported(p, monkeypatch):
    """fails without the feature: enable(4) is RT_ERR_INVALID there, and modes 1 and 2 refuse this world for having no light of theirs"""
    set_env(monkeypatch, {})
    run = MW.run("triangle_lit")
    r = make(p, run, mode=0)
    assert r.light_sampling_mode() == 0 and r.light_sampling_info() == {"enabled": False, "lights": 0}
    with pytest.raises(p.capi.RtError, match="no quad light"):
        r.light_sampling(1)
    with pytest.raises(p.capi.RtError, match="no light to sample"):
        r.light_sampling(2)
    r.light_sampling(4)
    out = (C.c_uint32 * 2)()
    assert p.lib().rt_renderer_light_sampling_info(r.h, out) == 0 and list(out) == [4, 1]
    assert r.light_sampling_mode() == 4 and r.light_sampling_info() == {"enabled": True, "lights": 1}
    assert r.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 1, 0, 0), nee=1) and r.kernel_triangles()   # an existing instantiation
    for bad in (3, 5, 8):
        with pytest.raises(p.capi.RtError, match="on must be 0 \\(off\\), 1 "):
            r.light_sampling(bad)
    with pytest.raises(p.capi.RtError, match="must be 0"):
        r.light_sampling(3)
    assert r.light_sampling_mode() == 4
    r.refine(run.spp)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling("off")
    assert r.light_sampling_mode() == 0
    r.light_sampling("mesh")
    assert r.light_sampling_mode() == 4
    r.close()


def test_switching_2_4_2_restarts_the_refinement_and_4_4_does_not(p, monkeypatch):
    set_env(monkeypatch, {})
    run = MW.run("three_kinds")
    r = make(p, run, mode=2)
    assert r.light_sampling_info() == {"enabled": True, "lights": 2}
    r.refine(3)
    r.light_sampling(4)                       # 2 -> 4: another table, another sequence
    assert r.refine_info()["samples"] == 0 and r.light_sampling_info() == {"enabled": True, "lights": 3}
    r.refine(3)
    r.light_sampling(4)                       # 4 -> 4 keeps it
    r.light_sampling("mesh")
    assert r.refine_info()["samples"] == 3
    r.refine(1)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling(2)                       # 4 -> 2 discards, and mode 2's table is still its own
    assert r.refine_info()["samples"] == 0 and r.light_sampling_info() == {"enabled": True, "lights": 2}
    r.refine(run.spp)
    two = TW.run(mode=2, lamp=True, tri_light=True)
    assert bits_equal(r.refine_sums(), two.sums), mismatch_report(r.refine_sums(), two.sums)
    r.close()


@pytest.fixture(scope="module")
def first_of_world():
    """world name -> (form, sums, frame) of the first form rendered on it: what every later form of that world must repeat on EVERY pixel"""
    return {}


@pytest.mark.parametrize("form", list(TW.FORMS), ids=[TW.form_id(f) for f in TW.FORMS])
def test_every_triangle_instantiation_samples_a_triangle_light_as_the_twin_does(p, monkeypatch, first_of_world, form):
    """All 16 RT_KERNEL_TRI_NEE keys, each reached by its recipe of _tri_worlds.FORMS on the room with a quad light, a sphere lamp and a triangle light, and
    identified through kernel_form() and kernel_triangles(): frame and refinement sums against the twin, two passes, uneven steps.  An EXT = 2 room holds an
    image-textured triangle: the twin follows every other pixel, and on the rest every form of the room gives the bits of the first one rendered."""
    world, exact, ext, big, wide = form
    variant, env = TW.FORMS[form]
    name = "three_kinds" + ("_textured" if ext == 2 else "") + ("_list" if world == TW.LIST else "")
    run = MW.run(name)
    keep = run.pixel_followed
    assert run.followed if ext == 1 else 0.8 < keep.mean() < 1.0
    set_env(monkeypatch, env)
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # a cut inside the frame: two passes
    r = make(p, run, variant=variant)
    assert r.light_sampling_info() == {"enabled": True, "lights": 3} and r.light_sampling_mode() == 4
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1) and r.kernel_triangles()
    r.Render()
    img = r.DownloadRenderbuffer()
    assert bits_equal(img[keep], run.frame[keep]), mismatch_report(img[keep], run.frame[keep])
    r.refine(1)
    r.refine(3)   # uneven steps
    sums = r.refine_sums()
    r.close()
    assert bits_equal(sums[keep], run.sums[keep]), mismatch_report(sums[keep], run.sums[keep])
    assert np.isfinite(sums[keep]).all()
    if ext == 2:   # the list and the tree of one room see the same hits (tests/test_triangles_cpu.py), exact and fast division the same quotients' decisions
        first_id, first_sums, first_img = first_of_world.setdefault(name, (TW.form_id(form), sums, img))
        assert bits_equal(sums, first_sums) and bits_equal(img, first_img), f"against {first_id}: " + mismatch_report(sums, first_sums)


@pytest.mark.parametrize("big", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("name", MW.EDGE_WORLDS)
def test_the_remaining_worlds_are_the_twin_bit_for_bit(p, monkeypatch, name, big):
    """three kinds in one table; a closed emissive icosphere(0) and a tetrahedron (both crossings contribute); 64 triangle lights of different areas; one light
    (no index draw); and 64 lights under the seed whose index draw is the uniform 1 (tests/test_mesh_lights_cpu.py holds each world to what it is there for)"""
    run = MW.run(name)
    assert run.followed
    if name == "mesh_lamp":
        assert run.lights == 20 and run.stats["two_tri_crossings"] > 0   # both crossings of the closed mesh are reached
    if name == "clamped_triangle_index":
        assert run.stats["index_clamped"] > 0
    set_env(monkeypatch, TW.NARROW if big else TW.LDS)
    r = make(p, run)
    assert r.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 1, big, 0), nee=1) and r.kernel_triangles()
    assert r.light_sampling_info() == {"enabled": True, "lights": run.lights}
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.refine(run.spp)
    sums = r.refine_sums()
    r.close()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(frame, run.frame) and np.isfinite(sums).all() and (sums[..., :3] > 0).any(axis=2).mean() > 0.5


def test_sixty_five_lights_are_refused(p, monkeypatch):
    set_env(monkeypatch, {})
    s = MW.scene("sixty_five")
    r = p.Renderer.MakeRenderer(32, 32, 1, 4, TW.camera(p), s.getWorldPtr(), seed=MW.SEED)
    with pytest.raises(p.capi.RtError, match="more than 64 lights"):
        r.light_sampling(4)
    assert r.light_sampling_mode() == 0
    r.Render()   # a refused enable leaves the renderer as it was
    r.close()


def test_without_a_triangle_light_mode_4_is_mode_2_bit_for_bit(p, monkeypatch):
    set_env(monkeypatch, {})
    run = MW.run("plain_lamp")
    frames = {}
    for mode in (2, 4):
        r = make(p, run, mode=mode)
        assert r.light_sampling_info() == {"enabled": True, "lights": 2} and r.kernel_triangles()
        r.Render()
        frame = r.DownloadRenderbuffer()
        r.refine(run.spp)
        frames[mode] = (frame, r.refine_sums())
        r.close()
    assert bits_equal(frames[4][0], frames[2][0]) and bits_equal(frames[4][1], frames[2][1])
    assert bits_equal(frames[4][1], run.sums) and bits_equal(run.sums, TW.run(mode=2, lamp=True).sums)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_modes_0_1_2_on_a_triangle_lit_world_are_what_tri_twin_says(p, monkeypatch, mode):
    set_env(monkeypatch, {})
    old = TW.run(mode=mode, lamp=True, tri_light=True)
    run = MW.run("three_kinds")
    r = make(p, run, mode=4)     # through mode 4 and back: its table changes nothing of the others
    r.refine(1)
    r.light_sampling(mode)
    assert r.light_sampling_info()["lights"] == (mode or 1) and r.refine_info()["samples"] == 0
    r.refine(run.spp)
    assert bits_equal(r.refine_sums(), old.sums), mismatch_report(r.refine_sums(), old.sums)
    r.close()


def test_two_ranks_in_mode_4_render_the_single_renderers_frame(p, monkeypatch):
    set_env(monkeypatch, {})
    run = MW.run("mesh_lamp")
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    m = p.MultiRenderer.MakeRenderer(run.W, run.H, run.spp, run.depth, run.cam, run.scene.getWorldPtr(), 2, seed=run.seed)
    with pytest.raises(p.capi.RtError, match="must be 0"):
        m.light_sampling(3)
    m.light_sampling("mesh")
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), run.frame), mismatch_report(m.DownloadRenderbuffer(), run.frame)
    m.refine(run.spp)
    assert bits_equal(m.DownloadRenderbuffer(), run.frame)
    m.close()
    r = make(p, run)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), run.frame)
    r.close()


def test_feature_buffers_are_unchanged_by_the_mode(p, monkeypatch):
    set_env(monkeypatch, {})
    run = MW.run("three_kinds")
    exp = TT.first_hit_sums(run.world, as_oracle_camera(run.cam), run.W, run.H, run.spp, run.seed)
    got = {}
    for mode in (0, 4):
        r = make(p, run, mode=mode)
        r.enable_aov()
        r.refine(1)
        r.refine(run.spp - 1)
        got[mode] = r.aov_sums()
        r.close()
    assert bits_equal(got[4], got[0]), mismatch_report(got[4], got[0])
    assert bits_equal(got[4][..., 0:4], exp[..., 0:4]) and bits_equal(got[4][..., 7], exp[..., 4])


def test_mode_4_and_plain_path_tracing_agree_in_expectation_on_the_tetrahedron_lamp(p, monkeypatch):
    """16 seeds x 256 spp per mode, 32 x 32, depth 8: the frame-mean radiance per channel of mode 0 and of mode 4 differ by at most 5 sqrt(SE0^2 + SE4^2), the
    standard errors taken from the spread over the 16 seeds.  The lamp (a tetrahedron of scale 1.2 under the ceiling) is large enough for plain path tracing to
    know the mean to a fraction of a percent, so a density wrong by a factor of 2 — which moves the light half's share of the mean by tens of percent — would
    exceed the bound many times over.  Measured on one MI355X (EXPERIMENTS.md E10): MEASURED below."""
    set_env(monkeypatch, {})
    scene = MW.scene("tetrahedron_lamp")
    cam = TW.camera(p)
    means = {0: [], 4: []}
    for mode in (0, 4):
        for seed in range(16):
            r = p.Renderer.MakeRenderer(32, 32, 256, 8, cam, scene.getWorldPtr(), seed=1000 + seed)
            if mode:
                r.light_sampling(mode)
            r.refine(256)   # the linear sums: the framebuffer is clamped and square-rooted, and its mean is not the mean radiance
            means[mode].append(r.refine_sums()[..., :3].astype(np.float64).mean(axis=(0, 1)) / 256.0)
            r.close()
    m0, m4 = np.mean(means[0], axis=0), np.mean(means[4], axis=0)
    se0, se4 = np.std(means[0], axis=0, ddof=1) / 4.0, np.std(means[4], axis=0, ddof=1) / 4.0
    bound = 5 * np.sqrt(se0 ** 2 + se4 ** 2)
    print(f"tetrahedron_lamp 16 x 256 spp: mode 0 mean {m0} se {se0}; mode 4 mean {m4} se {se4}; |diff| / bound {np.abs(m0 - m4) / bound}")
    assert (se0 < 0.01 * m0).all()   # plain path tracing knows the mean well: the check is sharp
    assert (np.abs(m0 - m4) <= bound).all()


MEASURED = """one MI355X, seeds 1000..1015, frame-mean radiance (R, G, B) from the linear refinement sums:
mode 0: mean 0.49246666 0.38121569 0.28627472, SE 0.00051968 0.00032543 0.00025991 (0.1 % of the mean)
mode 4: mean 0.49298981 0.38121029 0.28633416, SE 0.00025961 0.00020879 0.00016122
|difference| / (5 sqrt(SE0^2 + SE4^2)): 0.180 0.003 0.039"""
