"""Sphere lights in light sampling on the GPU (mode 2): the 16 NEE instantiations, given a table that holds both kinds of light, against
the numpy twin of a whole sample (tests/_nee2_twin.py, pinned by tests/test_light_sampling_spheres_cpu.py), bit for bit — a sphere-lit room, a mixed
room and a world without any quad, in the LDS and the global-memory form, as a BVH under variants 2 and 3 and as a list, cut into refine steps and
passes; the estimator's edges; that mode 1 is what it was; what switching between modes does; two ranks; and the noise figure on the lamp-lit Cornell box."""
import ctypes as C

import numpy as np
import pytest

import _nee2_twin as T2
import _nee2_worlds as NW2
import _nee_twin as T
import _nee_worlds as NW
from _common import as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu

SEED = 1984
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


def make(p, run, mode=2, variant=0, spp=None):
    r = p.Renderer.MakeRenderer(run.W, run.H, spp or run.spp, run.depth, run.cam, run.scene.getWorldPtr(), seed=run.seed, variant=variant)
    if mode:
        r.light_sampling(mode)
    return r


def test_mode_2_is_accepted_on_a_sphere_lit_room_and_reported(p, monkeypatch):
    """fails without the feature: enable(2) is RT_ERR_INVALID there, and mode 1 refuses this world for having no quad light"""
    set_env(monkeypatch, {})
    run = NW2.run("lamp_room")
    r = make(p, run, mode=0)
    assert r.light_sampling_mode() == 0 and r.light_sampling_info() == {"enabled": False, "lights": 0}
    with pytest.raises(p.capi.RtError, match="no quad light"):
        r.light_sampling(True)
    r.light_sampling(2)
    out = (C.c_uint32 * 2)()
    assert p.lib().rt_renderer_light_sampling_info(r.h, out) == 0 and list(out) == [2, 1]
    assert r.light_sampling_mode() == 2 and r.light_sampling_info() == {"enabled": True, "lights": 1}
    assert r.kernel_form() == NW.kernel_form_of((NW.BVH, 0, 1, 0, 0))   # the same instantiation as mode 1, nee = 1
    with pytest.raises(p.capi.RtError, match="must be 0"):
        r.light_sampling(3)
    assert r.light_sampling_mode() == 2
    r.light_sampling("off")
    assert r.light_sampling_mode() == 0
    r.close()
    mixed = make(p, NW2.run("mixed_room"), mode="all")
    assert mixed.light_sampling_info() == {"enabled": True, "lights": 2}
    mixed.light_sampling("quads")
    assert mixed.light_sampling_mode() == 1 and mixed.light_sampling_info() == {"enabled": True, "lights": 1}
    mixed.close()


def render_run(p, run, variant, expect_form):
    r = make(p, run, variant=variant)
    assert r.kernel_form() == expect_form, (r.kernel_form(), expect_form)
    assert r.light_sampling_info() == {"enabled": True, "lights": run.lights} and r.light_sampling_mode() == 2
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.refine(run.spp)
    sums = r.refine_sums()
    r.close()
    assert bits_equal(frame, T.resolve(sums, run.spp)), mismatch_report(frame, T.resolve(sums, run.spp))
    return sums, frame


@pytest.mark.parametrize("variant,big", [(3, 0), (3, 1), (2, 0), (2, 1)], ids=["fast-lds", "fast-global", "exact-lds", "exact-global"])
@pytest.mark.parametrize("name", NW2.ROOM_WORLDS)
def test_bvh_rooms_are_the_twin_on_every_pixel(p, monkeypatch, name, variant, big):
    run = NW2.run(name)
    assert run.followed.all()
    set_env(monkeypatch, NW.NARROW if big else NW.LDS)
    sums, frame = render_run(p, run, variant, NW.kernel_form_of((NW.BVH, int(variant == 2), 1, big, 0)))
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(frame, T.resolve(run.sums, run.spp))
    assert np.isfinite(sums).all() and (sums[..., :3] > 0).any(axis=2).mean() > 0.9


@pytest.mark.parametrize("big", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("name", NW2.LIST_WORLDS)
def test_list_rooms_are_the_twin_on_every_pixel(p, monkeypatch, name, big):
    run = NW2.run(name)
    set_env(monkeypatch, NW.NARROW if big else NW.LDS)
    sums, _ = render_run(p, run, 0, NW.kernel_form_of((NW.LIST, 1, 1, big, big)))
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(run.sums, NW2.run(name[:-5]).sums)   # the list and the BVH of one room: the same samples


@pytest.fixture(scope="module")
def first_of_world():
    """world name -> (form, sums, frame) of the first form rendered on it: what every later form of that world must repeat on EVERY pixel"""
    return {}


# (world, exact, ext, big, wide) -> (world name, kernel variant, environment): the EXT = 2 forms, which spill the most, and the 32-bit-reference forms
TEXTURED_FORMS = {
    (NW.BVH, 0, 2, 0, 0): ("textured_mixed_room", 3, NW.LDS),   (NW.BVH, 1, 2, 0, 0): ("textured_mixed_room", 2, NW.LDS),
    (NW.BVH, 0, 2, 1, 0): ("textured_mixed_room", 3, NW.NARROW), (NW.BVH, 1, 2, 1, 0): ("textured_mixed_room", 2, NW.NARROW),
    (NW.BVH, 0, 2, 1, 1): ("textured_mixed_room", 3, NW.WIDE),  (NW.BVH, 1, 2, 1, 1): ("textured_mixed_room", 2, NW.WIDE),
    (NW.LIST, 1, 2, 0, 0): ("textured_mixed_room_list", 0, NW.LDS), (NW.LIST, 1, 2, 1, 1): ("textured_mixed_room_list", 0, NW.NARROW),
    (NW.BVH, 0, 1, 1, 1): ("mixed_room", 3, NW.WIDE),           (NW.BVH, 1, 1, 1, 1): ("mixed_room", 2, NW.WIDE),
}


@pytest.mark.parametrize("form", list(TEXTURED_FORMS), ids=NW.form_id)
def test_ext_2_and_wide_forms_run_a_sphere_light_and_are_the_twin(p, monkeypatch, first_of_world, form):
    """the twin on every pixel it follows; on the pixels behind the noise and image materials, the same bits in every form of the world"""
    name, variant, env = TEXTURED_FORMS[form]
    run = NW2.run(name)
    set_env(monkeypatch, env)
    sums, frame = render_run(p, run, variant, NW.kernel_form_of(form))
    f = run.followed
    assert bits_equal(sums[f], run.sums[f]), mismatch_report(sums[f], run.sums[f])
    assert np.isfinite(sums[f]).all()
    first_id, first_sums, first_frame = first_of_world.setdefault(name, (NW.form_id(form), sums, frame))
    assert bits_equal(sums, first_sums) and bits_equal(frame, first_frame), f"against {first_id}: " + mismatch_report(sums, first_sums)


def test_variants_without_a_light_sampling_form_refuse_mode_2_with_mode_1s_words(p, monkeypatch):
    set_env(monkeypatch, {})
    run = NW2.run("lamp_room")
    r = make(p, run, mode=0, variant=1)
    with pytest.raises(p.capi.RtError, match="variant 1 has no light-sampling form") as e:
        r.light_sampling(2)
    assert e.value.code == 1 and r.light_sampling_mode() == 0
    r.close()
    from _common import config_cameras, config_scene
    plain = config_scene(p, "book1_final")   # a BVH world of the reference's feature set: variants 5 and 6 take it
    for variant in (5, 6):
        r = p.Renderer.MakeRenderer(32, 32, 1, 6, config_cameras(p, "book1_final", 32, 32), plain.getWorldPtr(), seed=SEED, variant=variant)
        with pytest.raises(p.capi.RtError, match=f"variant {variant} has no light-sampling form"):
            r.light_sampling("all")
        assert r.light_sampling_mode() == 0
        r.close()
    r = p.Renderer.MakeRenderer(32, 32, 1, 6, config_cameras(p, "book1_final", 32, 32), plain.getWorldPtr(), seed=SEED)
    with pytest.raises(p.capi.RtError, match="no light to sample"):
        r.light_sampling(2)
    r.Render()   # a refused enable leaves the renderer as it was
    r.close()


@pytest.mark.parametrize("name", ["lamp_room", "mixed_room"])
def test_uneven_refine_steps_and_passes_are_the_same_sums(p, monkeypatch, name):
    run = NW2.run(name)
    set_env(monkeypatch, {})
    r = make(p, run)
    for n in (1, 2, 1):
        r.refine(n)
    assert r.refine_info()["samples"] == 4
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    assert bits_equal(r.DownloadRenderbuffer(), T.resolve(run.sums, 4))
    r.close()
    for pass_spp in (1, 3):
        monkeypatch.setenv("RT06_PASS_SPP", str(pass_spp))
        r = make(p, run)
        info = r.pass_info()
        assert info["pass_spp"] == pass_spp and info["n_passes"] == -(-4 // pass_spp) > 1
        r.Render()
        assert bits_equal(r.DownloadRenderbuffer(), T.resolve(run.sums, 4))
        r.refine(4)
        assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
        r.close()


@pytest.mark.parametrize("big", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("name", NW2.EDGE_WORLDS)
def test_estimator_edges_are_the_twin_bit_for_bit(p, monkeypatch, name, big):
    """a small lamp so far away that drawn points are lost on its silhouette (failed scatters); a hit point inside a large sphere light; lights tangent to walls; a sphere under a quad light (two terms in pl); 16 sphere lights of different
    radii; and the same under the seed of _nee_worlds whose light-index draw is the uniform 1 (tests/test_light_sampling_spheres_cpu.py holds each
    world to what it is there for)"""
    run = NW2.run(name)
    assert run.followed.all()
    set_env(monkeypatch, NW.NARROW if big else NW.LDS)
    sums, _ = render_run(p, run, 0, NW.kernel_form_of((NW.BVH, 0, 1, big, 0)))
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert np.isfinite(sums).all() and (sums[..., :3] > 0).any(axis=2).mean() > 0.5


def test_mode_1_on_the_mixed_room_is_the_quad_twin_and_mode_2_differs(p, monkeypatch):
    set_env(monkeypatch, {})
    run = NW2.run("mixed_room")
    one, followed = T.frame_samples(as_oracle_world(run.scene.getWorldPtr()), as_oracle_camera(run.cam), run.W, run.H, run.spp, run.depth, run.seed, light_sampling=True)
    assert followed.all()
    one_sums = T.in_order_sums(one)
    r = make(p, run, mode=1)
    assert r.light_sampling_info() == {"enabled": True, "lights": 1}
    r.refine(run.spp)
    got = r.refine_sums()
    r.close()
    assert bits_equal(got, one_sums), mismatch_report(got, one_sums)   # the sphere emits and is not sampled, as ever
    assert not bits_equal(run.sums, one_sums)


def test_switching_between_modes(p, monkeypatch):
    set_env(monkeypatch, {})
    run = NW2.run("mixed_room")
    r = make(p, run, mode=1)
    r.enable_aov()
    r.refine(3)
    assert r.refine_info()["samples"] == 3
    r.light_sampling(1)                       # the same mode: the refinement goes on
    assert r.refine_info()["samples"] == 3
    r.light_sampling(2)                       # 1 -> 2: another estimator, another sequence
    assert r.refine_info()["samples"] == 0 and r.light_sampling_mode() == 2
    r.refine(3)
    r.light_sampling(2)                       # 2 -> 2 keeps it
    r.light_sampling("all")
    assert r.refine_info()["samples"] == 3
    r.refine(1)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling(1)                       # 2 -> 1 discards, and mode 1's table is still its own
    assert r.refine_info()["samples"] == 0 and r.light_sampling_info() == {"enabled": True, "lights": 1}
    r.light_sampling(2)
    r.light_sampling(0)                       # off after 2: the plain renderer's bits
    assert r.refine_info()["samples"] == 0 and r.light_sampling_mode() == 0
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.refine(run.spp)
    sums = r.refine_sums()
    r.close()
    off, followed = T2.frame_samples(as_oracle_world(run.scene.getWorldPtr()), as_oracle_camera(run.cam), run.W, run.H, run.spp, run.depth, run.seed, mode=0)
    assert followed.all()   # mode 0 of this twin is orc_radiance_batch bit for bit (tests/test_light_sampling_spheres_cpu.py)
    assert bits_equal(sums, T.in_order_sums(off)), mismatch_report(sums, T.in_order_sums(off))
    assert bits_equal(frame, T.resolve(T.in_order_sums(off), run.spp))
    fresh = make(p, run, mode=0)
    fresh.Render()
    assert bits_equal(fresh.DownloadRenderbuffer(), frame)
    fresh.close()


def test_two_ranks_in_mode_2_render_the_single_renderers_frame(p, monkeypatch):
    set_env(monkeypatch, {})
    run = NW2.run("mixed_room")
    frame = T.resolve(run.sums, run.spp)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    m = p.MultiRenderer.MakeRenderer(run.W, run.H, run.spp, run.depth, run.cam, run.scene.getWorldPtr(), 2, seed=run.seed)
    m.light_sampling(2)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), frame), mismatch_report(m.DownloadRenderbuffer(), frame)
    m.refine(run.spp)
    assert bits_equal(m.DownloadRenderbuffer(), frame)
    m.close()
    r = make(p, run)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), frame)
    r.close()


def test_noise_figure_falls_on_the_lamp_lit_cornell_box(p, monkeypatch):
    """64x64, 16 spp, depth 50: the relative standard error of the frame's mean luminance, strictly lower in mode 2 (measured: EXPERIMENTS.md E8)"""
    set_env(monkeypatch, {})
    W = H = 64
    scene = p.Scene.cornell_lamp()
    cam = p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)
    noise = {}
    for mode in (0, 2):
        r = p.Renderer.MakeRenderer(W, H, 16, 50, cam, scene.getWorldPtr(), seed=SEED)
        if mode:
            r.light_sampling(mode)
        r.refine(16)
        noise[mode] = r.noise()
        r.close()
    print(f"cornell_lamp noise figure at 64x64x16, depth 50: off {noise[0]:.4f}, mode 2 {noise[2]:.4f}, ratio {noise[2] / noise[0]:.3f}")
    assert np.isfinite(noise[2]) and noise[2] < noise[0]
