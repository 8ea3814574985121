"""Light sampling on the GPU: the NEE instantiations of render_kernel_stream against the numpy twin of a whole sample
(tests/_nee_twin.py, pinned to the oracle by tests/test_light_sampling_cpu.py), bit for bit, in the LDS-resident and the global-memory
form; what switching it on and off does to a renderer's state; and that it leaves every other path — materials that do not sample,
feature buffers, the multi-GPU driver — with the bits it had."""
import numpy as np
import pytest

import _nee_twin as T
from _common import as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, pkg

pytestmark = pytest.mark.gpu

SEED = 1984


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def twin_samples(scene, cam, W, H, spp, depth, on=True):
    return T.frame_samples(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, spp, depth, SEED, light_sampling=on)


@pytest.fixture(scope="module")
def cornell(p):
    """the Cornell box at 32x32, depth 6, and the twin's four samples per pixel with sampling on (computed once, never modified)"""
    W = H = 32
    scene = config_scene(p, "cornell_box")
    cam = config_cameras(p, "cornell_box", W, H)
    samples, followed = twin_samples(scene, cam, W, H, 4, 6)
    assert followed.all()
    samples.setflags(write=False)
    return scene, cam, W, H, 6, samples


def make(p, scene, cam, W, H, spp, depth, on=True, variant=0):
    r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, scene.getWorldPtr(), seed=SEED, variant=variant)
    if on:
        r.light_sampling(True)
    return r


@pytest.mark.parametrize("spp", [1, 4])
def test_cornell_box_is_the_twin_bit_for_bit_however_the_samples_are_cut(p, cornell, spp):
    scene, cam, W, H, depth, samples = cornell
    sums = T.in_order_sums(samples[:, :, :spp])
    frame = T.resolve(sums, spp)
    r = make(p, scene, cam, W, H, spp, depth)
    assert r.light_sampling_info() == {"enabled": True, "lights": 1}
    r.Render()
    img = r.DownloadRenderbuffer()
    assert bits_equal(img, frame), mismatch_report(img, frame)
    r.refine(spp)
    assert bits_equal(r.DownloadRenderbuffer(), frame) and bits_equal(r.refine_sums(), sums), mismatch_report(r.refine_sums(), sums)
    r.refine_reset()
    for _ in range(spp):
        r.refine(1)
    assert bits_equal(r.DownloadRenderbuffer(), frame) and bits_equal(r.refine_sums(), sums), mismatch_report(r.refine_sums(), sums)
    r.close()
    assert (samples[:, :, :spp].sum(axis=(2, 3)) > 0).mean() > 0.5   # a sampled light reaches most pixels, even at this sample count


def two_light_room(p):
    """a closed 6-quad room seen from inside, two quad lights of different size (one skew), a metal, a checker and a dielectric sphere"""
    s = p.Scene()
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    light_a, light_b = s.DiffuseLight((8, 8, 8)), s.DiffuseLight((20, 14, 6))
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), white)       # floor
    s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), white)      # ceiling
    s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), red)         # left
    s.MakeQuad((10, 0, 0), (0, 10, 0), (0, 0, 10), green)      # right
    s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 10, 0), white)      # back
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 10, 0), white)       # front, behind the camera
    s.MakeQuad((2, 9.9, 3), (2, 0, 0), (0, 0, 2), light_a)
    s.MakeQuad((6.5, 9.5, 6), (1, 0.2, 0), (0, 0.1, 0.7), light_b)
    s.MakeSphere((3, 1.5, 6), 1.5, s.Metal((0.8, 0.8, 0.9), 0.1))
    s.MakeSphere((7, 1.2, 5), 1.2, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    s.MakeSphere((5, 1, 3), 1.0, s.Dielectric((1, 1, 1), 1.5))
    s.BuildBVH_SAH()
    return s


def test_two_light_room_is_the_twin_in_the_lds_and_the_global_memory_form(p, monkeypatch):
    W = H = 32
    spp, depth = 4, 8
    scene = two_light_room(p)
    cam = p.PinholeCamera((5, 5, 0.5), (5, 4, 10), (0, 1, 0), 80.0, W / H)
    samples, followed = twin_samples(scene, cam, W, H, spp, depth)
    pixel_followed = followed.all(axis=2)
    assert 0.5 < pixel_followed.mean() < 1.0   # the dielectric sphere is in view: there the twin stops, elsewhere it goes all the way
    sums = T.in_order_sums(np.where(followed[..., None], samples, 0))
    got = {}
    for form in ("lds", "global"):
        if form == "global":
            monkeypatch.setenv("RT06_FORCE_BIG", "1")   # as tests/test_gpu_parity.py forces the global-memory path
        r = make(p, scene, cam, W, H, spp, depth)
        assert r.kernel_info()["lds_resident"] == (form == "lds") and r.light_sampling_info() == {"enabled": True, "lights": 2}
        r.refine(spp)
        got[form] = (r.refine_sums(), r.DownloadRenderbuffer())
        r.close()
        assert bits_equal(got[form][0][pixel_followed], sums[pixel_followed]), form + ": " + mismatch_report(got[form][0][pixel_followed], sums[pixel_followed])
    assert bits_equal(got["lds"][0], got["global"][0]) and bits_equal(got["lds"][1], got["global"][1])
    assert np.isfinite(got["lds"][0][pixel_followed]).all()


def test_a_world_without_lambertian_hits_draws_nothing_more(p):
    """metal, dielectric and one quad light only: no hit ever samples, so every per-pixel sum keeps the bits it has with sampling off"""
    s = p.Scene()
    mirror, glass, light = s.Metal((0.8, 0.7, 0.6), 0.2), s.Dielectric((1, 1, 1), 1.5), s.DiffuseLight((6, 6, 6))
    s.MakeQuad((-6, -0.5, -8), (12, 0, 0), (0, 0, 12), mirror)
    s.MakeQuad((-1, 3, -3), (2, 0, 0), (0, 0, 2), light)
    s.MakeSphere((-1, 0.5, -2), 1.0, glass)
    s.MakeSphere((1.2, 0.5, -2.5), 1.0, mirror)
    s.BuildBVH_TopDown()
    W, H, spp, depth = 40, 24, 4, 12
    cam = p.PinholeCamera((0, 1.5, 2), (0, 0.5, -2), (0, 1, 0), 70.0, W / H)
    sums = []
    for on in (False, True):
        r = make(p, s, cam, W, H, spp, depth, on=on)
        r.refine(spp)
        sums.append(r.refine_sums())
        r.close()
    assert bits_equal(sums[0], sums[1]), mismatch_report(sums[1], sums[0])
    assert (sums[0][..., :3] > 0).any(axis=2).mean() > 0.5


def test_enable_discards_the_refinement_and_disable_restores_the_plain_renderer(p, cornell):
    scene, cam, W, H, depth, samples = cornell
    plain = make(p, scene, cam, W, H, 4, depth, on=False)
    plain.Render()
    plain_frame = plain.DownloadRenderbuffer()
    plain.refine(4)
    plain_sums = plain.refine_sums()
    plain.close()
    r = make(p, scene, cam, W, H, 4, depth, on=False)
    assert r.light_sampling_info() == {"enabled": False, "lights": 1}
    r.refine(3)
    assert r.refine_info()["samples"] == 3
    r.light_sampling(False)                       # nothing changes: the refinement goes on
    assert r.refine_info()["samples"] == 3
    r.light_sampling(True)                        # another estimator: what was accumulated belongs to another sequence
    assert r.refine_info()["samples"] == 0 and r.light_sampling_info()["enabled"]
    r.refine(4)
    assert bits_equal(r.refine_sums(), T.in_order_sums(samples)) and not bits_equal(r.refine_sums(), plain_sums)
    r.light_sampling(False)
    assert r.refine_info()["samples"] == 0 and not r.light_sampling_info()["enabled"]
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), plain_frame)
    r.refine(4)
    assert bits_equal(r.refine_sums(), plain_sums)
    r.close()


def test_variants_without_a_light_sampling_form_are_refused(p, cornell):
    scene, cam, W, H, depth, _ = cornell
    r = make(p, scene, cam, W, H, 1, depth, on=False, variant=1)
    with pytest.raises(p.capi.RtError, match="variant 1") as e:
        r.light_sampling(True)
    assert e.value.code == 1
    r.close()
    plain = config_scene(p, "book1_final")   # a BVH world of the reference's feature set: variants 5 and 6 take it
    for variant in (5, 6):
        r = make(p, plain, config_cameras(p, "book1_final", W, H), W, H, 1, depth, on=False, variant=variant)
        with pytest.raises(p.capi.RtError, match=f"variant {variant}"):
            r.light_sampling(True)
        assert r.light_sampling_info() == {"enabled": False, "lights": 0}
        r.close()
    r = make(p, plain, config_cameras(p, "book1_final", W, H), W, H, 1, depth, on=False)
    with pytest.raises(p.capi.RtError, match="no quad light"):
        r.light_sampling(True)
    r.Render()   # a refused enable leaves the renderer as it was
    r.close()


def test_feature_buffers_keep_their_bits_and_the_denoiser_runs(p, cornell):
    scene, cam, W, H, depth, samples = cornell
    aov = []
    for on in (False, True):
        r = make(p, scene, cam, W, H, 4, depth, on=on)
        r.enable_aov()
        r.refine(4)
        aov.append(r.aov_sums())
        if on:
            assert bits_equal(r.refine_sums(), T.in_order_sums(samples))
            den = r.denoise()
            assert den.shape == (H, W, 4) and np.isfinite(den).all() and den[..., :3].max() > 0
        r.close()
    assert bits_equal(aov[0], aov[1])


def test_two_ranks_render_the_single_renderers_frame(p, cornell, monkeypatch):
    scene, cam, W, H, depth, samples = cornell
    frame = T.resolve(T.in_order_sums(samples), 4)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    m = p.MultiRenderer.MakeRenderer(W, H, 4, depth, cam, scene.getWorldPtr(), 2, seed=SEED)
    m.light_sampling(True)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), frame)
    m.refine(4)
    assert bits_equal(m.DownloadRenderbuffer(), frame)
    m.close()
    r = make(p, scene, cam, W, H, 4, depth)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), frame)
    r.close()


def test_noise_figure_falls_on_the_cornell_box(p):
    """64x64, 16 spp, depth 50: the relative standard error of the frame's mean luminance, strictly lower with sampling on (measured: EXPERIMENTS.md E7)"""
    W = H = 64
    scene = config_scene(p, "cornell_box")
    cam = config_cameras(p, "cornell_box", W, H)
    noise = {}
    for on in (False, True):
        r = make(p, scene, cam, W, H, 16, 50, on=on)
        r.refine(16)
        noise[on] = r.noise()
        r.close()
    print(f"noise figure at 64x64x16, depth 50: off {noise[False]:.4f}, on {noise[True]:.4f}, ratio {noise[True] / noise[False]:.3f}")
    assert np.isfinite(noise[True]) and noise[True] < noise[False]
