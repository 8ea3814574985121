"""The denoiser (rt_renderer_denoise) on the GPU.

1. A numpy float32 twin of prepare / iterations / final, written from include/rt06.h's statement of the filter, is BIT-IDENTICAL to the device
   output: only + - * / sqrt and comparisons, each rounded on its own, in the documented tap order.
2. Quality: against the existing, oracle-verified Render() at a sample count whose own noise figure is below one tenth of the 16-spp frame's,
   RMSE(denoised) < RMSE(16-spp refined), both in the framebuffer's gamma space (the bound the issue sets; the ratios are printed).

Measured on an MI355X (EXPERIMENTS.md E6): RMSE ratio denoised / refined 0.9203 on the Cornell box 200x200, 0.8371 on Book-1 final 300x200."""
import numpy as np
import pytest

from _common import bits_equal, config_cameras, config_scene, mismatch_report, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
H_TAPS = {-2: f32(0.0625), -1: f32(0.25), 0: f32(0.375), 1: f32(0.25), 2: f32(0.0625)}


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def gmax(a, b):   # glm::max(a, b) = a < b ? b : a
    return np.where(a < b, b, a).astype(f32)


def gmin(a, b):   # glm::min(a, b) = b < a ? b : a
    return np.where(b < a, b, a).astype(f32)


def luma(r, g, b):
    return (f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b


def twin_prepare(sums, aov, n, na, demodulate):
    inv_n, inv_na = f32(1.0) / f32(n), f32(1.0) / f32(na)
    c = sums[..., 0:3] * inv_n
    A = gmax(aov[..., 4:7] * inv_na, f32(1e-3))
    m = luma(sums[..., 0], sums[..., 1], sums[..., 2]) / f32(n)
    d = sums[..., 3] / f32(n) - m * m
    v = np.where(d < 0, f32(0.0), d).astype(f32) / f32(n - 1)
    I = c
    if demodulate:
        I = c / A
        ya = gmax(luma(A[..., 0], A[..., 1], A[..., 2]), f32(1e-3))
        v = v / (ya * ya)
    return I.astype(f32), v.astype(f32), (aov[..., 0:3] * inv_na).astype(f32), (aov[..., 3] * inv_na).astype(f32), A


def twin_iteration(I, v, N, Z, step, sigma_depth, sigma_lum):
    H, W = v.shape
    finite = np.isfinite(I).all(axis=2) & np.isfinite(v)
    yp = luma(I[..., 0], I[..., 1], I[..., 2])
    den_l = f32(sigma_lum) * np.sqrt(gmax(v, f32(0.0))) + f32(1e-6)
    sz = f32(sigma_depth) * f32(step)
    sw, sI, sv = np.zeros((H, W), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                w, Iq, vq = np.full((H, W), f32(0.140625)), I, v
            else:
                ys, xs = np.arange(H) + dy * step, np.arange(W) + dx * step
                inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
                yc, xc = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
                take = lambda a: a[yc][:, xc]
                Iq, vq, Nq, Zq = take(I), take(v), take(N), take(Z)
                valid = inside & take(finite)
                dn = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                wn = np.where(f32(0.0) < dn, dn, f32(0.0)).astype(f32)
                for _ in range(5):
                    wn = wn * wn
                dz = np.abs(Z - Zq) / (sz * gmin(Z, Zq) + f32(1e-6))
                wz = f32(1.0) / (f32(1.0) + dz * dz)
                dl = np.abs(yp - luma(Iq[..., 0], Iq[..., 1], Iq[..., 2])) / den_l
                wl = f32(1.0) / (f32(1.0) + dl * dl)
                w = (((H_TAPS[dx] * H_TAPS[dy]) * wn) * wz) * wl
                w = np.where(valid, w, f32(0.0)).astype(f32)   # a tap that is left out adds +0 to every sum: the same bits
                Iq, vq = np.where(valid[..., None], Iq, f32(0.0)).astype(f32), np.where(valid, vq, f32(0.0)).astype(f32)
            sw = sw + w
            sI = sI + w[..., None] * Iq
            sv = sv + (w * w) * vq
    I2, v2 = sI / sw[..., None], sv / (sw * sw)
    return np.where(finite[..., None], I2, I).astype(f32), np.where(finite, v2, v).astype(f32)


def twin_denoise(sums, aov, n, na, iterations, sigma_depth, sigma_lum, demodulate):
    with np.errstate(all="ignore"):
        I, v, N, Z, A = twin_prepare(sums, aov, n, na, demodulate)
        for i in range(iterations):
            I, v = twin_iteration(I, v, N, Z, 1 << i, sigma_depth, sigma_lum)
        rad = I * A if demodulate else I
        c = np.where(rad < 0, f32(0.0), rad).astype(f32)       # glm::max(rad, 0)
        c = np.where(f32(1.0) < c, f32(1.0), c).astype(f32)   # glm::min(.., 1)
        out = np.ones(I.shape[:2] + (4,), f32)
        out[..., 0:3] = np.sqrt(c)
    return out


def refined(p, which, W, H, n, depth=12):
    scene, cam = config_scene(p, which), config_cameras(p, which, W, H)
    r = p.Renderer.MakeRenderer(W, H, n, depth, cam, scene.getWorldPtr())
    r.enable_aov()
    r.refine(n)
    return r, scene, cam


@pytest.mark.parametrize("which,W,H", [("cornell_box", 96, 96), ("book1_final", 150, 100)])
@pytest.mark.parametrize("demodulate,iterations", [(1, 5), (1, 1), (0, 5), (0, 1)])
def test_numpy_twin_is_bit_identical(p, which, W, H, demodulate, iterations):
    r, _scene, _cam = refined(p, which, W, H, 16)
    dp = p.Renderer.denoise_params()
    frame = r.DownloadRenderbuffer()
    got = r.denoise(iterations=iterations, demodulate=demodulate)
    exp = twin_denoise(r.refine_sums(), r.aov_sums(), 16, 16, iterations, dp.sigma_depth, dp.sigma_lum, demodulate)
    assert bits_equal(got, exp), mismatch_report(got, exp)
    assert not bits_equal(got, frame)                       # it filtered something ...
    assert bits_equal(r.DownloadRenderbuffer(), frame)      # ... and the refined framebuffer is not what it wrote to
    r.close()


def test_feature_limit_below_the_colour_count_and_other_sigmas(p):
    """na < n (max_samples) and non-default sigmas go through the same twin"""
    W, H = 96, 64
    scene, cam = config_scene(p, "book2_moving"), config_cameras(p, "book2_moving", W, H)
    r = p.Renderer.MakeRenderer(W, H, 8, 12, cam, scene.getWorldPtr())
    r.enable_aov(4)
    r.refine(8)
    r.refine(8)
    assert r.aov_info()["samples"] == 4
    got = r.denoise(iterations=3, sigma_depth=0.2, sigma_lum=1.5)
    exp = twin_denoise(r.refine_sums(), r.aov_sums(), 16, 4, 3, f32(0.2), f32(1.5), 1)
    assert bits_equal(got, exp), mismatch_report(got, exp)
    r.close()


def test_constant_frame_with_constant_guides_comes_back_unchanged(p):
    """A light that fills the view, facing the camera: every sample is the emission (powers of two: every weighted sum is exact), the normal
    and the distance along the camera axis are the same in every pixel.  The filter must return the frame's bits, borders included."""
    W = H = 64
    s = p.Scene()
    m = s.add_material(p.capi.MAT_DIFFUSE_LIGHT, (0.25, 0.5, 1.0), 0.0)
    s.MakeQuad((-5, -5, -1), (10, 0, 0), (0, 10, 0), m)
    s.MakeHittableList()
    r = p.Renderer.MakeRenderer(W, H, 8, 8, p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 1.0), s.getWorldPtr())
    r.enable_aov()
    r.refine(8)
    f = r.aov()
    assert (f["coverage"] == 1).all() and np.unique(f["normal"].reshape(-1, 3), axis=0).shape[0] == 1
    frame = r.DownloadRenderbuffer()
    assert np.unique(frame.reshape(-1, 4), axis=0).shape[0] == 1
    for demodulate in (1, 0):
        assert bits_equal(r.denoise(demodulate=demodulate), frame)
    r.close()


def test_filter_and_refine_steps_on_different_streams_order_themselves(p):
    """refine on one stream, the filter on another, the next step on the first again: the library orders them by events, so the filtered
    frame is the one a blocking caller gets, and the step behind it does not disturb it"""
    import torch
    W, H = 160, 120
    scene, cam = config_scene(p, "book1_final"), config_cameras(p, "book1_final", W, H)
    blocking = p.Renderer.MakeRenderer(W, H, 8, 12, cam, scene.getWorldPtr())
    blocking.enable_aov()
    blocking.refine(8)
    want = blocking.denoise()
    blocking.refine(8)
    want16 = blocking.denoise()
    r = p.Renderer.MakeRenderer(W, H, 8, 12, cam, scene.getWorldPtr())
    r.enable_aov()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    r.refine_async(8, stream=a.cuda_stream)
    r.denoise_async(stream=b.cuda_stream)
    got = np.zeros((H, W, 4), f32)
    p.capi.check(p.lib().rt_renderer_denoise_download(r.h, got, got.size))
    r.refine_async(8, stream=a.cuda_stream)
    r.denoise_async(stream=b.cuda_stream)
    r.denoise_async(stream=a.cuda_stream)   # shares the colour buffers with the one before: ordered behind it
    got16 = np.zeros((H, W, 4), f32)
    p.capi.check(p.lib().rt_renderer_denoise_download(r.h, got16, got16.size))
    torch.cuda.synchronize()
    assert bits_equal(got, want) and bits_equal(got16, want16)
    assert bits_equal(r.DownloadRenderbuffer(), blocking.DownloadRenderbuffer())
    r.close()
    blocking.close()


def test_preconditions(p):
    W, H = 32, 32
    scene, cam = config_scene(p, "three_spheres"), config_cameras(p, "three_spheres", W, H)
    r = p.Renderer.MakeRenderer(W, H, 4, 8, cam, scene.getWorldPtr())
    r.refine(4)
    with pytest.raises(p.capi.RtError, match="feature"):
        r.denoise()
    r.enable_aov()
    r.refine(1)
    with pytest.raises(p.capi.RtError, match="2 samples"):
        r.denoise()
    r.refine(1)
    for bad in ({"iterations": 0}, {"iterations": 9}, {"sigma_lum": 0.0}, {"sigma_depth": float("nan")}):
        with pytest.raises(p.capi.RtError):
            r.denoise(**bad)
    assert r.denoise().shape == (H, W, 4)
    r.close()


def rmse(a, b, keep):
    d = (a[..., 0:3].astype(np.float64) - b[..., 0:3].astype(np.float64))[keep]
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("which,W,H", [("cornell_box", 200, 200), ("book1_final", 300, 200)])
def test_denoised_frame_is_closer_to_the_converged_render_than_the_refined_one(p, which, W, H):
    r, scene, cam = refined(p, which, W, H, 16, depth=50)
    noisy, noise16 = r.DownloadRenderbuffer(), r.noise()
    den = r.denoise()
    SPP = 4096   # the standard error falls as 1 / sqrt(n): 256 x the samples, a sixteenth of the noise; checked below, not assumed
    y = p.Renderer.MakeRenderer(W, H, SPP, 50, cam, scene.getWorldPtr())
    y.Render()
    yard = y.DownloadRenderbuffer()
    y.refine(SPP)   # the same frame, bit for bit (tests/test_gpu_session.py), through the path that has a noise figure
    assert bits_equal(y.DownloadRenderbuffer(), yard)
    assert y.noise() < noise16 / 10.0, (y.noise(), noise16)
    keep = np.isfinite(noisy).all(axis=2) & np.isfinite(den).all(axis=2) & np.isfinite(yard).all(axis=2)
    assert (~keep).sum() <= 1
    e_noisy, e_den = rmse(noisy, yard, keep), rmse(den, yard, keep)
    print(f"\n[quality] {which} {W}x{H}: RMSE 16 spp {e_noisy:.5f}, denoised {e_den:.5f}, ratio {e_den / e_noisy:.4f}; noise 16 spp {noise16:.5f}, yardstick {y.noise():.5f}")
    assert e_den < e_noisy
    r.close()
    y.close()
