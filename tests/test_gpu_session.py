"""A renderer that lives across frames, on the GPU: the camera of every Render() and progressive refinement.

The contract under test (DESIGN.md "Sessions"): rt_renderer_set_camera is `params.cam = *m.cam` of Renderer.cu:117, and after ANY sequence of
refine steps the framebuffer has the bits of ONE render at samples_per_pixel = the accumulated count.  Every expected frame comes from the CPU
oracle (tests/_oracle.py), never from the GPU code under test; the bounds below are exact equality except the noise figure's 1e-9 (the fp64
summation-order bound (N - 1) * 2^-53 < 4.7e-10 for N <= 2^22 non-negative terms; nothing else differs)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _oracle as O
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, pkg

pytestmark = pytest.mark.gpu

SESSION_APP = os.path.join(ROOT, "tests", "cpp_session", "session_app")
THREADS = min(16, os.cpu_count() or 1)
STEPS = (1, 3, 4, 8)   # accumulated: 1, 4, 8, 16
f32 = np.float32


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


_frames = {}


def oracle(w, cam, W, H, spp, depth):
    geometry = (C.string_at(w.prims, w.n_prims * 32) if w.n_prims else b"") + (C.string_at(w.quads, w.n_quads * 80) if w.n_quads else b"")
    key = (w.kind, w.n_nodes, hash(geometry), bytes(cam), W, H, spp, depth)
    if key not in _frames:
        _frames[key] = O.render(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, depth, 1984, threads=THREADS)[0]
    return _frames[key]


def camera_pairs(p, kind, W, H):
    a = W / H
    if kind == "pinhole":
        return "three_spheres", p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, a), p.PinholeCamera((0.5, 0.3, 0.4), (0, 0, -1), (0, 1, 0), 70.0, a)
    if kind == "defocus":
        return "book1_final", p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, a, 0.1, 10.0), p.DefocusBlurCamera((-8, 3, 7), (0, 0.5, 0), (0, 1, 0), 30.0, a, 0.3, 9.0)
    if kind == "motion":
        return "book2_moving", p.MotionBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, a, 0.0, 1.0), p.MotionBlurCamera((-9, 3, 6), (0, 0.5, 0), (0, 1, 0), 35.0, a, 0.0, 0.5)
    assert kind == "type_change"
    return "book1_final", p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, a, 0.1, 10.0), p.PinholeCamera((4, 5, 12), (0, 0, 0), (0, 1, 0), 40.0, a)


def bad_camera(p, cam):
    bad = p.capi.Camera()
    C.memmove(C.byref(bad), C.byref(cam), C.sizeof(cam))
    bad.type = 3   # > RT_CAM_MOTION
    return bad


# ------------------------------------------------------------------------------------------------
# 1. the camera of every Render()
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pinhole", "defocus", "motion", "type_change"])
def test_render_follows_set_camera(p, kind):
    W, H, spp, depth = 160, 90, 4, 8
    which, cam_a, cam_b = camera_pairs(p, kind, W, H)
    scene = config_scene(p, which)   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, spp, depth, cam_a, w)
    r.Render()
    f1 = r.DownloadRenderbuffer()
    assert bits_equal(f1, oracle(w, cam_a, W, H, spp, depth)), mismatch_report(f1, oracle(w, cam_a, W, H, spp, depth))
    r.set_camera(cam_b)
    r.Render()
    f2 = r.DownloadRenderbuffer()
    assert bits_equal(f2, oracle(w, cam_b, W, H, spp, depth)), mismatch_report(f2, oracle(w, cam_b, W, H, spp, depth))
    assert not bits_equal(f2, f1)
    r.set_camera(cam_a)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), f1)
    # an invalid camera is refused and changes nothing
    with pytest.raises(p.capi.RtError) as e:
        r.set_camera(bad_camera(p, cam_b))
    assert e.value.code == 1
    with pytest.raises(p.capi.RtError):
        r.set_camera(None)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), f1)
    r.close()


def test_cpp_renderer_reads_the_callers_camera_object_at_every_render(p, tmp_path):
    """session_app mutates the camera OBJECT in place and never tells the renderer (Renderer.cu:117: `params.cam = *m.cam`)."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SESSION_APP)])
    W, H, spp, depth = 160, 90, 3, 8
    prefix = str(tmp_path / "cam")
    out = subprocess.check_output([SESSION_APP, "camera", str(W), str(H), str(spp), str(depth), prefix], text=True)
    assert len(re.findall(r"fnv=[0-9a-f]{16}", out)) == 4, out
    scene = config_scene(p, "book2_moving")   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    a = W / H
    first = p.MotionBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 30.0, a, 0.1, 1.0)
    cams = [first, p.MotionBlurCamera((-9, 3, 6), (0, 0.5, 0), (0, 1, 0), 35.0, a, 0.0, 0.5), first, p.PinholeCamera((4, 5, 12), (0, 0, 0), (0, 1, 0), 40.0, a)]
    frames = [np.fromfile(f"{prefix}_{i}.f32", dtype=np.float32).reshape(H, W, 4) for i in range(4)]
    for i, (got, cam) in enumerate(zip(frames, cams)):
        ref = oracle(w, cam, W, H, spp, depth)
        assert bits_equal(got, ref), f"frame {i}: " + mismatch_report(got, ref)
    assert not bits_equal(frames[1], frames[0]) and not bits_equal(frames[3], frames[0])


@pytest.mark.parametrize("ranks", [2, 3])
def test_multi_renderer_follows_set_camera(p, monkeypatch, ranks):
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    W, H, spp, depth = 100, 75, 4, 8
    which, cam_a, cam_b = camera_pairs(p, "motion", W, H)
    scene = config_scene(p, which)   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    m = p.MultiRenderer.MakeRenderer(W, H, spp, depth, cam_a, w, ranks)
    m.Render()
    f1 = m.DownloadRenderbuffer()
    assert bits_equal(f1, oracle(w, cam_a, W, H, spp, depth))
    m.set_camera(cam_b)
    m.Render()
    f2 = m.DownloadRenderbuffer()
    assert bits_equal(f2, oracle(w, cam_b, W, H, spp, depth)), mismatch_report(f2, oracle(w, cam_b, W, H, spp, depth))
    assert not bits_equal(f2, f1)
    with pytest.raises(p.capi.RtError) as e:
        m.set_camera(bad_camera(p, cam_a))
    assert e.value.code == 1
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), f2)
    m.set_camera(cam_a)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), f1)
    m.close()


# ------------------------------------------------------------------------------------------------
# 2. refinement equals one shot
# ------------------------------------------------------------------------------------------------
REFINE_SCENES = [("book1_final", 160, 90, 8), ("book2_moving", 100, 75, 12), ("three_spheres", 160, 90, 50), ("cornell_box", 72, 72, 50), ("book2_final", 64, 40, 40)]


@pytest.mark.parametrize("mode", ["plain", "pass_spp_2", "past_configured_count"])
@pytest.mark.parametrize("which,W,H,depth", REFINE_SCENES)
def test_refined_frame_is_the_one_shot_frame_bit_for_bit(p, monkeypatch, which, W, H, depth, mode):
    if mode == "pass_spp_2":
        monkeypatch.setenv("RT06_PASS_SPP", "2")   # read at creation: a step of 3, 4 or 8 spans several internal passes
    scene, cam = config_scene(p, which), config_cameras(p, which, W, H)
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 4 if mode == "past_configured_count" else 16, depth, cam, w)
    if which == "book2_final":
        assert not r.kernel_info()["lds_resident"]   # the global-memory form
    if which == "three_spheres":
        assert w.kind == p.capi.WORLD_LIST
    if mode == "pass_spp_2":
        assert r.refine_info()["pass_spp"] == 2
    if mode == "past_configured_count":
        assert r.refine_info()["pass_spp"] <= 4
    done = 0
    for step in STEPS:
        done += step
        assert r.refine(step) == done
        got, ref = r.DownloadRenderbuffer(), oracle(w, cam, W, H, done, depth)
        assert np.all(got[..., 3] == 1.0)
        assert bits_equal(got, ref), f"after {done} samples: " + mismatch_report(got, ref)
    assert r.refine_info()["bytes"] >= ((W + 7) // 8) * ((H + 7) // 8) * 64 * 16
    r.close()


def test_cpp_refine_matches_the_oracle_and_restarts_when_the_camera_moves(p, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(SESSION_APP)])
    W, H, depth = 100, 75, 8
    prefix = str(tmp_path / "ref")
    out = subprocess.check_output([SESSION_APP, "refine", str(W), str(H), str(depth), prefix] + [str(s) for s in STEPS], text=True)
    assert re.findall(r"^samples=(\d+)", out, re.M) == ["1", "4", "8", "16"], out
    noise = [float(x) for x in re.findall(r"noise=(\S+)", out)]
    assert len(noise) == 3 and all(math.isfinite(v) and v > 0 for v in noise) and noise[2] < noise[0]
    assert "after the camera moved: samples=2" in out
    scene = config_scene(p, "book2_moving")   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    cam = p.MotionBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 30.0, W / H, 0.1, 1.0)
    for done in (1, 4, 8, 16):
        got = np.fromfile(f"{prefix}_{done}.f32", dtype=np.float32).reshape(H, W, 4)
        assert bits_equal(got, oracle(w, cam, W, H, done, depth)), f"{done} samples: " + mismatch_report(got, oracle(w, cam, W, H, done, depth))
    moved = p.MotionBlurCamera((-9, 3, 6), (0, 0.5, 0), (0, 1, 0), 35.0, W / H, 0.0, 0.5)
    got = np.fromfile(f"{prefix}_moved.f32", dtype=np.float32).reshape(H, W, 4)
    assert bits_equal(got, oracle(w, moved, W, H, 2, depth))


# ------------------------------------------------------------------------------------------------
# 3. independence of Render() and the refinement state; what resets it
# ------------------------------------------------------------------------------------------------
def test_render_between_refine_steps_disturbs_neither(p, monkeypatch):
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # Render() itself carries running sums from pass to pass
    W, H, spp, depth = 160, 90, 7, 8
    which, cam, other = camera_pairs(p, "defocus", W, H)
    scene = config_scene(p, which)   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    fresh = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w)
    fresh.Render()
    one_shot = fresh.DownloadRenderbuffer()
    fresh.close()
    assert bits_equal(one_shot, oracle(w, cam, W, H, spp, depth))
    r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w)
    r.refine(4)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), one_shot)
    assert r.refine(4) == 8
    assert bits_equal(r.DownloadRenderbuffer(), oracle(w, cam, W, H, 8, depth))
    # the same bytes keep the count; reset and another camera take it to 0
    r.set_camera(cam)
    assert r.refine_info()["samples"] == 8
    r.refine_reset()
    assert r.refine_info()["samples"] == 0
    assert r.refine(3) == 3
    assert bits_equal(r.DownloadRenderbuffer(), oracle(w, cam, W, H, 3, depth))
    r.set_camera(other)
    assert r.refine_info()["samples"] == 0
    assert r.refine(5) == 5
    got = r.DownloadRenderbuffer()
    assert bits_equal(got, oracle(w, other, W, H, 5, depth)), mismatch_report(got, oracle(w, other, W, H, 5, depth))
    r.close()


# ------------------------------------------------------------------------------------------------
# 4. shards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world_size", [2, 3])
def test_sharded_renderers_refine_into_their_shards(p, monkeypatch, world_size):
    import torch
    monkeypatch.setenv("RT06_PASS_SPP", "2")
    W, H, depth = 100, 75, 8
    which, cam, _ = camera_pairs(p, "motion", W, H)
    scene = config_scene(p, which)   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    single = p.Renderer.MakeRenderer(W, H, 8, depth, cam, w)
    ranks = [p.Renderer.MakeRenderer(W, H, 8, depth, cam, w, rank=k, world_size=world_size) for k in range(world_size)]
    bufs = [torch.zeros(r.shard_floats(), dtype=torch.float32, device="cuda:0") for r in ranks]
    stream = torch.cuda.current_stream().cuda_stream
    done = 0
    for step in (3, 5):
        done += step
        single.refine(step)
        for r, buf in zip(ranks, bufs):
            r.refine_async(step, stream, buf.data_ptr())
        image = torch.empty(H * W * 4, dtype=torch.float32, device="cuda:0")
        ranks[0].assemble(torch.cat(bufs).data_ptr(), image.data_ptr(), stream)
        torch.cuda.synchronize()
        got = image.cpu().numpy().reshape(H, W, 4)
        assert bits_equal(got, single.DownloadRenderbuffer())
        assert bits_equal(got, oracle(w, cam, W, H, done, depth)), mismatch_report(got, oracle(w, cam, W, H, done, depth))
        assert all(r.refine_info()["samples"] == done for r in ranks)
    for r in ranks + [single]:
        r.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_multi_renderer_refine(p, monkeypatch, ranks):
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    W, H, depth = 100, 75, 8
    which, cam, other = camera_pairs(p, "motion", W, H)
    scene = config_scene(p, which)   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    m = p.MultiRenderer.MakeRenderer(W, H, 4, depth, cam, w, ranks)
    m.refine(3)
    assert bits_equal(m.DownloadRenderbuffer(), oracle(w, cam, W, H, 3, depth))
    m.refine(5)
    got = m.DownloadRenderbuffer()
    assert bits_equal(got, oracle(w, cam, W, H, 8, depth)), mismatch_report(got, oracle(w, cam, W, H, 8, depth))
    m.set_camera(other)   # every rank starts over
    m.refine(2)
    assert bits_equal(m.DownloadRenderbuffer(), oracle(w, other, W, H, 2, depth))
    with pytest.raises(p.capi.RtError) as e:
        m.refine(0)
    assert e.value.code == 1
    m.close()


# ------------------------------------------------------------------------------------------------
# 5. / 6. the accumulation and the noise figure
# ------------------------------------------------------------------------------------------------
def numpy_sums(w, cam, W, H, n, depth):
    """(sum R, sum G, sum B, sum Y^2) per pixel in float32, samples in order, from the oracle's per-sample radiance."""
    gid = np.repeat(np.arange(W * H, dtype=np.uint32), n)
    s = np.tile(np.arange(n, dtype=np.uint32), W * H)
    keys = np.ascontiguousarray(np.stack([gid, s], axis=1))
    rad = np.zeros((len(keys), 3), np.float32)
    ow, oc = as_oracle_world(w), as_oracle_camera(cam)
    assert O.lib().orc_radiance_batch(C.byref(ow), C.byref(oc), W, H, depth, 1984, len(keys), keys, rad) == 0
    rad = rad.reshape(W * H, n, 3)
    S, Q = np.zeros((W * H, 3), np.float32), np.zeros(W * H, np.float32)
    for k in range(n):
        c = rad[:, k, :]
        S = S + c
        Y = (f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1]) + f32(0.0722) * c[:, 2]
        Q = Q + Y * Y
    assert S.dtype == np.float32 and Q.dtype == np.float32
    return np.concatenate([S, Q[:, None]], axis=1).reshape(H, W, 4)


def numpy_noise(sums, n):
    S, Q = sums[..., :3], sums[..., 3]
    nf, n1 = f32(n), f32(n - 1)
    m = ((f32(0.2126) * S[..., 0] + f32(0.7152) * S[..., 1]) + f32(0.0722) * S[..., 2]) / nf
    v = np.maximum(f32(0.0), Q / nf - m * m) / n1
    assert m.dtype == np.float32 and v.dtype == np.float32
    ok = np.isfinite(m) & np.isfinite(v)   # rt06.h: a pixel whose m or v is not finite is left out of both means (all pixels where none is)
    return math.sqrt(v[ok].astype(np.float64).mean()) / m[ok].astype(np.float64).mean()


@pytest.mark.parametrize("which,depth", [("book1_final", 8), ("cornell_box", 50)])
def test_refine_sums_are_numpy_float32_sums_in_sample_order(p, monkeypatch, which, depth):
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # the sums cross pass boundaries
    W, H = 64, 48
    cam = config_cameras(p, which, W, H)
    scene = config_scene(p, which)   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 8, depth, cam, w)
    r.refine(5)
    r.refine(3)
    got, exp = r.refine_sums(), numpy_sums(w, cam, W, H, 8, depth)
    assert bits_equal(got[..., :3], exp[..., :3]), mismatch_report(got[..., :3], exp[..., :3])
    assert bits_equal(got[..., 3], exp[..., 3]), mismatch_report(got[..., 3], exp[..., 3])
    assert got[..., 3].max() > 0
    r.close()


@pytest.mark.parametrize("W,H", [(64, 48), (203, 117)])
def test_noise_repeats_bit_for_bit_and_matches_numpy(p, W, H):
    cam = config_cameras(p, "book1_final", W, H)
    scene = config_scene(p, "book1_final")   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 8, 8, cam, w)
    r.refine(1)
    with pytest.raises(p.capi.RtError) as e:   # a variance needs two samples
        r.noise()
    assert e.value.code == 1
    r.refine(7)
    a, b = r.noise(), r.noise()
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    exp = numpy_noise(r.refine_sums(), 8)
    print(f"noise {W}x{H} at 8 samples: GPU {a!r} numpy {exp!r} relative difference {abs(a - exp) / exp:.3e}")
    assert math.isfinite(a) and a > 0
    assert abs(a - exp) <= 1e-9 * exp
    r.close()


def test_noise_falls_as_samples_are_added(p):
    W, H = 96, 64
    cam = config_cameras(p, "book1_final", W, H)
    scene = config_scene(p, "book1_final")   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 16, 8, cam, w)
    r.refine(4)
    at4 = r.noise()
    r.refine(60)
    at64 = r.noise()
    print(f"noise at 4 samples {at4:.6f}, at 64 samples {at64:.6f}")
    assert r.refine_info()["samples"] == 64 and at64 < at4
    r.close()


def test_noise_leaves_non_finite_pixels_out(p):
    """The reference's arithmetic yields a NaN sample now and then ("NaN pixels"); here a light of 3e38 makes whole regions overflow.
    Such pixels are left out of both means instead of turning the figure into NaN."""
    s = p.Scene()
    s.MakeSphere((0, -100.5, -1), 100.0, s.Lambertian((0.5, 0.5, 0.5)))
    s.MakeQuad((-0.5, 0.2, -1.5), (1, 0, 0), (0, 1, 0), s.DiffuseLight((3e38, 3e38, 3e38)))
    s.set_background((0.2, 0.3, 0.5))
    s.BuildBVH_TopDown()
    W, H = 64, 40
    r = p.Renderer.MakeRenderer(W, H, 6, 8, p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, W / H), s.getWorldPtr())
    r.refine(6)
    sums = r.refine_sums()
    finite = np.isfinite(sums).all(axis=-1)
    assert 0.05 < finite.mean() < 0.95, finite.mean()   # both kinds of pixel are in the frame
    got, exp = r.noise(), numpy_noise(sums, 6)
    print(f"noise over the {finite.sum()} finite pixels of {W * H}: GPU {got!r} numpy {exp!r}")
    assert math.isfinite(got) and got > 0 and abs(got - exp) <= 1e-9 * exp
    r.close()


def test_noise_of_a_black_frame_is_infinite(p):
    """A world nothing lights: every sample is 0, the mean luminance is 0 -> +inf, not an error."""
    s = p.Scene()
    s.MakeSphere((0, 0, -1), 0.5, s.Lambertian((0.5, 0.5, 0.5)))
    s.set_background((0, 0, 0))
    s.BuildBVH_TopDown()
    W, H = 40, 24
    r = p.Renderer.MakeRenderer(W, H, 4, 8, p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, W / H), s.getWorldPtr())
    r.refine(4)
    assert not r.refine_sums().any()
    assert r.noise() == math.inf
    r.close()


# ------------------------------------------------------------------------------------------------
# 7. refusals      8. per-kernel times of a refine call
# ------------------------------------------------------------------------------------------------
def test_refusals(p):
    W, H = 64, 48
    cam = config_cameras(p, "book1_final", W, H)
    scene = config_scene(p, "book1_final")   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    base = p.Renderer.MakeRenderer(W, H, 4, 8, cam, w, variant=1)
    with pytest.raises(p.capi.RtError, match="baseline kernel") as e:
        base.refine(1)
    assert e.value.code == 1
    base.Render()   # still a working renderer
    base.close()
    r = p.Renderer.MakeRenderer(W, H, 4, 8, cam, w)
    L = p.lib()
    for call in (lambda: r.refine(0), lambda: r.refine_sums(), lambda: r.noise()):
        with pytest.raises(p.capi.RtError) as e:
            call()
        assert e.value.code == 1
    assert L.rt_renderer_refine_noise(r.h, None) == 1 and L.rt_renderer_set_camera(r.h, None) == 1
    r.refine(1)
    with pytest.raises(p.capi.RtError, match="2\\^31") as e:   # 1 + 2^31 samples
        r.refine(0x80000000)
    assert e.value.code == 1
    assert r.refine_info()["samples"] == 1
    wrong = np.zeros(W * H * 4 - 4, np.float32)
    assert L.rt_renderer_refine_download_sums(r.h, wrong, wrong.size) == 1
    assert bits_equal(r.DownloadRenderbuffer(), oracle(w, cam, W, H, 1, 8))
    r.close()
    shard = p.Renderer.MakeRenderer(W, H, 4, 8, cam, w, rank=1, world_size=2)
    shard.refine(2)
    with pytest.raises(p.capi.RtError, match="shard"):
        shard.refine_sums()
    assert math.isfinite(shard.noise())   # its own pixels, padding left out
    shard.close()


def test_kernel_times_follow_the_pass_count_of_each_call(p, monkeypatch):
    monkeypatch.setenv("RT06_PASS_SPP", "2")
    W, H = 160, 90
    cam = config_cameras(p, "book1_final", W, H)
    scene = config_scene(p, "book1_final")   # owns the arrays the flat world points into: alive for the whole test
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 6, 8, cam, w)
    assert r.pass_info()["n_passes"] == 3
    r.refine(9)             # 5 passes: more than a Render() of this renderer has
    t_refine = r.kernel_times(0)
    r.Render()              # 3 passes
    t_render, t_back = r.kernel_times(0), r.kernel_times(1)
    r.refine(1)             # 1 pass: fewer
    t_small = r.kernel_times(0)
    for t in (t_refine, t_render, t_back, t_small, r.kernel_times(1), r.kernel_times(2)):
        assert len(t) == 3 and all(math.isfinite(x) and x > 0 for x in t), t
    assert t_back == t_refine
    r.close()
