"""Run-ahead: a two-slot renderer generates and traces a queued render_async ahead of the caller's stream and only resolves in its order.
What a caller can see must not change: every queued frame has the bits of a synchronous Render() of a fresh one-slot renderer (RT06_RUN_AHEAD=0) — itself
held to the CPU oracle once per size — whatever the stream, with the camera moving between the calls, with other work of the caller between them, with
serial calls (refine, denoise) behind them and with the renderer closed right after them; and every renderer that cannot run ahead says so and
renders the same bits.  Frames are Book-1 final at 240x160x24 and at 61x37x4 (ragged tiles, padding blocks, two tiles per row), depth 8."""
import contextlib
import functools
import os

import numpy as np
import pytest

import _oracle as O
from _common import bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu

SIZES = [(240, 160, 24), (61, 37, 4)]
DEPTH = 8
SEED = 1984
CAMERAS = [((13, 2, 3), (0, 0, 0)), ((-6, 3, 10), (0, 0.5, 0)), ((4, 6, -11), (1, 0, 0))]
N_QUEUED = 8


@contextlib.contextmanager
def environment(**kv):
    """the renderer reads these when it is created"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def camera(mod, k, W, H):
    lookfrom, lookat = CAMERAS[k]
    return (mod.camera_defocus if mod is O else mod.DefocusBlurCamera)(lookfrom, lookat, (0, 1, 0), 20.0, W / H, 0.1, 10.0)


@functools.lru_cache(maxsize=None)
def scene(kind="bvh"):
    s = pkg().Scene.book1_final(SEED)
    return s.MakeHittableList() if kind == "list" else s


def make(size, k=0, kind="bvh", variant=0):
    W, H, spp = size
    return pkg().Renderer.MakeRenderer(W, H, spp, DEPTH, camera(pkg(), k, W, H), scene(kind).getWorldPtr(), seed=SEED, variant=variant)


@functools.lru_cache(maxsize=None)
def reference(size, k=0, kind="bvh", variant=0):
    """a synchronous Render() of a fresh one-slot renderer; computed once, shared, read-only"""
    with environment(RT06_RUN_AHEAD="0"):
        r = make(size, k, kind, variant)
    assert r.run_ahead_info() == {"slots": 1, "calls": 0, "overlapped": 0, "second_set_bytes": 0}
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    img.setflags(write=False)
    return img


def streams():
    """(a non-blocking stream, the legacy default stream) as the handles render_async takes; the first is kept alive by the caller"""
    import torch
    s = torch.cuda.Stream()
    return {"nonblocking": (s, s.cuda_stream), "default": (None, torch.cuda.default_stream().cuda_stream)}


def frame_buffers(size, n):
    import torch
    W, H, _ = size
    bufs = [torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0") for _ in range(n)]
    torch.cuda.synchronize()
    return bufs


def frame(buf, size):
    W, H, _ = size
    return buf.cpu().numpy().reshape(H, W, 4)


@pytest.mark.parametrize("size", SIZES)
def test_the_reference_is_the_cpu_oracle(size):
    W, H, spp = size
    oscene = O.Scene.book1_final(SEED)   # (owns the arrays its world points into: kept while the oracle renders)
    want, _ = O.render(oscene.world, camera(O, 0, W, H), W, H, spp, DEPTH, SEED)
    assert bits_equal(reference(size), want), mismatch_report(reference(size), want)


@pytest.mark.parametrize("which", ["nonblocking", "default"])
@pytest.mark.parametrize("size", SIZES)
def test_queued_frames_are_the_reference_bit_for_bit(size, which):
    import torch
    keep, st = streams()[which]
    want = reference(size)
    r = make(size)
    bufs = frame_buffers(size, N_QUEUED)
    for b in bufs:   # no host synchronisation between the calls
        r.render_async(st, b.data_ptr())
    torch.cuda.synchronize()
    info = r.run_ahead_info()
    print(f"{size} {which}: {info}, kernel times of the last call {r.kernel_times(0)}")
    for k, b in enumerate(bufs):
        assert bits_equal(frame(b, size), want), (k, mismatch_report(frame(b, size), want))
    W, H, spp = size
    assert info["slots"] == 2 and info["calls"] == N_QUEUED and info["second_set_bytes"] == W_pad_pixels(size) * spp * 60
    assert info["overlapped"] >= 1, info   # the run is not allowed to test nothing: frames were in flight together
    assert r.pass_info()["bytes_per_sample"] == 60 and r.pass_info()["buffer_bytes"] == info["second_set_bytes"]   # of one slot, not doubled
    assert all(t > 0 for t in r.kernel_times(0)) and all(t > 0 for t in r.kernel_times(N_QUEUED - 1))
    r.close()


def W_pad_pixels(size):
    """pixels of the frame's 8x8 tiles, padding included: what the per-pass buffers are sized for"""
    W, H, _ = size
    return ((W + 7) // 8) * ((H + 7) // 8) * 64


@pytest.mark.parametrize("size", SIZES)
def test_every_queued_frame_keeps_the_camera_of_its_call(size):
    import torch
    W, H, _ = size
    keep, st = streams()["nonblocking"]
    r = make(size)
    bufs = frame_buffers(size, N_QUEUED)
    for k, b in enumerate(bufs):
        r.set_camera(camera(pkg(), k % 3, W, H))
        r.render_async(st, b.data_ptr())
    torch.cuda.synchronize()
    assert r.run_ahead_info()["slots"] == 2 and r.run_ahead_info()["calls"] == N_QUEUED
    for k, b in enumerate(bufs):
        assert bits_equal(frame(b, size), reference(size, k % 3)), (k, mismatch_report(frame(b, size), reference(size, k % 3)))
    assert not bits_equal(reference(size, 0), reference(size, 1)) and not bits_equal(reference(size, 1), reference(size, 2))
    r.close()


@pytest.mark.parametrize("which", ["nonblocking", "default"])
@pytest.mark.parametrize("size", SIZES)
def test_the_resolve_stays_in_the_callers_stream_order(size, which):
    """render A into B, copy B -> C on the same stream, render A' into B: a resolve that ran ahead of the copy would put A' into C"""
    import torch
    W, H, _ = size
    keep, st = streams()[which]
    r = make(size)
    B, Cc = frame_buffers(size, 2)
    r.render_async(st, B.data_ptr())
    with torch.cuda.stream(keep if keep is not None else torch.cuda.default_stream()):
        Cc.copy_(B, non_blocking=True)
    r.set_camera(camera(pkg(), 1, W, H))
    r.render_async(st, B.data_ptr())
    torch.cuda.synchronize()
    assert r.run_ahead_info()["calls"] == 2
    assert bits_equal(frame(Cc, size), reference(size, 0)), mismatch_report(frame(Cc, size), reference(size, 0))
    assert bits_equal(frame(B, size), reference(size, 1)), mismatch_report(frame(B, size), reference(size, 1))
    r.close()


@pytest.mark.parametrize("size", SIZES)
def test_serial_calls_order_behind_queued_renders(size):
    """two renders, a refine step and a denoise, queued with no synchronisation, against the same calls with one between each"""
    import torch
    p = pkg()
    keep, st = streams()["nonblocking"]
    n_refine = 6

    def run(sync):
        r = make(size)
        r.enable_aov()
        bufs = frame_buffers(size, 2)
        wait = torch.cuda.synchronize if sync else (lambda: None)
        for b in bufs:
            r.render_async(st, b.data_ptr())
            wait()
        r.refine_async(n_refine, st)
        wait()
        r.denoise_async(st)
        torch.cuda.synchronize()
        filtered = np.zeros((size[1], size[0], 4), dtype=np.float32)
        p.capi.check(p.lib().rt_renderer_denoise_download(r.h, filtered, filtered.size))
        out = (r.run_ahead_info(), [frame(b, size) for b in bufs], r.refine_sums(), filtered, r.DownloadRenderbuffer())
        r.close()
        return out

    info, frames, sums, filtered, fb = run(sync=False)
    info_s, frames_s, sums_s, filtered_s, fb_s = run(sync=True)
    assert info["slots"] == 2 and info["calls"] == 2 and info_s["calls"] == 2 and info_s["overlapped"] == 0
    for f in frames + frames_s:
        assert bits_equal(f, reference(size)), mismatch_report(f, reference(size))
    assert bits_equal(sums, sums_s), mismatch_report(sums, sums_s)
    assert bits_equal(filtered, filtered_s), mismatch_report(filtered, filtered_s)
    assert bits_equal(fb, fb_s) and np.isfinite(sums[..., :3]).any()


def queued(r, size, n=4):
    import torch
    keep, st = streams()["nonblocking"]
    bufs = frame_buffers(size, n)
    for b in bufs:
        r.render_async(st, b.data_ptr())
    torch.cuda.synchronize()
    return [frame(b, size) for b in bufs]


@pytest.mark.parametrize("size", SIZES)
def test_renderers_that_cannot_run_ahead_say_so_and_render_the_same_bits(size):
    spp = size[2]
    with environment(RT06_PASS_SPP=str((spp + 2) // 3)):   # 24 spp: three passes of 8; 4 spp: two passes of 2
        r = make(size)
    assert r.pass_info()["n_passes"] == (3 if spp == 24 else 2) and r.run_ahead_info()["slots"] == 1
    for f in queued(r, size):
        assert bits_equal(f, reference(size)), mismatch_report(f, reference(size))
    assert r.run_ahead_info()["calls"] == 0 and r.run_ahead_info()["second_set_bytes"] == 0
    r.close()
    with environment(RT06_RUN_AHEAD="0"):
        r = make(size)
    assert r.run_ahead_info()["slots"] == 1
    for f in queued(r, size):
        assert bits_equal(f, reference(size)), mismatch_report(f, reference(size))
    assert r.run_ahead_info()["calls"] == 0
    r.close()
    for variant in (1, 2):   # a HittableList world: the baseline kernel, and the streaming kernel of a world that stays on one slot
        r = make(size, kind="list", variant=variant)
        assert r.kernel_info()["variant"] == variant and r.run_ahead_info()["slots"] == 1
        want = reference(size, 0, "list", variant)
        for f in queued(r, size):
            assert bits_equal(f, want), (variant, mismatch_report(f, want))
        assert r.run_ahead_info()["calls"] == 0
        r.close()


@pytest.mark.parametrize("size", SIZES)
def test_close_directly_after_queued_calls(size):
    import torch
    p = pkg()
    keep, st = streams()["nonblocking"]
    r = make(size)
    bufs = frame_buffers(size, 3)
    for b in bufs:
        r.render_async(st, b.data_ptr())
    r.close()   # drains what is queued before it frees what the queued launches use
    assert r.h is None
    for b in bufs:   # (the resolves were queued too: the frames are there without a further wait on the stream)
        assert bits_equal(frame(b, size), reference(size))
    torch.cuda.synchronize()
    again = make(size)
    again.Render()
    assert bits_equal(again.DownloadRenderbuffer(), reference(size))
    assert again.run_ahead_info()["slots"] == 2 and again.run_ahead_info()["calls"] == 0   # the blocking Render() never runs ahead
    again.close()
