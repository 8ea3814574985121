#!/usr/bin/env python3
"""What the textured feature mode costs and buys (EXPERIMENTS.md E20).  One GPU.  Sections, any subset of:

    python tools/aov_textured_cost.py time quality

  time     a refine step of 16 samples at 400 x 400, depth 50, host clock around the synchronous call, 7 alternating rounds, best / median / worst:
           the textured room with features off and in the textured mode (their difference is the feature pass), beside the streaming kernel's own HIP-event time of
           the same step; and a texture-free room with features off, in the plain mode and in the textured mode (the TEX form against the plain form)
  quality  the textured room at 16 and 64 samples against 4096 samples of the same world: RMSE over the frame (the displayed values, after clamp and sqrt) of the
           noisy frame, of the denoised one with the default parameters, and of the denoised one with demodulate = 0
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as G
import _tri_worlds as TW

ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["time", "quality"])
ap.add_argument("--size", type=int, default=400)
ap.add_argument("--reference-spp", type=int, default=4096)
a = ap.parse_args()
p = G.load_package()
W = H = a.size
DEPTH, STEP = 50, 16
print("source", p.lib().rt_source_hash().decode(), flush=True)


def tiles(n, cell, seed):
    """an n x n image of cell x cell blocks of random saturated colours with a dark grid between them: detail a filter without the albedo would blur"""
    rng = np.random.default_rng(seed)
    img = np.repeat(np.repeat(rng.integers(60, 256, (n // cell, n // cell, 3)), cell, axis=0), cell, axis=1).astype(np.uint8)
    img[::cell, :, :] = 25
    img[:, ::cell, :] = 25
    return img


def textured_room():
    def add(s):
        wall = s.add_image(tiles(64, 8, 1), "repeat", "nearest")
        floor = s.add_image(tiles(128, 16, 2), "repeat", "bilinear")
        globe = s.add_image(tiles(64, 4, 3), "clamp", "bilinear")
        s.MakeQuad((0.5, 3.0, 9.95), (9, 0, 0), (0, 6.5, 0), s.ImageTexture(wall))
        s.MakeQuad((0.2, 0.02, 0.2), (9.6, 0, 0), (0, 0, 9.6), s.ImageTexture(floor))
        v, f, n, t = TW.mesh_io().uv_sphere(24, 12)
        s.MakeMesh(v, f, s.ImageTexture(globe), 1.5, 25.0, (5, 4.6, 6.5), uvs=t)
    return TW.tri_room(p, more=add)


def step_times(renderers, rounds=7):
    """{name: (sorted host ms of refine(STEP), sorted streaming-kernel ms)}, the renderers taking turns within every round"""
    host, kern = {k: [] for k in renderers}, {k: [] for k in renderers}
    for r in renderers.values():   # warm up: code objects, buffers
        r.refine(STEP)
    for _ in range(rounds):
        for name, r in renderers.items():
            r.refine_reset()
            t0 = time.perf_counter()
            r.refine(STEP)
            host[name].append((time.perf_counter() - t0) * 1e3)
            kern[name].append(r.kernel_times()[1])
    return {k: (sorted(host[k]), sorted(kern[k])) for k in renderers}


def report(label, res):
    for name, (h, k) in res.items():
        print("time", label, name, "refine(%d) host ms best %.3f median %.3f worst %.3f | streaming kernel ms median %.3f" % (STEP, h[0], h[len(h) // 2], h[-1], k[len(k) // 2]), flush=True)


if "time" in a.sections:
    scene, cam = textured_room(), TW.camera(p, W, H)
    rs = {"features off": p.Renderer.MakeRenderer(W, H, STEP, DEPTH, cam, scene.getWorldPtr()), "textured mode": p.Renderer.MakeRenderer(W, H, STEP, DEPTH, cam, scene.getWorldPtr())}
    rs["textured mode"].enable_aov(textured=True)
    report("textured room", step_times(rs))
    for r in rs.values():
        r.close()
    scene = TW.tri_room(p)
    rs = {k: p.Renderer.MakeRenderer(W, H, STEP, DEPTH, cam, scene.getWorldPtr()) for k in ("features off", "plain mode", "textured mode")}
    rs["plain mode"].enable_aov()
    rs["textured mode"].enable_aov(textured=True)
    report("texture-free room", step_times(rs))
    same = np.array_equal(rs["plain mode"].aov_sums().view(np.uint32), rs["textured mode"].aov_sums().view(np.uint32))
    print("time texture-free room: the two modes' feature sums have the same bits:", same, flush=True)
    for r in rs.values():
        r.close()

if "quality" in a.sections:
    scene, cam = textured_room(), TW.camera(p, W, H)
    ref = p.Renderer.MakeRenderer(W, H, 64, DEPTH, cam, scene.getWorldPtr(), seed=7)   # another seed than the frames it judges
    for _ in range(a.reference_spp // 64):
        ref.refine(64)
    truth = ref.DownloadRenderbuffer()[..., 0:3].astype(np.float64)
    ref.close()
    rmse = lambda img: float(np.sqrt(np.mean((img[..., 0:3].astype(np.float64) - truth) ** 2)))   # noqa: E731
    for spp in (16, 64):
        r = p.Renderer.MakeRenderer(W, H, 16, DEPTH, cam, scene.getWorldPtr())
        r.enable_aov(textured=True)
        for _ in range(spp // 16):
            r.refine(16)
        noisy, den, flat = r.DownloadRenderbuffer(), r.denoise(), r.denoise(demodulate=0)
        print("quality %d spp against %d spp, %d x %d: RMSE noisy %.5f | denoised, default parameters %.5f | denoised, demodulate = 0 %.5f"
              % (spp, a.reference_spp, W, H, rmse(noisy), rmse(den), rmse(flat)), flush=True)
        r.close()
