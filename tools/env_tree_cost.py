#!/usr/bin/env python3
"""What sampling the map and the light tree together costs and buys (EXPERIMENTS.md E19).  One GPU.  Sections, any subset of:

    python tools/env_tree_cost.py costs noise noise-image

The world: a 10 x 10 x 10 room whose right wall is missing — a window onto image_io.sky_environment(1024, 512) — lit as well by an icosphere(2) lamp of 320
triangles under its ceiling, holding a Lambertian and a metal sphere; 600 x 400, depth 50, a pinhole camera inside the room.

  costs        the dominant kernel's time (rt_renderer_kernel_times) of one refine step of 32 samples in modes 0, 16, 32 and 48, three alternating rounds, each
               turn a renderer of its own, one warm-up step and five timed ones: min, median, max per turn, so the spread between rounds is visible
  noise        the noise figure (rt_renderer_refine_noise) and the milliseconds of the refine steps so far (rt_renderer_last_kernel_ms) after 16, 64 and 256
               samples in each mode; then, per mode, the samples and the time it needs on its own 1 / sqrt(n) line through its last point to reach mode 48's
               figure at 64 samples: equal samples, and equal time
  noise-image  the same with the floor an image-textured parallelogram (the texture table's entry 1, repeat / bilinear): where modes 16 and 32 do not sample at all
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["costs", "noise", "noise-image"])
ap.add_argument("--width", type=int, default=600)
ap.add_argument("--height", type=int, default=400)
a = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as G
p = G.load_package()
from ray_tracing_v06_amd import image_io, mesh_io
print("source", p.lib().rt_source_hash().decode(), flush=True)
W, H = a.width, a.height
DEPTH, STEP = 50, 32
MODES = (0, 16, 32, 48)
ENV = image_io.sky_environment(1024, 512)


def room(image_floor):
    s = p.Scene()
    white, red = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05))
    if image_floor:
        s.set_image(np.random.default_rng(19).integers(0, 256, (3, 5, 3)).astype(np.uint8))
        floor = s.ImageTexture(s.add_image(np.random.default_rng(20).integers(64, 256, (16, 16, 3)).astype(np.uint8), "repeat", "bilinear"))
    else:
        floor = white
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), floor)
    s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), white)
    s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), red)
    s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 10, 0), white)
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 10, 0), white)
    s.MakeSphere((3, 1.5, 6), 1.5, s.Lambertian((0.3, 0.4, 0.8)))
    s.MakeSphere((7, 1.2, 5), 1.2, s.Metal((0.8, 0.8, 0.9), 0.1))
    s.MakeMesh(*mesh_io.icosphere(2), s.DiffuseLight((18, 15, 10)), 0.8, 15.0, (5, 7.5, 5.5))
    s.set_environment(ENV, rotate_y=0.0)
    s.BuildBVH_SAH()
    return s


def renderer(scene, mode):
    r = p.Renderer.MakeRenderer(W, H, STEP, DEPTH, p.PinholeCamera((5, 5, 0.5), (5, 4, 10), (0, 1, 0), 80.0, W / H), scene.getWorldPtr())
    if mode:
        r.light_sampling(mode)
    assert r.kernel_env_light() == (mode in (32, 48)) and r.kernel_light_tree() == (mode in (16, 48))
    return r


def noise_at(r, counts):
    """[(samples, noise, ms so far)] at each of the ascending sample counts"""
    out, done, ms = [], 0, 0.0
    for n in counts:
        while done < n:
            step = min(STEP, n - done)
            r.refine(step)
            ms += r.last_kernel_ms()
            done += step
        out.append((n, r.noise(), ms))
    return out


def noise(tag, scene):
    lines = {}
    for mode in MODES:
        r = renderer(scene, mode)
        if mode == 48:
            k = r.kernel_form()
            print(tag + " mode 48 kernel: world %d exact %d ext %d big %d nee %d, lights %d" % (k["world"], k["exact"], k["ext"], k["big"], k["nee"], r.light_sampling_info()["lights"]), flush=True)
        lines[mode] = noise_at(r, [16, 64, 256])
        r.close()
        for n, fig, ms in lines[mode]:
            print(tag + " mode %2d samples %4d noise %.5f ms %.2f" % (mode, n, fig, ms), flush=True)
    n48, fig48, ms48 = lines[48][1]
    for mode in MODES:
        n_ref, fig_ref, ms_ref = lines[mode][-1]   # the mode's own 1 / sqrt(n) line through its last point
        need = n_ref * (fig_ref / fig48) ** 2
        print(tag + " at 64 samples mode %2d has %.3f of mode 48's noise: a mode-48 sample is worth %.2f of its samples; to mode 48's figure (%.5f, %.2f ms) it needs %.0f samples, %.2f ms at its %.4f ms per sample: %.2f x the time" % (
            mode, lines[mode][1][1] / fig48, (lines[mode][1][1] / fig48) ** 2, fig48, ms48, need, need * ms_ref / n_ref, ms_ref / n_ref, (need * ms_ref / n_ref) / ms48), flush=True)


if "costs" in a.sections:
    scene = room(False)
    med = {m: [] for m in MODES}
    for rnd in range(3):
        for mode in MODES:
            r = renderer(scene, mode)
            r.refine(STEP)
            t = []
            for _ in range(5):
                r.refine(STEP)
                t.append(r.kernel_times(0)[1])
            r.close()
            med[mode].append(statistics.median(t))
            print("costs round %d mode %2d dominant kernel of a %d-sample step: median %.3f ms, min %.3f, max %.3f" % (rnd, mode, STEP, med[mode][-1], min(t), max(t)), flush=True)
    for mode in MODES[1:]:
        print("costs a mode-%d sample costs %s of a plain one (per round)" % (mode, " / ".join("%.3f" % (x / y) for x, y in zip(med[mode], med[0]))), flush=True)
    print("costs a mode-48 sample costs %s of a mode-16 one, %s of a mode-32 one (per round)" % (
        " / ".join("%.3f" % (x / y) for x, y in zip(med[48], med[16])), " / ".join("%.3f" % (x / y) for x, y in zip(med[48], med[32]))), flush=True)
if "noise" in a.sections:
    noise("noise", room(False))
if "noise-image" in a.sections:
    noise("noise-image", room(True))
