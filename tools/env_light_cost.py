#!/usr/bin/env python3
"""What environment light sampling buys and what it costs (EXPERIMENTS.md E16).  One GPU.  Sections, any subset of:

    python tools/env_light_cost.py buys sun costs

  buys   three spheres (the prefab, a HittableList) under image_io.sky_environment(1024, 512), 600 x 600, depth 50, refined in steps of at most 64 samples: the
         noise figure (rt_renderer_refine_noise) of mode 32 after N = 16 and 64 samples, and of mode off — the parent's estimator, bit for bit — after N, 4 N,
         16 N and 64 N, each with the milliseconds of its refine steps so far (rt_renderer_last_kernel_ms, HIP events); then the samples and the time mode off
         needs to reach mode 32's figure at N = 64, read off its own 1 / sqrt(n) line; then (buys-behind) the map turned by 180 degrees, which puts the sun
         behind the camera: the pixels that see the sun's rim directly are noisy under any estimator of the bounces and weigh on the frame's figure
  sun    the same table under a 2048 x 1024 sky whose sun is the real one's size — a disc of 0.27 degrees radius, a few texels, 5e-6 of the sphere — at the radiance
         that keeps the 4-degree sun's power (60 * (4 / 0.27)^2): the case the plain estimator is worst at; then (sun-behind) the map turned by 180 degrees, and
         (sun-behind-diffuse) that with every surface Lambertian, where no glass or metal carries light from the sun along paths that neither estimator samples
  costs  the same world under maps of 1024 x 512 and 2048 x 1024: the dominant kernel's time (rt_renderer_kernel_times) of one refine step of 64 samples, mode off
         and mode 32, median of 9 after a warm-up; the ratio is what a sample costs
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["buys", "sun", "costs"])
ap.add_argument("--size", type=int, default=600)
a = ap.parse_args()
sys.path.insert(0, ROOT)
import __graft_entry__ as G
p = G.load_package()
from ray_tracing_v06_amd import image_io
print("source", p.lib().rt_source_hash().decode(), flush=True)
W = H = a.size
DEPTH, STEP = 50, 64


def renderer(env, mode, diffuse=False, rotate=0.0):
    if diffuse:   # the prefab's layout with every surface Lambertian: no specular path to the sun is left for either estimator to miss
        s = p.Scene()
        s.MakeSphere((0, -100.5, -1), 100.0, s.Lambertian((0.8, 0.8, 0.0)))
        for x, c in ((-1.0, (0.8, 0.8, 0.8)), (0.0, (0.1, 0.2, 0.5)), (1.0, (0.8, 0.6, 0.2))):
            s.MakeSphere((x, 0, -1), 0.5, s.Lambertian(c))
        s.MakeHittableList()
    else:
        s = p.Scene.three_spheres()
    s.set_environment(env, rotate_y=rotate)
    r = p.Renderer.MakeRenderer(W, H, STEP, DEPTH, p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, W / H), s.getWorldPtr())
    if mode:
        r.light_sampling(mode)
    assert r.kernel_env_light() == (mode == 32)
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


def buys(tag, env, diffuse=False, rotate=0.0):
    r = renderer(env, 32, diffuse, rotate)
    k = r.kernel_form()
    print(tag + " mode 32 kernel: world %d exact %d ext %d big %d nee %d, env_light %d" % (k["world"], k["exact"], k["ext"], k["big"], k["nee"], r.kernel_env_light()), flush=True)
    on = noise_at(r, [16, 64])
    r.close()
    r = renderer(env, 0, diffuse, rotate)
    off = noise_at(r, [16, 64, 256, 1024, 4096])
    r.close()
    for n, noise, ms in on:
        print(tag + " mode 32 samples %5d noise %.5f ms %.2f" % (n, noise, ms), flush=True)
    for n, noise, ms in off:
        print(tag + " mode off samples %5d noise %.5f ms %.2f" % (n, noise, ms), flush=True)
    for (n, noise_on, ms_on), (_, noise_off, ms_off) in zip(on, off):
        print(tag + " at %d samples: noise on / off %.3f, a mode-32 sample is worth %.2f plain ones; ms on / off %.2f" % (n, noise_on / noise_off, (noise_off / noise_on) ** 2, ms_on / ms_off), flush=True)
    n_ref, noise_ref, ms_ref = off[-1]     # mode off's own 1 / sqrt(n) line through its last point
    need = n_ref * (noise_ref / on[-1][1]) ** 2
    print(tag + " to mode 32's figure at %d samples (%.5f, %.2f ms) mode off needs %.0f samples, %.2f ms at its %.4f ms per sample: %.2f x the time" % (
        on[-1][0], on[-1][1], on[-1][2], need, need * ms_ref / n_ref, ms_ref / n_ref, (need * ms_ref / n_ref) / on[-1][2]), flush=True)


if "buys" in a.sections:
    buys("buys", image_io.sky_environment(1024, 512))
    buys("buys-behind", image_io.sky_environment(1024, 512), rotate=180.0)
if "sun" in a.sections:
    import numpy as np
    env = image_io.sky_environment(2048, 1024, sun_radius_deg=0.27).copy()   # the sky and the glow as they are; only the disc shrinks and brightens
    disc = (env == np.array([60.0, 54.0, 45.0], np.float32)).all(axis=2)
    env[disc] *= np.float32((4.0 / 0.27) ** 2)
    print("sun disc: %d texels of %d" % (int(disc.sum()), disc.size), flush=True)
    buys("sun", env)
    buys("sun-behind", env, rotate=180.0)
    buys("sun-behind-diffuse", env, diffuse=True, rotate=180.0)

if "costs" in a.sections:
    for w, h in ((1024, 512), (2048, 1024)):
        env = image_io.sky_environment(w, h)
        med = {}
        for mode in (0, 32):
            r = renderer(env, mode)
            r.refine(STEP)
            t = []
            for _ in range(9):
                r.refine(STEP)
                t.append(r.kernel_times(0)[1])
            med[mode] = statistics.median(t)
            print("costs map %dx%d mode %2d dominant kernel of a %d-sample step: median %.3f ms, min %.3f, max %.3f" % (w, h, mode, STEP, med[mode], min(t), max(t)), flush=True)
            r.close()
        print("costs map %dx%d a mode-32 sample costs %.3f of a plain one" % (w, h, med[32] / med[0]), flush=True)
