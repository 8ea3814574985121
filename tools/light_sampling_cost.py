#!/usr/bin/env python3
"""What light sampling buys and costs (EXPERIMENTS.md E7, E8), one GPU, one JSON line per measurement.

  * Cornell box 600x600, depth 50: the noise figure (rt_renderer_refine_noise) after 16, 64, 256 and 1024 samples, sampling off and on,
    with the milliseconds of the refine steps so far (rt_renderer_last_kernel_ms, HIP events);
  * the off-mode's noise figure at --target-spp (5000) samples, and the samples / milliseconds sampling on needs to get below it
    (steps of 64);
  * the quality table of E6 with sampling on: Cornell box 200x200, 16 spp, refined and denoised frame against Render() at 4096 plain
    spp (RMSE over RGB in the framebuffer's gamma space);
  * cost per sample: the dominant kernel's time per step of 64 samples, on against off (median of --repeats steps after a warm-up),
    on the Cornell box 600x600 and on the Book-2 final scene 800x800 — which has constant media, so the refusal is what is reported.

--mode quads (the default) is E7: the Cornell box, RT_LIGHT_SAMPLING_QUADS.  --mode all is E8: the Cornell box lit by a lamp (Scene.cornell_lamp),
RT_LIGHT_SAMPLING_ALL; its cost row still adds the Cornell box itself in mode 1, the figure E8 holds against the parent commit.
--sections picks among noise, target, quality, cost.

    python tools/light_sampling_cost.py [--mode quads|all] [--sections noise,target,quality,cost] [--repeats 9] [--target-spp 5000]
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--target-spp", type=int, default=5000)
ap.add_argument("--mode", choices=["quads", "all"], default="quads")
ap.add_argument("--sections", default="noise,target,quality,cost")
a = ap.parse_args()
sections = set(a.sections.split(","))
p = G.load_package()
import numpy as np


def cornell(W, H, lamp=(a.mode == "all")):
    return (p.Scene.cornell_lamp() if lamp else p.Scene.cornell_box()), p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)


def renderer(scene, cam, W, H, spp, on, mode=a.mode):
    r = p.Renderer.MakeRenderer(W, H, spp, 50, cam, scene.getWorldPtr())
    if on:
        try:
            r.light_sampling(mode)
        except p.capi.RtError:
            r.close()
            raise
    return r


tag = "cornell" if a.mode == "quads" else "cornell_lamp"
W = H = 600
scene, cam = cornell(W, H)
if "noise" in sections:
    for on in (False, True):
        r = renderer(scene, cam, W, H, 64, on)
        done, ms = 0, 0.0
        for upto in (16, 64, 256, 1024):
            while done < upto:
                n = min(64, upto - done)
                r.refine(n)
                ms += r.last_kernel_ms()
                done += n
            print(json.dumps({tag + "_600": "noise", "light_sampling": on, "samples": done, "noise": round(r.noise(), 5), "ms": round(ms, 2)}), flush=True)
        r.close()

if "target" in sections:
    r = renderer(scene, cam, W, H, 250, False)
    ms = 0.0
    for _ in range(a.target_spp // 250):
        r.refine(250)
        ms += r.last_kernel_ms()
    target = r.noise()
    print(json.dumps({tag + "_600": "target", "light_sampling": False, "samples": r.refine_info()["samples"], "noise": round(target, 6), "ms": round(ms, 1)}), flush=True)
    r.close()
    r = renderer(scene, cam, W, H, 64, True)
    ms, noise = 0.0, float("inf")
    while noise > target and r.refine_info()["samples"] < 2 * a.target_spp:
        r.refine(64)
        ms += r.last_kernel_ms()
        noise = r.noise()
    print(json.dumps({tag + "_600": "target", "light_sampling": True, "samples": r.refine_info()["samples"], "noise": round(noise, 6), "ms": round(ms, 1)}), flush=True)
    r.close()

if "quality" in sections:
    W = H = 200
    scene, cam = cornell(W, H)
    r = renderer(scene, cam, W, H, 4096, False)
    r.Render()
    yard = r.DownloadRenderbuffer()[..., :3]
    r.close()
    for on in (False, True):
        r = renderer(scene, cam, W, H, 16, on)
        r.enable_aov()
        r.refine(16)
        refined, noise = r.DownloadRenderbuffer()[..., :3], r.noise()
        den = r.denoise()[..., :3]
        rmse = lambda x: float(np.sqrt(np.mean((x.astype(np.float64) - yard) ** 2)))
        print(json.dumps({tag + "_200": "quality at 16 spp", "light_sampling": on, "noise": round(noise, 5), "rmse_refined": round(rmse(refined), 5),
                          "rmse_denoised": round(rmse(den), 5), "ratio": round(rmse(den) / rmse(refined), 4)}), flush=True)
        r.close()

# cost per step of 64 samples; (world, mode): mode quads measures E7's pair, mode all the lamp world in mode 2 and the Cornell box in mode 1 (E8's "mode 1 must not pay")
costs = [("cornell_box", "quads", 600, 600), ("book2_final", "quads", 800, 800)] if a.mode == "quads" else [("cornell_lamp", "all", 600, 600), ("cornell_box", "quads", 600, 600)]
for which, mode, W, H in (costs if "cost" in sections else []):
    if which.startswith("cornell"):
        scene, cam = cornell(W, H, lamp=(which == "cornell_lamp"))
    else:
        scene, cam = p.Scene.book2_final(1984), p.MotionBlurCamera((478, 278, -600), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    row = {"cost_per_step_of_64": which, "mode": mode, "width": W, "height": H}
    for on in (False, True):
        try:
            r = renderer(scene, cam, W, H, 64, on, mode)
        except p.capi.RtError as e:
            row["refused"] = str(e)
            continue
        r.refine(64)   # warm-up
        dom = []
        for _ in range(a.repeats):
            r.refine(64)
            dom.append(r.kernel_times(0)[1])
        row["dominant_ms_on" if on else "dominant_ms_off"] = round(statistics.median(dom), 4)
        r.close()
    if "dominant_ms_on" in row:
        row["on_over_off"] = round(row["dominant_ms_on"] / row["dominant_ms_off"], 4)
    print(json.dumps(row), flush=True)
