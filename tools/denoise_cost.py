#!/usr/bin/env python3
"""What the feature buffers and the denoiser cost (EXPERIMENTS.md E6), by HIP events.

  * a refine step with the feature buffers on against off: Book-1 final 1200x800 and the Cornell box 600x600, steps of 8 and of 64 samples
    (rt_renderer_last_kernel_ms: the events around the whole step, feature pass included; median of --repeats steps after one warm-up step);
  * rt_renderer_denoise_async between two events of a torch stream, default parameters, at 1200x800 and 3840x2160 (Book-1 final, 8 spp).

    python tools/denoise_cost.py [--repeats 9]
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9)
a = ap.parse_args()
p = G.load_package()
import torch


def setup(which, W, H):
    if which == "cornell_box":
        return p.Scene.cornell_box(), p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)
    return p.Scene.book1_final(1984), p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)


for which, W, H in (("book1_final", 1200, 800), ("cornell_box", 600, 600)):
    scene, cam = setup(which, W, H)
    for step in (8, 64):
        row = {"scene": which, "width": W, "height": H, "step": step}
        for mode in ("off", "on"):
            r = p.Renderer.MakeRenderer(W, H, step, 50, cam, scene.getWorldPtr())
            if mode == "on":
                r.enable_aov()
            r.refine(step)   # warm-up
            ms, kern = [], []
            for _ in range(a.repeats):
                r.refine(step)
                ms.append(r.last_kernel_ms())
                kern.append(sum(r.kernel_times(0)))
            row[f"step_ms_{mode}"] = round(statistics.median(ms), 4)
            row[f"three_kernels_ms_{mode}"] = round(statistics.median(kern), 4)   # primary + dominant + refine_resolve: the feature pass is the rest
            r.close()
        row["feature_pass_ms"] = round(row["step_ms_on"] - row["three_kernels_ms_on"] - (row["step_ms_off"] - row["three_kernels_ms_off"]), 4)
        print(json.dumps(row), flush=True)

stream = torch.cuda.Stream()
for W, H in ((1200, 800), (3840, 2160)):
    scene, cam = setup("book1_final", W, H)
    r = p.Renderer.MakeRenderer(W, H, 8, 50, cam, scene.getWorldPtr())
    r.enable_aov()
    r.refine(8)
    ms = []
    for _ in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r.denoise_async(stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"denoise": f"{W}x{H}", "iterations": 5, "ms": round(statistics.median(ms[1:]), 4), "first_call_ms": round(ms[0], 4),
                      "ns_per_pixel": round(statistics.median(ms[1:]) * 1e6 / (W * H), 3)}), flush=True)
    r.close()
