#!/usr/bin/env python3
"""What a session costs (EXPERIMENTS.md E5): Book-1 final at 1200x800, 500 samples as ONE Render() against refine steps of 500, 50 and 8;
the achieved HBM rate of refine_resolve_kernel next to resolve_kernel's; set_camera + Render() against destroy + create + Render().

    python tools/session_cost.py [--width 1200 --height 800 --spp 500 --depth 50]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1200)
ap.add_argument("--height", type=int, default=800)
ap.add_argument("--spp", type=int, default=500)
ap.add_argument("--depth", type=int, default=50)
a = ap.parse_args()
p = G.load_package()
W, H, SPP = a.width, a.height, a.spp
scene = p.Scene.book1_final(1984)
world = scene.getWorldPtr()
cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
cam_b = p.DefocusBlurCamera((12, 2.2, 4), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
n_local = ((W + 7) // 8) * ((H + 7) // 8) * 64


def wall(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


r = p.Renderer.MakeRenderer(W, H, SPP, a.depth, cam, world)
r.Render()   # warm-up
one_shot = min(wall(r.Render) for _ in range(3))
k = r.kernel_times(0)
one = {"what": f"Render() at {SPP} spp", "ms": round(one_shot, 3), "kernels_ms": [round(x, 3) for x in k],
       "resolve_TBps": round((n_local * SPP * 12 + W * H * 16) / (k[2] * 1e-3) / 1e12, 3)}
print(json.dumps(one), flush=True)
for step in (SPP, 50, 8):
    r.refine_reset()
    done, ms, kern = 0, [], [0.0, 0.0, 0.0]
    while done < SPP:
        n = min(step, SPP - done)
        ms.append(wall(lambda: r.refine(n)))
        kern = [x + y for x, y in zip(kern, r.kernel_times(0))]
        done += n
    total = sum(ms)
    # refine_resolve_kernel: 12 B per sample read, the accumulation read (not on a first step) and written, the frame written, per pixel
    bytes_moved = n_local * SPP * 12 + len(ms) * (W * H * 48) - W * H * 16
    print(json.dumps({"what": f"refine in steps of {step}", "steps": len(ms), "ms_per_step": round(total / len(ms), 3), "ms_total": round(total, 3),
                      "ratio_to_one_shot": round(total / one_shot, 4), "kernels_ms_total": [round(x, 3) for x in kern],
                      "refine_resolve_TBps": round(bytes_moved / (kern[2] * 1e-3) / 1e12, 3), "noise": r.noise()}), flush=True)
# a camera change: the renderer kept against the renderer rebuilt
r.Render()
kept = wall(lambda: (r.set_camera(cam_b), r.Render()))
r.close()


def rebuilt():
    global r
    r = p.Renderer.MakeRenderer(W, H, SPP, a.depth, cam_b, world)
    r.Render()


r = p.Renderer.MakeRenderer(W, H, SPP, a.depth, cam, world)
r.Render()
rebuild = wall(lambda: (r.close(), rebuilt()))
r.close()
print(json.dumps({"what": "camera change", "set_camera_plus_render_ms": round(kept, 3), "destroy_create_render_ms": round(rebuild, 3)}), flush=True)
