#!/usr/bin/env python3
"""What the lens cameras cost (EXPERIMENTS.md E29).  One GPU.  Sections, any subset of:

    python tools/cameras_cost.py forms ortho          # this tree only
    python tools/cameras_cost.py --parent DIR ab      # DIR: a built checkout of the commit to compare with

  forms  a 1200 x 800 x 500 frame of book1_final at depth 50 under the scene's own eye, per form of primary_rays_lens_kernel — four projections, lens off / on,
         shutter off / on — the three rt_renderer_kernel_times (ray generator, tracing kernel, resolve; HIP events, summed over the frame's passes; best and
         median of 3 renders after a first one), next to the pinhole's and the defocus camera's on primary_rays_kernel.  The tracing kernel's time differs between
         projections because they see different parts of the scene; the generator's column is the one the forms are compared by.
  legacy the pinhole's and the defocus camera's three times alone, in each tree (with --parent: primary_rays_kernel on the parent commit, then here).
  ortho  the whole frame of an orthographic view along -z, where every primary ray has two zero direction components and so lies outside the fast-division class
         (the tracing kernel takes its irregular-ray path for them), next to the same window seen obliquely.
  ab     nothing an existing camera launches changed, so bench.py's headline must be what it was: this tree against the parent in alternating rounds, each round a
         process of its own (tools/cutout_cost.py's method; `bench.py --gpus 1 --steps 5 --warmup 2 --cpu-seconds 0`: the GPU leg and its parity check, no CPU baseline); per tree the median over the rounds, their ratio, and each tree's own round-to-round spread.
Every line starts with its section's name."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["forms", "ortho"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (section ab)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", default="1200,800,500", metavar="W,H,SPP")
a = ap.parse_args()
trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]

COMMON = r'''
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import __graft_entry__ as G
p = G.load_package()
W, H, SPP = (int(x) for x in sys.argv[1].split(","))
EYE, AT, UP = (13, 2, 3), (0, 0, 0), (0, 1, 0)
scene = p.Scene.book1_final(1984)


def timed(cam, n=3):
    r = p.Renderer.MakeRenderer(W, H, SPP, 50, cam, scene.getWorldPtr())
    r.Render()
    t = []
    for _ in range(n):
        r.Render(); t.append(r.kernel_times())
    r.close()
    t = np.array(t)
    return "generator best %.3f median %.3f ms, tracer best %.3f median %.3f ms, resolve best %.3f median %.3f ms" % tuple(
        x for k in range(3) for x in (t[:, k].min(), float(np.median(t[:, k]))))
'''

LEGACY = COMMON + r'''
print(sys.argv[2], p.lib().rt_source_hash().decode()[:12], "%d x %d x %d" % (W, H, SPP), flush=True)
print(sys.argv[2], "pinhole (primary_rays_kernel)", timed(p.PinholeCamera(EYE, AT, UP, 20.0, W / H)), flush=True)
print(sys.argv[2], "defocus (primary_rays_kernel)", timed(p.DefocusBlurCamera(EYE, AT, UP, 20.0, W / H, 0.1, 10.0)), flush=True)
'''

FORMS = LEGACY + r'''
for name, ctor, p0, p1 in (("perspective", p.api.PerspectiveCamera, 20.0, W / H), ("orthographic", p.api.OrthographicCamera, 5.0, W / H),
                           ("fisheye", p.api.FisheyeCamera, 180.0, W / H), ("panorama", p.api.PanoramaCamera, 360.0, 180.0)):
    for lens in (0, 1):
        for shutter in (0, 1):
            cam = ctor(EYE, AT, UP, p0, p1, 0.1 if lens else 0.0, 10.0, 0.0, 1.0 if shutter else 0.0)
            print("forms", "%s lens %d shutter %d" % (name, lens, shutter), timed(cam), flush=True)
'''

ORTHO = COMMON + r'''
print("ortho", "%d x %d x %d" % (W, H, SPP), flush=True)
print("ortho", "oblique", timed(p.api.OrthographicCamera(EYE, AT, UP, 5.0, W / H)), flush=True)
cam = p.api.OrthographicCamera((0, 1.5, 13.5), (0, 1.5, 0), UP, 5.0, W / H)
assert sum(1 for c in cam.w if c == 0) == 2
print("ortho", "along -z", timed(cam), flush=True)
print("ortho", "pinhole from there", timed(p.PinholeCamera((0, 1.5, 13.5), (0, 1.5, 0), UP, 20.0, W / H)), flush=True)
'''

if "legacy" in a.sections:
    for name, tree in trees:
        subprocess.run([sys.executable, "-c", LEGACY, a.size, "legacy " + name], cwd=tree, check=True, timeout=900)
if "forms" in a.sections:
    subprocess.run([sys.executable, "-c", FORMS, a.size, "forms"], cwd=ROOT, check=True, timeout=900)
if "ortho" in a.sections:
    subprocess.run([sys.executable, "-c", ORTHO, a.size], cwd=ROOT, check=True, timeout=900)
if "ab" in a.sections:
    values = {}
    for rnd in range(a.rounds):
        for name, tree in trees:
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--cpu-seconds", "0"], cwd=tree, check=True, timeout=600, stdout=subprocess.PIPE,
                                 text=True).stdout
            line = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
            print("ab", name, "round", rnd, line.get("metric"), line.get("value"), line.get("unit"), flush=True)
            values.setdefault(name, []).append(float(line["value"]))
    mid = {t: sorted(v)[len(v) // 2] for t, v in values.items()}
    line = "ab summary: " + ", ".join("%s %.4f" % (t, m) for t, m in mid.items())
    if "parent" in mid:
        spread = {t: (max(v) - min(v)) / mid[t] for t, v in values.items()}
        line += "; this / parent %.4f; the parent's spread over its rounds %.4f, this tree's %.4f" % (mid["this"] / mid["parent"], spread["parent"], spread["this"])
    print(line, flush=True)
