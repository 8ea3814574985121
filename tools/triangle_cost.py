#!/usr/bin/env python3
"""What triangles cost (EXPERIMENTS.md E9).  One GPU.  Sections, any subset of:

    python tools/triangle_cost.py ico leaks                       # this tree only
    python tools/triangle_cost.py --parent DIR ab flat ico leaks  # DIR: a built checkout of the commit to compare with

  ab     tools/ab_kernels.py's child (8 timed renders, per-kernel HIP-event means) on configs 2, 3 and 4, once per tree and round, alternating
  flat   the three kernels that read rt_quad::kind from the flat record, per tree and round: the baseline kernel (variant 1) on the Cornell box
         200x200x16, and a refine step of 16 samples with and without the feature pass on the Cornell box 600x600 (host wall-clock, best of 5)
  ico    throughput of the Cornell box 600x600, 64 spp, depth 50 with a metal icosphere(L), L = 1..5, and the memory form each level resolves to
  leaks  primary rays from outside a closed icosphere(3) aimed at points inside it: the share rt_probe_trace reports as a miss (>= 10^7 rays),
         and the numpy twin of tests/ on the first 20 000
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["ico", "leaks"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (sections ab, flat)")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]

AB_CHILD = open(os.path.join(ROOT, "tools", "ab_kernels.py")).read().split("CHILD = r'''", 1)[1].split("'''", 1)[0] + \
    '\nprint("  hash", p.lib().rt_source_hash().decode()[:12], flush=True)\n'
FLAT_CHILD = r'''
import os, sys, time
sys.path.insert(0, os.getcwd())
import __graft_entry__ as G
p = G.load_package()
cam = lambda W, H: p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)
scene = p.Scene.cornell_box()
r = p.Renderer.MakeRenderer(200, 200, 16, 50, cam(200, 200), scene.getWorldPtr(), variant=1)
r.Render()
t = []
for _ in range(5):
    r.Render(); t.append(r.last_kernel_ms())
r.close()
out = "baseline kernel best %.3f mean %.3f ms" % (min(t), sum(t) / len(t))
for aov in (False, True):
    r = p.Renderer.MakeRenderer(600, 600, 16, 50, cam(600, 600), scene.getWorldPtr())
    if aov: r.enable_aov()
    r.refine(16)
    t = []
    for _ in range(5):
        r.refine_reset(); t0 = time.perf_counter(); r.refine(16); t.append((time.perf_counter() - t0) * 1e3)
    r.close()
    out += " | refine 16 %s best %.3f mean %.3f ms" % ("with feature pass" if aov else "plain", min(t), sum(t) / len(t))
print(out, "| hash", p.lib().rt_source_hash().decode()[:12], flush=True)
'''


def child(code, tree, **env):
    e = dict(os.environ, **env)
    e.pop("RT06_LIB", None)
    res = subprocess.run([sys.executable, "-c", code], env=e, cwd=tree, capture_output=True, text=True, timeout=200)
    if res.returncode != 0:
        sys.exit(f"child failed in {tree}: rc {res.returncode}\n{res.stderr[-600:]}")   # nothing more is started on the GPU
    return " |".join(l.strip() for l in res.stdout.strip().splitlines())


sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as G
p = G.load_package()
from ray_tracing_v06_amd import mesh_io
print("source", p.lib().rt_source_hash().decode(), flush=True)
if "ab" in a.sections:
    for wl in ("book1_final", "cornell_box", "book2_final"):
        for rnd in range(1, a.rounds + 1):
            for name, tree in trees:
                print("ab", wl, "round", rnd, name, child(AB_CHILD, tree, AB_WORKLOAD=wl), flush=True)
if "flat" in a.sections:
    for rnd in range(1, a.rounds + 1):
        for name, tree in trees:
            print("flat round", rnd, name, child(FLAT_CHILD, tree), flush=True)
if "ico" in a.sections:
    W = H = 600
    spp = 64
    cam = p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0)
    for L in (None, 1, 2, 3, 4, 5):
        s = p.Scene.cornell_box()
        n = 0
        if L is not None:
            _, n = s.MakeMesh(*mesh_io.icosphere(L), s.Metal((0.8, 0.85, 0.88), 0.0), 90.0, 0.0, (278, 300, 200))
            s.BuildBVH_TopDown()
        r = p.Renderer.MakeRenderer(W, H, spp, 50, cam, s.getWorldPtr())
        r.Render()
        t = []
        for _ in range(5):
            r.Render()
            t.append(r.last_kernel_ms())
        f = r.kernel_form()
        print("ico level", L, "triangles", n, "ms best %.3f mean %.3f" % (min(t), sum(t) / len(t)), "Msamples/s %.1f" % (W * H * spp / min(t) / 1e3),
              "lds_resident", int(r.kernel_info()["lds_resident"]), "big", f["big"], "wide", f["wide"], "ext", f["ext"], "triangle family", int(r.kernel_triangles()), flush=True)
        r.close()
if "leaks" in a.sections:
    s = p.Scene()
    s.MakeMesh(*mesh_io.icosphere(3), s.Lambertian((0.5, 0.5, 0.5)))
    s.BuildBVH_TopDown()
    w = s.getWorldPtr()
    rng = np.random.default_rng(9)
    origin = np.array([3.0, 1.7, 2.2], np.float32)
    total = missed = 0
    first = None
    for _ in range(10):
        n = 1 << 20
        target = (rng.standard_normal((n, 3)) * 0.35).astype(np.float32)   # pulled into the ball of radius 0.9, inside the mesh's inscribed sphere (~0.98)
        target *= np.minimum(1.0, 0.9 / np.maximum(np.linalg.norm(target, axis=1), 1e-9))[:, None].astype(np.float32)
        rays = np.zeros((n, 7), np.float32)
        rays[:, 0:3] = origin
        rays[:, 3:6] = target - origin
        hit = np.asarray(p.api.probe_trace(w, rays)[0])
        total += n
        missed += int((hit == 0).sum())
        if first is None:
            first = (rays[:20000].copy(), hit[:20000].copy())
    print("leaks icosphere(3), 1280 triangles:", missed, "misses of", total, "rays =", missed / total, flush=True)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _tri_twin as TT
    from _common import as_oracle_world
    th = TT.closest_intersection(as_oracle_world(w), first[0])[0]
    print("leaks twin on the first", len(th), "rays:", int((th == 0).sum()), "misses; the probe's answer on every ray:", bool((th == first[1]).all()), flush=True)
