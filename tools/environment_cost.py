#!/usr/bin/env python3
"""What environment maps cost and what they buy (EXPERIMENTS.md E15).  One GPU.  Sections, any subset of:

    python tools/environment_cost.py --parent DIR ext2                     # DIR: a built checkout of the commit to compare with
    python tools/environment_cost.py three

  ext2   what the EXT 2 kernels pay with the map off: the Book-2 final scene (BASELINE configs[4]'s, the one shipped EXT 2 workload) through tools/ab_kernels.py,
         each tree's library under its own Python package (a library is bound symbol by symbol, so the parent's does not load under this tree's), the two trees
         alternating, two child processes of 8 renders per turn, --runs of them each (default 6); per tree the median over its runs of the mean dominant-kernel
         time, and the parent's own max - min
  three  the Book-1 final scene at BASELINE configs[2]'s shape (800 x 800, 1000 spp, depth 50) under its gradient (the EXT 0 default kernel), under a constant
         background (EXT 1) and under image_io.sky_environment (EXT 2): Msamples/s from the mean dominant-kernel time of 5 renders.  The price of the kernel
         FAMILY, not of the lookup
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, re, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["three"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (section ext2)")
ap.add_argument("--runs", type=int, default=6, help="child processes per tree (section ext2); ab_kernels.py runs two per call")
a = ap.parse_args()

THREE = r'''
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import __graft_entry__ as G
p = G.load_package()
from ray_tracing_v06_amd import image_io
W, H, spp = 800, 800, 1000
cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
for name in ("gradient", "constant", "sky"):
    s = p.Scene.book1_final(1984)
    if name == "constant":
        s.set_background((0.7, 0.8, 1.0))
    elif name == "sky":
        s.set_environment(image_io.sky_environment(1024, 512))
    r = p.Renderer.MakeRenderer(W, H, spp, 50, cam, s.getWorldPtr())
    r.Render()
    t = []
    for _ in range(5):
        r.Render()
        t.append(r.kernel_times()[1])
    ms = sum(t) / len(t)
    k = r.kernel_form()
    print(name, "ext %d exact %d big %d" % (k["ext"], k["exact"], k["big"]), "dominant kernel ms best %.3f mean %.3f" % (min(t), ms), "Msamples/s %.1f" % (W * H * spp / ms / 1e3), flush=True)
    r.close()
'''

sys.path.insert(0, ROOT)
import __graft_entry__ as G
print("source", G.load_package().lib().rt_source_hash().decode(), flush=True)
if "ext2" in a.sections:
    if not a.parent:
        sys.exit("section ext2 needs --parent")
    trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
    times = {name: [] for name in trees}
    for call in range((a.runs + 1) // 2):
        for name, tree in trees.items():
            e = dict(os.environ, AB_WORKLOAD="book2_final")
            e.pop("RT06_LIB", None)
            res = subprocess.run([sys.executable, os.path.join(tree, "tools", "ab_kernels.py"), os.path.join(tree, "ray-tracing-v06_amd", "csrc", "librt06.so")], env=e,
                                 cwd=tree, capture_output=True, text=True, timeout=280)
            if res.returncode != 0:
                sys.exit(f"ab_kernels.py failed in {tree}: rc {res.returncode}\n{res.stderr[-800:]}")   # nothing more is started on the GPU
            for line in res.stdout.splitlines():
                m = re.search(r"dominant ([0-9.]+)", line)
                if m:
                    times[name].append(float(m.group(1)))
                    print("ext2 turn", call + 1, name, line.strip(), flush=True)
    med = {n: statistics.median(t) for n, t in times.items()}
    spread = max(times["parent"]) - min(times["parent"])
    print("ext2 median of the runs' mean dominant-kernel ms: parent %.3f this %.3f (%+.3f ms, %+.2f %%) | parent max - min %.3f ms over %d runs | this max - min %.3f ms" % (
        med["parent"], med["this"], med["this"] - med["parent"], 100.0 * (med["this"] - med["parent"]) / med["parent"], spread, len(times["parent"]),
        max(times["this"]) - min(times["this"])), flush=True)
    print("ext2 verdict:", "not slower than the parent by more than its spread" if med["this"] - med["parent"] <= spread else "SLOWER than the parent by more than its spread", flush=True)
if "three" in a.sections:
    e = dict(os.environ)
    e.pop("RT06_LIB", None)
    res = subprocess.run([sys.executable, "-c", THREE], env=e, cwd=ROOT, capture_output=True, text=True, timeout=280)
    if res.returncode != 0:
        sys.exit(f"child failed: rc {res.returncode}\n{res.stderr[-800:]}")
    for line in res.stdout.strip().splitlines():
        if not line.startswith("/opt/"):
            print("three", line.strip(), flush=True)
