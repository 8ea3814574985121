#!/usr/bin/env python3
"""What vertex normals cost (EXPERIMENTS.md E12).  One GPU.  Sections, any subset of:

    python tools/smooth_normals_cost.py table                      # this tree only
    python tools/smooth_normals_cost.py --parent DIR existing table  # DIR: a built checkout of the commit to compare with

  existing  the triangle families WITHOUT a table against the parent, E9's worlds and method: the Cornell box 600x600, 64 spp, depth 50 with a metal
            icosphere(5) (20 480 flat triangles, the global-memory form), and two controls without a triangle — the Book-2 final scene 400x400x32 and
            config 2 (Book-1 final scene) 600x400x32 —, once per tree and round, alternating: dominant-kernel HIP-event time, best and mean of 5 renders
  table     the price of the table in this tree: the same Cornell room with an icosphere(L), L = 3 and 5, flat and with its vertex normals on —
            dominant-kernel time and Gsamples/s
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["table"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (section existing)")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]

CHILD = r'''
import os, sys
sys.path.insert(0, os.getcwd())
import __graft_entry__ as G
p = G.load_package()
from ray_tracing_v06_amd import mesh_io
wl, level, smooth = os.environ["SN_WORKLOAD"], int(os.environ.get("SN_LEVEL", "5")), os.environ.get("SN_SMOOTH") == "1"
if wl == "cornell_ico":
    W, H, spp = 600, 600, 64
    cam = p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0)
    s = p.Scene.cornell_box()
    v, f = mesh_io.icosphere(level)
    if smooth:
        s.MakeMesh(v, f, s.Metal((0.8, 0.85, 0.88), 0.0), 90.0, 0.0, (278, 300, 200), normals=mesh_io.icosphere_normals(level))
    else:
        s.MakeMesh(v, f, s.Metal((0.8, 0.85, 0.88), 0.0), 90.0, 0.0, (278, 300, 200))
    s.BuildBVH_TopDown()
elif wl == "book2_final":
    W, H, spp = 400, 400, 32
    cam = p.MotionBlurCamera((478, 278, -600), (278, 278, 0), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    s = p.Scene.book2_final(1984)
else:
    W, H, spp = 600, 400, 32
    cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
    s = p.Scene.book1_final(1984)
r = p.Renderer.MakeRenderer(W, H, spp, 50, cam, s.getWorldPtr())
r.Render()
t = []
for _ in range(5):
    r.Render()
    t.append(r.kernel_times()[1])
f = r.kernel_form()
on = r.shading_normals_info()["enabled"] if hasattr(r, "shading_normals_info") else False
print("dominant kernel ms best %.3f mean %.3f" % (min(t), sum(t) / len(t)), "Gsamples/s %.3f" % (W * H * spp / min(t) / 1e6), "big", f["big"], "ext", f["ext"],
      "triangle family", int(r.kernel_triangles()), "table", int(on), "hash", p.lib().rt_source_hash().decode()[:12], flush=True)
r.close()
'''


def child(tree, **env):
    e = dict(os.environ, **env)
    e.pop("RT06_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], env=e, cwd=tree, capture_output=True, text=True, timeout=200)
    if res.returncode != 0:
        sys.exit(f"child failed in {tree}: rc {res.returncode}\n{res.stderr[-600:]}")   # nothing more is started on the GPU
    return " |".join(l.strip() for l in res.stdout.strip().splitlines() if not l.startswith("/opt/"))


sys.path.insert(0, ROOT)
import __graft_entry__ as G
print("source", G.load_package().lib().rt_source_hash().decode(), flush=True)
if "existing" in a.sections:
    for wl in ("cornell_ico", "book2_final", "book1_final"):
        for rnd in range(1, a.rounds + 1):
            for name, tree in trees:
                print("existing", wl, "round", rnd, name, child(tree, SN_WORKLOAD=wl, SN_LEVEL="5", SN_SMOOTH="0"), flush=True)
if "table" in a.sections:
    for level in (3, 5):
        for rnd in range(1, a.rounds + 1):
            for smooth in ("0", "1"):
                print("table icosphere", level, "round", rnd, "smooth" if smooth == "1" else "flat", child(ROOT, SN_WORKLOAD="cornell_ico", SN_LEVEL=str(level), SN_SMOOTH=smooth), flush=True)
