#!/usr/bin/env python3
"""What microfacet surfaces cost (EXPERIMENTS.md E24).  One GPU.  Sections, any subset of:

    python tools/microfacet_cost.py --parent DIR off   # DIR: a built checkout of the commit to compare with
    python tools/microfacet_cost.py on                 # this tree only

  off  no microfacet table, this tree against the parent, alternating, each round in a process of its own: BASELINE config 4's scene (Book-2 final, the
       global-memory form) at 960 x 540, 32 spp, and an LDS-resident EXT 2 world (tests/_tri_worlds.tri_room(textured=True)) at 600 x 400, 32 spp; depth 50;
       dominant-kernel HIP-event time, best, median and worst of 7 renders
  on   the microfacet test room (tests/_mfac_worlds.room: §28's room with a coated floor, two rough conductors, a coated mesh under a roughness map and a normal
       map, glass, inside a coated shell) at 600 x 400, 32 spp, depth 50, in this tree: the table off (the normal-map kernel the parent runs), on, off and on
       again, alternating on one renderer; then the same under light-sampling mode 48
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["on"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (section off)")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]

COMMON = r'''
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import __graft_entry__ as G
p = G.load_package()


def timed(r, n=7):
    r.Render()
    t = []
    for _ in range(n):
        r.Render(); t.append(r.kernel_times()[1])
    return "best %.3f median %.3f worst %.3f ms" % (min(t), float(np.median(t)), max(t))
'''

OFF = COMMON + r'''
import _tri_worlds as TW
W, H = 960, 540
scene = p.Scene.book2_final(1984)   # (kept alive: the flat world borrows its arrays)
r = p.Renderer.MakeRenderer(W, H, 32, 50, p.MotionBlurCamera((478, 278, -600), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 1.0), scene.getWorldPtr())
print("off", sys.argv[1], "book2_final", r.kernel_form(), timed(r), flush=True)
r.close()
W, H = 600, 400
scene = TW.tri_room(p, textured=True)
r = p.Renderer.MakeRenderer(W, H, 32, 50, TW.camera(p, W, H), scene.getWorldPtr())
print("off", sys.argv[1], "tri_room", r.kernel_form(), timed(r), flush=True)
r.close()
'''

ON = COMMON + r'''
import _mfac_worlds as MW
W, H = 600, 400
print("on", p.lib().rt_source_hash().decode(), flush=True)
for mode in (0, 48):
    scene = MW.room(p, env=bool(mode))
    table = scene.microfacets()
    r = p.Renderer.MakeRenderer(W, H, 32, 50, MW.camera(p, W, H), scene.getWorldPtr())
    if mode:
        r.light_sampling(mode)
    for rnd in range(2):
        for name, t in (("table off", None), ("table on", table)):
            r.microfacets(t)
            print("on", "mode %d" % mode, name, "mfac kernel" if r.kernel_microfacet() else "nmap kernel" if r.kernel_normal_map() else "plain kernel", timed(r), flush=True)
    r.close()
'''

if "off" in a.sections:
    for rnd in range(a.rounds):
        for name, tree in trees:
            subprocess.run([sys.executable, "-c", OFF, name], cwd=tree, check=True, timeout=600)
if "on" in a.sections:
    subprocess.run([sys.executable, "-c", ON], cwd=ROOT, check=True, timeout=600)
