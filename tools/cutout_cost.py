#!/usr/bin/env python3
"""What alpha cutouts cost (EXPERIMENTS.md E27).  One GPU.  Sections, any subset of:

    python tools/cutout_cost.py --parent DIR ab      # DIR: a built checkout of the commit to compare with
    python tools/cutout_cost.py room                 # this tree only

  ab    the rule went into sixteen NEW forms, so every world without a cutout table runs the kernel it ran and must cost what it cost: §32's solid-glass test
        room (tests/_interior_worlds.room, table on: an INTR form) and an unrecorded world (tests/_tri_worlds.tri_room(textured=True)), both at 600 x 400, 32 spp,
        depth 50, this tree against the parent in alternating rounds, each round of each tree in a process of its own (tools/interior_cost.py's method);
        dominant-kernel HIP-event time, best, median and worst of 7 renders.  The last lines are, per world, the median over the rounds of each tree's medians,
        their ratio, and the parent's own round-to-round spread.
  room  the cutout test room (tests/_cutout_worlds.room) at 400 x 400, 256 spp, depth 50, in this tree, four ways on one renderer, twice over, all four under
        the same interior table whose records are all off, so that the cutout table is the only difference: on the INTR form without the cutout table (`intr`:
        the interior table puts the renderer there), on the CUT form with every record off (`off`: what carrying the rule costs), on the CUT form with an opaque
        mask on every material (`opaque`: what the lookups cost, the frame unchanged), and on the CUT form with the room's masks (`masks`: another frame — rays
        go on through the holes); then the same under mode 48.
Every line starts with its section's name."""
import argparse, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["room"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (section ab)")
ap.add_argument("--rounds", type=int, default=9)
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

AB = COMMON + r'''
import _interior_worlds as IW
import _tri_worlds as TW
W, H = 600, 400
scene = IW.room(p)
r = p.Renderer.MakeRenderer(W, H, 32, 50, IW.camera(p, IW.OUTSIDE, W, H), scene.getWorldPtr())
assert r.kernel_interior()
print("ab", sys.argv[1], "solid_room", timed(r), flush=True)
r.close()
scene = TW.tri_room(p, textured=True)
r = p.Renderer.MakeRenderer(W, H, 32, 50, TW.camera(p, W, H), scene.getWorldPtr())
print("ab", sys.argv[1], "tri_room", timed(r), flush=True)
r.close()
'''

ROOM = COMMON + r'''
import _cutout_worlds as CW
W, H = 400, 400
print("room", p.lib().rt_source_hash().decode(), flush=True)
for mode in (0, 48):
    scene = CW.room(p, env=bool(mode))
    masks = scene.cutouts()
    opaque = CW.all_of(p, scene, scene.names["images"]["white"])
    none = np.zeros(len(masks), p.capi.CUTOUT_DT)
    world = scene.getWorldPtr()
    del world.cutouts
    r = p.Renderer.MakeRenderer(W, H, 256, 50, CW.camera(p, W, H), world)
    if mode:
        r.light_sampling(mode)
    r.interiors(np.zeros(len(masks), p.capi.INTERIOR_DT))
    for rnd in range(2):
        for name, cut in (("intr", None), ("off", none), ("opaque", opaque), ("masks", masks)):
            r.cutouts(cut)
            assert r.kernel_cutout() == (cut is not None) and r.kernel_interior() and r.interiors_info() == {"enabled": True, "records": 0}
            print("room", "mode %d" % mode, name, timed(r, 5), flush=True)
    r.close()
'''

if "ab" in a.sections:
    medians = {}
    for rnd in range(a.rounds):
        for name, tree in trees:
            out = subprocess.run([sys.executable, "-c", AB, name], cwd=tree, check=True, timeout=600, stdout=subprocess.PIPE, text=True).stdout
            sys.stdout.write(out)
            sys.stdout.flush()
            for tree_name, world, median in re.findall(r"^ab (\w+) (\w+) best [\d.]+ median ([\d.]+)", out, re.M):
                medians.setdefault(world, {}).setdefault(tree_name, []).append(float(median))
    for world, by_tree in medians.items():
        mid = {t: sorted(v)[len(v) // 2] for t, v in by_tree.items()}
        line = "ab summary %s: " % world + ", ".join("%s %.3f ms" % (t, m) for t, m in mid.items())
        if "parent" in mid:
            v = by_tree["parent"]
            line += "; this / parent %.4f; the parent's spread over its rounds %.4f, this tree's %.4f" % (
                mid["this"] / mid["parent"], (max(v) - min(v)) / mid["parent"], (max(by_tree["this"]) - min(by_tree["this"])) / mid["this"])
        print(line, flush=True)
if "room" in a.sections:
    subprocess.run([sys.executable, "-c", ROOM], cwd=ROOT, check=True, timeout=900)
