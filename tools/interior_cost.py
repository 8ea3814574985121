#!/usr/bin/env python3
"""What solid glass costs (EXPERIMENTS.md E26).  One GPU.  Sections, any subset of:

    python tools/interior_cost.py --parent DIR ab     # DIR: a built checkout of the commit to compare with
    python tools/interior_cost.py solid               # this tree only

  ab     the rule went into sixteen NEW forms, so every world without an interior table runs the kernel it ran and must cost what it cost: §29's recorded test
         room (tests/_mfac_worlds.room, table on) plain and under light-sampling mode 48 at 600 x 400, 32 spp, and an unrecorded world
         (tests/_tri_worlds.tri_room(textured=True) at 600 x 400, 32 spp), depth 50, this tree against the parent in alternating rounds, nine by default, each
         round of each tree in a process of its own (tools/rough_glass_cost.py's method); dominant-kernel HIP-event time, best, median and worst of 7 renders.
         The last lines are, per world, the median over the rounds of each tree's medians, their ratio, and the parent's own round-to-round spread.
  solid  the solid-glass test room (tests/_interior_worlds.room) at a user's size, 400 x 400 at 256 spp, depth 50, in this tree, three ways on one renderer, twice
         over: on the INTR form with its records (`solid`), on the INTR form with every record off (`off`: what carrying the rule costs), on the MFAC form
         without the table (`none`); then the same under mode 48.  solid - off is what the facing's other paths and the exponentials cost.
Every line starts with its section's name."""
import argparse, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["solid"])
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
import _mfac_worlds as MW
import _tri_worlds as TW
W, H = 600, 400
for mode in (0, 48):
    scene = MW.room(p, env=bool(mode))
    r = p.Renderer.MakeRenderer(W, H, 32, 50, MW.camera(p, W, H), scene.getWorldPtr())
    if mode:
        r.light_sampling(mode)
    assert r.kernel_microfacet()
    print("ab", sys.argv[1], "room_mode%d" % mode, timed(r), flush=True)
    r.close()
scene = TW.tri_room(p, textured=True)
r = p.Renderer.MakeRenderer(W, H, 32, 50, TW.camera(p, W, H), scene.getWorldPtr())
print("ab", sys.argv[1], "tri_room", timed(r), flush=True)
r.close()
'''

SOLID = COMMON + r'''
import _interior_worlds as IW
W, H = 400, 400
print("solid", p.lib().rt_source_hash().decode(), flush=True)
for mode in (0, 48):
    scene = IW.room(p, env=bool(mode))
    table = scene.interiors()
    r = p.Renderer.MakeRenderer(W, H, 256, 50, IW.camera(p, IW.OUTSIDE, W, H), scene.getWorldPtr())
    if mode:
        r.light_sampling(mode)
    for rnd in range(2):
        for name, t in (("solid", table), ("off", IW.all_off(table)), ("none", None)):
            r.interiors(t)
            assert r.kernel_interior() == (t is not None) and r.kernel_microfacet()
            print("solid", "mode %d" % mode, name, timed(r, 5), flush=True)
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
if "solid" in a.sections:
    subprocess.run([sys.executable, "-c", SOLID], cwd=ROOT, check=True, timeout=900)
