#!/usr/bin/env python3
"""What the texture table costs (EXPERIMENTS.md E17).  One GPU.  Sections, any subset of:

    python tools/textures_cost.py --parent DIR off      # DIR: a built checkout of the commit to compare with
    python tools/textures_cost.py on                    # this tree only

  off  the table off, this tree against the parent, alternating, each round in a process of its own: BASELINE config 4's scene (Book-2 final, the global-memory
       form, the earth image) at 960 x 540, 32 spp, and an LDS-resident EXT 2 world (tests/_tri_worlds.tri_room(textured=True)) at 600 x 400, 32 spp; depth 50;
       dominant-kernel HIP-event time, best, median and worst of 7 renders
  on   the same two worlds in this tree: no table; a one-entry clamp / nearest table; that entry bilinear; three images (the world's, and two more on two spheres
       added to the world, one repeat / bilinear)
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
import _tri_worlds as TW
p = G.load_package()


def worlds(extra):
    """(name, scene, camera, W, H): extra(s, name) may add to a world before it is built"""
    W, H = 960, 540
    s = p.Scene.book2_final(1984)
    if extra(s, "book2_final"):
        s.BuildBVH_TopDown()
    yield "book2_final", s, p.MotionBlurCamera((478, 278, -600), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 1.0), W, H
    W, H = 600, 400
    yield "tri_room", TW.tri_room(p, textured=True, more=lambda s: extra(s, "tri_room")), TW.camera(p, W, H), W, H


def timed(r, label):
    r.Render()
    t = []
    for _ in range(7):
        r.Render()
        t.append(r.kernel_times()[1])
    t.sort()
    print(label, "dominant kernel ms best %.3f median %.3f worst %.3f" % (t[0], t[3], t[6]), "big", r.kernel_form()["big"], "hash", p.lib().rt_source_hash().decode()[:12], flush=True)
'''

OFF = COMMON + r'''
for name, s, cam, W, H in worlds(lambda s, name: False):
    r = p.Renderer.MakeRenderer(W, H, 32, 50, cam, s.getWorldPtr())
    timed(r, name + " table off")
    r.close()
'''

ON = COMMON + r'''
rng = np.random.default_rng(3)
for name, s, cam, W, H in worlds(lambda s, name: False):
    r = p.Renderer.MakeRenderer(W, H, 32, 50, cam, s.getWorldPtr())
    timed(r, name + " no table")
    rec, tex = s.textures()
    r.textures((rec, tex))
    timed(r, name + " one entry clamp/nearest")
    rec["filter"][0] = 1
    r.textures((rec, tex))
    timed(r, name + " one entry clamp/bilinear")
    r.close()


def two_more(s, name):
    a = s.add_image(rng.integers(0, 256, (64, 128, 3)).astype(np.uint8), "repeat", "bilinear")
    b = s.add_image(rng.integers(0, 256, (37, 53, 3)).astype(np.uint8), "clamp", "nearest")
    at = ((200, 320, 250), (330, 330, 150), 45.0) if name == "book2_final" else ((2.5, 6.5, 6.5), (7.5, 6.0, 7.0), 1.0)
    s.MakeSphere(at[0], at[2], s.ImageTexture(a))
    s.MakeSphere(at[1], at[2], s.ImageTexture(b))
    return True


for name, s, cam, W, H in worlds(two_more):
    r = p.Renderer.MakeRenderer(W, H, 32, 50, cam, s.getWorldPtr())
    assert r.textures_info() == {"enabled": True, "entries": 3}
    timed(r, name + " plus two spheres, three images")
    r.close()
'''


def child(code, tree):
    e = dict(os.environ)
    e.pop("RT06_LIB", None)
    res = subprocess.run([sys.executable, "-c", code], env=e, cwd=tree, capture_output=True, text=True, timeout=200)
    if res.returncode != 0:
        sys.exit(f"child failed in {tree}: rc {res.returncode}\n{res.stderr[-800:]}")   # nothing more is started on the GPU
    return [l.strip() for l in res.stdout.strip().splitlines() if not l.startswith("/opt/")]


sys.path.insert(0, ROOT)
import __graft_entry__ as G
print("source", G.load_package().lib().rt_source_hash().decode(), flush=True)
if "off" in a.sections:
    for rnd in range(1, a.rounds + 1):
        for name, tree in trees:
            for line in child(OFF, tree):
                print("off round", rnd, name, line, flush=True)
if "on" in a.sections:
    for line in child(ON, ROOT):
        print("on", line, flush=True)
