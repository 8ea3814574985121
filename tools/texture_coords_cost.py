#!/usr/bin/env python3
"""What texture coordinates cost and what they buy (EXPERIMENTS.md E14).  One GPU.  Sections, any subset of:

    python tools/texture_coords_cost.py keys earth                 # this tree only
    python tools/texture_coords_cost.py --parent DIR keys          # DIR: a built checkout of the commit to compare with

  keys   the eight TRI && EXT 2 kernels (tests/_tri_worlds.FORMS) on tri_room(textured=True), 600 x 400, 32 spp, depth 50: dominant-kernel HIP-event time,
         best and mean of 5 renders, without a table and — this tree — with a table of random coordinates on; once per tree and round, alternating, each
         round in a process of its own
  earth  the Book-2 planet image on an analytic sphere and on uv_sphere(64, 32) with its own coordinates and normals, 400 x 400, 64 spp, depth 50:
         time per frame and the RMS difference of the two frames
Every line starts with its section's name; the first line is the library's rt_source_hash."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["keys"])
ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare with (section keys)")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]

KEYS = r'''
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import __graft_entry__ as G
import _tri_worlds as TW
p = G.load_package()
W, H, spp = 600, 400, 32
for form in [f for f in TW.FORMS if f[2] == 2]:
    variant, env = TW.FORMS[form]
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE"):
        os.environ.pop(k, None)
    os.environ.update(env)
    s = TW.tri_room(p, textured=True, as_list=form[0] == TW.LIST)
    r = p.Renderer.MakeRenderer(W, H, spp, 50, TW.camera(p, W, H), s.getWorldPtr(), variant=variant)
    assert r.kernel_form() == TW.kernel_form_of(form) and r.kernel_triangles()
    cases = ["none"] + (["table"] if hasattr(r, "texture_coords") else [])
    for case in cases:
        if case == "table":
            n = s.n_triangles()
            r.texture_coords((np.random.default_rng(1).random((n, 6), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)))
        r.Render()
        t = []
        for _ in range(5):
            r.Render()
            t.append(r.kernel_times()[1])
        print(TW.form_id(form), case, "dominant kernel ms best %.3f mean %.3f" % (min(t), sum(t) / len(t)), "hash", p.lib().rt_source_hash().decode()[:12], flush=True)
    r.close()
'''

EARTH = r'''
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import __graft_entry__ as G
p = G.load_package()
from ray_tracing_v06_amd import mesh_io
W = H = 400
spp = 64
img = p.Scene.book2_final(1984).image().copy()
cam = p.PinholeCamera((0, 1.2, 6.5), (0, 0, 0), (0, 1, 0), 40.0, 1.0)
frames = {}
for name in ("sphere", "uv_sphere(64, 32)"):
    s = p.Scene()
    s.set_image(img)
    s.set_background((0.7, 0.8, 1.0))
    s.MakeQuad((-8, -2, -8), (16, 0, 0), (0, 0, 16), s.Lambertian((0.5, 0.5, 0.5)))
    if name == "sphere":
        s.MakeSphere((0, 0, 0), 2.0, s.ImageTexture())
    else:
        v, f, n, t = mesh_io.uv_sphere(64, 32)
        s.MakeMesh(v, f, s.ImageTexture(), 2.0, 0.0, (0, 0, 0), normals=n, uvs=t)
    s.BuildBVH_SAH()
    r = p.Renderer.MakeRenderer(W, H, spp, 50, cam, s.getWorldPtr())
    r.Render()
    t = []
    for _ in range(5):
        r.Render()
        t.append(r.kernel_times()[1])
    frames[name] = r.DownloadRenderbuffer()[..., :3].astype(np.float64)
    print(name, "dominant kernel ms best %.3f mean %.3f" % (min(t), sum(t) / len(t)), "kernel", r.kernel_form(), flush=True)
    r.close()
a, b = frames["sphere"], frames["uv_sphere(64, 32)"]
print("RMS difference, whole frame %.5f" % np.sqrt(((a - b) ** 2).mean()), "| mean of the sphere's frame %.5f" % a.mean(), flush=True)
'''


def child(code, tree):
    e = dict(os.environ)
    e.pop("RT06_LIB", None)
    res = subprocess.run([sys.executable, "-c", code], env=e, cwd=tree, capture_output=True, text=True, timeout=280)
    if res.returncode != 0:
        sys.exit(f"child failed in {tree}: rc {res.returncode}\n{res.stderr[-800:]}")   # nothing more is started on the GPU
    return [l.strip() for l in res.stdout.strip().splitlines() if not l.startswith("/opt/")]


sys.path.insert(0, ROOT)
import __graft_entry__ as G
print("source", G.load_package().lib().rt_source_hash().decode(), flush=True)
if "keys" in a.sections:
    for rnd in range(1, a.rounds + 1):
        for name, tree in trees:
            for line in child(KEYS, tree):
                print("keys round", rnd, name, line, flush=True)
if "earth" in a.sections:
    for line in child(EARTH, ROOT):
        print("earth", line, flush=True)
