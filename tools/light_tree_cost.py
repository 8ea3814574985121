#!/usr/bin/env python3
"""What the light tree and the choice by area buy and cost (EXPERIMENTS.md E11), one GPU, one JSON line per measurement; E10's protocol and rooms
(tools/mesh_light_cost.py: the Cornell box without its ceiling light, median-split BVH, 600x600, depth 50, HIP-event kernel times).

  * cost: the dominant kernel's time per refine step of 64 samples on the panel room — one 130 x 105 panel under the ceiling cut into n_l triangles — at
    n_l = 1, 4, 16, 20, 64 with sampling off, in mode 4 (the linear loop) and in mode 16 (the tree), and at n_l = 256, 1024 off and in mode 16; median and
    spread (max - min) of --repeats steps after a warm-up;
  * noise: the room lit only by an emissive icosphere(2) (320 triangles) and icosphere(3) (1280): the noise figure (rt_renderer_refine_noise) after 16, 64, 256
    and 1024 samples off and in mode 16, with the milliseconds of the refine steps so far — equal samples and equal time are read off the two columns;
  * mixed: the panel (2 triangles) beside an icosphere(2): the same in mode 16, and the share of the light draws the panel gets by area (mode 16) and would
    get by count (mode 4's rule: 2 / n_l), from the host's table;
  * existing: mode 1 on Scene.cornell_box(), mode 2 on Scene.cornell_lamp(), mode 4 on the 20-triangle panel and the plain Cornell box, to be run once per
    library (RT06_LIB) and compared.

    python tools/light_tree_cost.py [--sections cost,noise,mixed,existing] [--repeats 9]
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--sections", default="cost,noise,mixed,existing")
a = ap.parse_args()
sections = set(a.sections.split(","))
p = G.load_package()
from ray_tracing_v06_amd import mesh_io

W = H = 600
CAM = p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)


def room(lights):
    """the Cornell box without its light, and what lights(s) adds (tools/mesh_light_cost.py's room)"""
    s = p.Scene()
    red, white, green = s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.12, 0.45, 0.15))
    s.MakeQuad((555, 0, 0), (0, 555, 0), (0, 0, 555), green)
    s.MakeQuad((0, 0, 0), (0, 555, 0), (0, 0, 555), red)
    s.MakeQuad((0, 0, 0), (555, 0, 0), (0, 0, 555), white)
    s.MakeQuad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white)
    s.MakeQuad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)
    s.MakeBox((0, 0, 0), (165, 330, 165), white, 15.0, (265, 0, 295))
    s.MakeBox((0, 0, 0), (165, 165, 165), white, -18.0, (130, 0, 65))
    lights(s)
    s.set_background((0, 0, 0))
    s.BuildBVH_TopDown()
    return s


def panel(n, x0=213.0, z0=227.0):
    """the 130 x 105 light panel at y = 554 as n triangles: n = 1 the half below the diagonal; otherwise a grid of n / 2 cells of two triangles (strips up to 64,
    as in E10; finer panels are cut both ways so that no triangle is a sliver)"""
    def lights(s):
        emit = s.DiffuseLight((15, 15, 15))
        dx, dz = 130.0, 105.0
        if n == 1:
            s.MakeTriangle((x0, 554, z0), (x0 + dx, 554, z0), (x0, 554, z0 + dz), emit)
            return
        k = n // 2
        rows = 1 if n <= 64 else (8 if n <= 256 else 16)
        cols = k // rows
        for j in range(rows):
            za, zb = z0 + dz * j / rows, z0 + dz * (j + 1) / rows
            for i in range(cols):
                xa, xb = x0 + dx * i / cols, x0 + dx * (i + 1) / cols
                s.MakeTriangle((xa, 554, za), (xb, 554, za), (xa, 554, zb), emit)
                s.MakeTriangle((xb, 554, zb), (xa, 554, zb), (xb, 554, za), emit)
    return lights


def icosphere_lamp(level):
    def lights(s):
        s.MakeMesh(*mesh_io.icosphere(level), s.DiffuseLight((40, 40, 40)), 40.0, 0.0, (278, 470, 278))
    return lights


def mixed(s):
    panel(2, x0=60.0, z0=300.0)(s)
    icosphere_lamp(2)(s)


def renderer(scene, spp, mode):
    r = p.Renderer.MakeRenderer(W, H, spp, 50, CAM, scene.getWorldPtr())
    if mode:
        r.light_sampling(mode)
    return r


def step_ms(scene, mode):
    r = renderer(scene, 64, mode)
    r.refine(64)   # warm-up
    dom = []
    for _ in range(a.repeats):
        r.refine(64)
        dom.append(r.kernel_times(0)[1])
    info = r.kernel_info()
    r.close()
    return round(statistics.median(dom), 4), round(max(dom) - min(dom), 4), info["workgroups_per_cu"]


def noise_rows(name, scene, modes):
    for mode in modes:
        r = renderer(scene, 64, mode)
        done, ms = 0, 0.0
        for upto in (16, 64, 256, 1024):
            while done < upto:
                n = min(64, upto - done)
                r.refine(n)
                ms += r.last_kernel_ms()
                done += n
            print(json.dumps({"room": name, "section": "noise", "mode": mode, "lights": r.light_sampling_info()["lights"] if mode else 0, "samples": done,
                              "noise": round(r.noise(), 5), "ms": round(ms, 2)}), flush=True)
        r.close()


print(json.dumps({"section": "library", "library": os.environ.get("RT06_LIB", "librt06.so"), "built_from": p.capi.library_hash()[:12]}), flush=True)
if "cost" in sections:
    for n in (1, 4, 16, 20, 64, 256, 1024):
        scene = room(panel(n))
        for mode in ((0, 4, 16) if n <= 64 else (0, 16)):
            try:
                med, spread, wg = step_ms(scene, mode)
                print(json.dumps({"section": "cost", "room": "panel", "mode": mode, "lights": n, "dominant_ms": med, "spread_ms": spread, "workgroups_per_cu": wg}), flush=True)
            except p.capi.RtError as e:
                print(json.dumps({"section": "cost", "room": "panel", "mode": mode, "lights": n, "refused": str(e)}), flush=True)

if "noise" in sections:
    for level in (2, 3):
        noise_rows(f"icosphere({level})", room(icosphere_lamp(level)), (0, 16))

if "mixed" in sections:
    scene = room(mixed)
    kind, index, area = scene.light_table("tree")
    quads = scene.quads()
    on_panel = [i for i in range(len(index)) if abs(float(quads["Q"][index[i]][1]) - 554.0) < 1e-3 and abs(float(quads["u"][index[i]][1])) < 1e-6 and abs(float(quads["v"][index[i]][1])) < 1e-6]
    print(json.dumps({"section": "mixed", "lights": len(index), "panel_lights": len(on_panel), "panel_share_by_area": round(float(area[on_panel].sum() / area.sum()), 5),
                      "panel_share_by_count": round(len(on_panel) / len(index), 5)}), flush=True)
    noise_rows("panel + icosphere(2)", scene, (0, 16))

if "existing" in sections:
    for which, mode in (("cornell_box", 1), ("cornell_lamp", 2), ("panel20", 4), ("cornell_box", 0)):
        scene = room(panel(20)) if which == "panel20" else getattr(p.Scene, which)()
        med, spread, _ = step_ms(scene, mode)
        print(json.dumps({"section": "existing", "library": os.environ.get("RT06_LIB", "librt06.so"), "built_from": p.capi.library_hash()[:12], "scene": which, "mode": mode,
                          "dominant_ms": med, "spread_ms": spread}), flush=True)
