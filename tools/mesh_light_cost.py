#!/usr/bin/env python3
"""What sampling triangle and mesh lights buys and costs (EXPERIMENTS.md E10), one GPU, one JSON line per measurement; E8's protocol (HIP-event kernel times).

The room is the Cornell box of "The Next Week" without its ceiling light (5 walls, two rotated boxes), median-split BVH, 600x600, depth 50.

  * noise: the room lit only by an emissive icosphere(0) (20 triangles), and only by an emissive tetrahedron: the noise figure (rt_renderer_refine_noise) after
    16, 64, 256 and 1024 samples with sampling off and in mode RT_LIGHT_SAMPLING_MESH, with the milliseconds of the refine steps so far;
  * target: the off-mode's noise figure at --target-spp samples, and the samples / milliseconds mode 4 needs to get below it (steps of 64): equal noise,
    compared in time;
  * loop: the dominant kernel's time per refine step of 64 samples with n_l = 1, 4, 16, 20 and 64 triangle lights — one 130 x 105 panel under the ceiling cut
    into n_l triangles, so the lit area stays what it is — in mode 4, against mode 2 on the same room with one sphere lamp (and mode 4 on that, whose table is
    mode 2's), median of --repeats steps after a warm-up;
  * existing: the same figure for mode 1 on Scene.cornell_box() and mode 2 on Scene.cornell_lamp(), to be run once per library (RT06_LIB) and compared.

    python tools/mesh_light_cost.py [--sections noise,target,loop,existing] [--repeats 9] [--target-spp 2048]
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--target-spp", type=int, default=2048)
ap.add_argument("--sections", default="noise,target,loop,existing")
a = ap.parse_args()
sections = set(a.sections.split(","))
p = G.load_package()
from ray_tracing_v06_amd import mesh_io

W = H = 600
CAM = p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)


def room(lights):
    """the Cornell box without its light, and what lights(s, emit) adds"""
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


def mesh_lamp(which):
    def lights(s):
        v, f = mesh_io.icosphere(0) if which == "icosphere" else mesh_io.tetrahedron()
        s.MakeMesh(v, f, s.DiffuseLight((40, 40, 40)), 40.0, 0.0, (278, 470, 278))   # where Scene.cornell_lamp() hangs its sphere of radius 40
    return lights


def panel(n):
    """the Cornell box's 130 x 105 light panel at y = 554 as n triangles: n = 1 the half below the diagonal; otherwise n / 2 strips of two triangles"""
    def lights(s):
        emit = s.DiffuseLight((15, 15, 15))
        x0, z0, dx, dz = 213.0, 227.0, 130.0, 105.0
        if n == 1:
            s.MakeTriangle((x0, 554, z0), (x0 + dx, 554, z0), (x0, 554, z0 + dz), emit)
            return
        k = n // 2
        for i in range(k):
            xa, xb = x0 + dx * i / k, x0 + dx * (i + 1) / k
            s.MakeTriangle((xa, 554, z0), (xb, 554, z0), (xa, 554, z0 + dz), emit)
            s.MakeTriangle((xb, 554, z0 + dz), (xa, 554, z0 + dz), (xb, 554, z0), emit)
    return lights


def sphere_lamp(s):
    s.MakeSphere((278, 470, 278), 40.0, s.DiffuseLight((40, 40, 40)))


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
    r.close()
    return round(statistics.median(dom), 4), round(max(dom) - min(dom), 4)


for which in (("icosphere", "tetrahedron") if sections & {"noise", "target"} else ()):
    scene = room(mesh_lamp(which))
    if "noise" in sections:
        for mode in (0, 4):
            r = renderer(scene, 64, mode)
            done, ms = 0, 0.0
            for upto in (16, 64, 256, 1024):
                while done < upto:
                    n = min(64, upto - done)
                    r.refine(n)
                    ms += r.last_kernel_ms()
                    done += n
                print(json.dumps({"room": which, "section": "noise", "mode": mode, "lights": r.light_sampling_info()["lights"], "samples": done,
                                  "noise": round(r.noise(), 5), "ms": round(ms, 2)}), flush=True)
            r.close()
    if "target" in sections:
        r = renderer(scene, 256, 0)
        ms = 0.0
        for _ in range(a.target_spp // 256):
            r.refine(256)
            ms += r.last_kernel_ms()
        target = r.noise()
        print(json.dumps({"room": which, "section": "target", "mode": 0, "samples": r.refine_info()["samples"], "noise": round(target, 6), "ms": round(ms, 1)}), flush=True)
        r.close()
        r = renderer(scene, 64, 4)
        ms, noise = 0.0, float("inf")
        while noise > target and r.refine_info()["samples"] < 2 * a.target_spp:
            r.refine(64)
            ms += r.last_kernel_ms()
            noise = r.noise()
        print(json.dumps({"room": which, "section": "target", "mode": 4, "samples": r.refine_info()["samples"], "noise": round(noise, 6), "ms": round(ms, 1)}), flush=True)
        r.close()

if "loop" in sections:
    lamp = room(sphere_lamp)
    for mode in (0, 2, 4):
        med, spread = step_ms(lamp, mode)
        print(json.dumps({"section": "loop", "room": "sphere lamp", "mode": mode, "lights": 1, "dominant_ms": med, "spread_ms": spread}), flush=True)
    for n in (1, 4, 16, 20, 64):
        scene = room(panel(n))
        for mode in (0, 4):
            med, spread = step_ms(scene, mode)
            print(json.dumps({"section": "loop", "room": "panel", "mode": mode, "lights": n, "dominant_ms": med, "spread_ms": spread}), flush=True)

if "existing" in sections:
    for which, mode in (("cornell_box", 1), ("cornell_lamp", 2), ("cornell_box", 0)):
        med, spread = step_ms(getattr(p.Scene, which)(), mode)
        print(json.dumps({"section": "existing", "library": os.environ.get("RT06_LIB", "librt06.so"), "built_from": p.capi.library_hash()[:12], "scene": which, "mode": mode,
                          "dominant_ms": med, "spread_ms": spread}), flush=True)
