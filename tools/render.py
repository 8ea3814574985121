#!/usr/bin/env python3
"""Command-line caller of the path — what FirstApp::MakeApp / Run hard-code (main/src/FirstApp.cpp:20-56,94-106):

    python tools/render.py --scene book1_final --width 1200 --height 800 --spp 500 --depth 50 --out out.png

Scenes: book1_final (DefocusBlurCamera vfov 20, aperture 0.1), book2_moving (MotionBlurCamera t in [0,1]),
three_spheres (PinholeCamera vfov 90).  Prints one JSON line with the render time and Msamples/s.

    python tools/render.py --scene book1_final --spp 500 --refine 50 --until 0.01 --out out.png

renders progressively (rt_renderer_refine): steps of 50 samples up to --spp, one line per step with the samples so far and the noise
figure (relative RMS standard error of the frame's mean luminance), stopping early once it is below --until.  The image written is the
last refined frame: bit for bit the frame a one-shot render at that sample count gives.

    python tools/render.py --scene cornell_box --spp 64 --refine 8 --until 0.05 --denoise --aov feat --out out.png

also accumulates first-hit feature buffers (rt_renderer_aov_enable) while refining.  --denoise writes the edge-aware filtered frame
(rt_renderer_denoise) next to the refined one, as out_denoised.png; --aov PREFIX writes PREFIX_normal.png (n * 0.5 + 0.5),
PREFIX_depth.png (nearest white, misses black) and PREFIX_albedo.png.  One GPU; a world with a noise or an image texture takes the textured
feature mode (rt_renderer_aov_enable_mode, DESIGN.md §27: the albedo is the first hit's marble or texel), one with alpha cutouts or a constant medium the full mode
(§35: the feature trace is the colour path's first trace, masks and the medium's draws included).

    python tools/render.py --scene cornell_box --spp 64 --light-sampling --out out.png

samples the world's quad lights at every Lambertian hit (rt_renderer_light_sampling_enable): the same expected image from far fewer
samples where a small emitter lights the world.  Works with every mode above; refused for worlds without a quad light or with a medium.

    python tools/render.py --scene cornell_lamp --spp 64 --light-sampling-mode all --out out.png

samples sphere lights too (RT_LIGHT_SAMPLING_ALL): the Cornell box lit by a lamp, which has no quad light for --light-sampling to take.

    python tools/render.py --scene cornell_lamp --mesh icosphere:0 --mesh-scale 30 --mesh-translate 150,400,300 --mesh-material light \
        --spp 64 --light-sampling-mode mesh --out out.png

samples the triangles of an emissive mesh too (RT_LIGHT_SAMPLING_MESH), up to 64 lights of all kinds together.  --light-sampling-mode tree
(RT_LIGHT_SAMPLING_TREE) takes up to 4096 — e.g. --mesh icosphere:2 — picks a light by its area and finds the lights a direction crosses through a tree.

    python tools/render.py --scene cornell_box --mesh icosphere:2 --mesh-scale 80 --mesh-translate 278,278,200 --mesh-material metal --out out.png

places a triangle mesh — an OBJ file, icosphere:LEVEL or tetrahedron (ray-tracing-v06_amd/mesh_io.py) — into the prefab scene before its BVH is
built again (rt_scene_add_mesh): scaled, rotated about y (degrees), translated, in that order.  Materials: white, red, metal, glass, checker, light.

    python tools/render.py --scene book1_final --env sky --env-rotate 90 --env-scale 0.5 --out out.png

lights the world with an environment map (rt_scene_set_environment) in the place of its background: a Radiance .hdr picture, a float .npy array
(H, W, 3), an 8-bit .png / .ppm (mapped to [0, 1]) or `sky`, the procedural sky of image_io.sky_environment.  --env-rotate turns it about y (degrees),
--env-scale multiplies it on the host before upload.

    python tools/render.py --scene three_spheres --env sky --light-sampling-mode env --spp 64 --out out.png

draws half of every Lambertian hit's directions from the map itself, in proportion to radiance times solid angle (RT_LIGHT_SAMPLING_ENV): a small
bright sun is found at once instead of by the few rays that happen to leave towards it.  Needs --env.  `--light-sampling-mode env+tree` samples the map and the
world's lights together (RT_LIGHT_SAMPLING_ENV_TREE), and samples at image-textured hits, which no other mode does.

    python tools/render.py --scene book2_final --mesh tests/golden/tex_demo.obj --mtl --texture-wrap repeat --texture-filter bilinear \
        --mesh-scale 120 --mesh-translate 150,160,120 --spp 64 --out out.png

renders each `usemtl` group of the OBJ as a mesh of its own with the image its material's map_Kd names (the scene's texture table): here the
book's earth sphere (image 0), a floor whose `vt` run to 4 — tiled under --texture-wrap repeat — and a UV-mapped pyramid, both filtered bilinearly.  A material's
`Pm`, `Pr` and `map_Pr` are applied too: `Pm >= 0.5` makes the group a metal with `Kd` as F0; `Pr` or `map_Pr` gives it a microfacet record — a rough
conductor on the metal, a coat of specular 0.04 on anything else —, `map_Pr` scaling the roughness by the image's green channel.  A group whose `d` is below 0.5
(`Tr` above) or whose `illum` is 4, 6, 7 or 9 is glass of index `Ni`, whatever its `Pm`; `Pr` and `map_Pr` frost it.  --rough-glass R frosts the
prefab `glass` material of --mesh-material.  --solid-glass makes such glass solid where its faces close a volume: rays leave it as well as
enter it, and --glass-tint R,G,B --glass-tint-at D (or the material's `Tf`) colours it by thickness.

    python tools/render.py --scene book2_moving --camera perspective --aperture 0.3 --focus-dist 10 --shutter 0,1 --out out.png
    python tools/render.py --scene cornell_box --camera orthographic --camera-height 560 --out plan.png
    python tools/render.py --scene cornell_box --camera panorama --lookfrom 278,278,278 --lookat 279,278,278 --width 512 --height 256 --out probe.hdr
    python tools/render.py --scene three_spheres --env probe.hdr --out lit.png

replace the prefab camera by a lens camera: perspective (--camera-fov: the vertical field of view, default the prefab's), orthographic
(--camera-height: the window's height in world units), fisheye (--camera-fov: degrees across the image's height, default 180) or panorama (--camera-span H,V degrees,
default 360,180), each with an optional lens (--aperture, --focus-dist) and shutter (--shutter T0,T1), from --lookfrom towards --lookat (default: the prefab
camera's place and direction).  --out FILE.hdr or FILE.npy writes the LINEAR mean radiance (the refinement sums over the sample count, unclamped, no gamma), top
row first: a panorama looking along +x with +y up written this way loads as an --env map without a flip or a turn — a light probe of one scene lights another.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="book1_final", choices=["book1_final", "book2_moving", "three_spheres", "cornell_box", "cornell_lamp", "book2_final"])
ap.add_argument("--width", type=int, default=1200)
ap.add_argument("--height", type=int, default=800)
ap.add_argument("--spp", type=int, default=500)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--seed", type=int, default=1984)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--gpus", type=int, default=1, help="> 1: tile-shard the frame over GPUs 0..N-1 of this node from this one process (rt_multi_renderer_*, one RCCL exchange)")
ap.add_argument("--refine", type=int, default=0, metavar="STEP", help="render in steps of STEP samples up to --spp, printing samples and noise per step")
ap.add_argument("--until", type=float, default=None, metavar="NOISE", help="with --refine: stop once the noise figure is below NOISE (one GPU)")
ap.add_argument("--denoise", action="store_true", help="with --refine: also write the denoised frame (<out>_denoised.<ext>)")
ap.add_argument("--aov", default=None, metavar="PREFIX", help="with --refine: write PREFIX_normal.png, PREFIX_depth.png, PREFIX_albedo.png")
ap.add_argument("--light-sampling", action="store_true", help="next-event estimation over the world's quad lights (rt_renderer_light_sampling_enable)")
ap.add_argument("--light-sampling-mode", choices=["quads", "all", "mesh", "tree", "env", "env+tree"], default=None,
                help="switch light sampling on in this mode: quads (what --light-sampling selects), all (quad and sphere lights, e.g. --scene cornell_lamp) or "
                     "mesh (those and triangle lights, e.g. --mesh ... --mesh-material light), tree (mesh's lights, up to 4096, by area through a light tree), env (the environment map of --env alone, by radiance times solid angle), "
                     "env+tree (that map and tree's lights together, at image-textured hits too; a world without lights is taken as the map alone)")
ap.add_argument("--mesh", default=None, metavar="FILE.obj|icosphere:LEVEL|tetrahedron", help="a triangle mesh to place into the scene (rt_scene_add_mesh)")
ap.add_argument("--mesh-scale", type=float, default=1.0)
ap.add_argument("--mesh-rotate-y", type=float, default=0.0, metavar="DEGREES")
ap.add_argument("--mesh-translate", default="0,0,0", metavar="X,Y,Z")
ap.add_argument("--mesh-material", default="white", choices=["white", "red", "metal", "glass", "checker", "light"])
ap.add_argument("--smooth", action="store_true", help="with --mesh: smooth shading from per-vertex normals (DESIGN.md §21) — an OBJ file's own `vn` normals if it has a complete "
                    "set, an icosphere's unit positions, else area-weighted ones (mesh_io.vertex_normals)")
ap.add_argument("--texture", default=None, action="append", metavar="FILE.ppm|FILE.png", help="with --mesh FILE.obj: the mesh's material is this image over the file's `vt` texture "
                    "coordinates (DESIGN.md §22; binary PPM or 8-bit RGB / RGBA PNG); refused when the OBJ has no complete set of them.  With --mtl it may be repeated: "
                    "the k-th one replaces the map_Kd of the k-th material group, in the order the OBJ first uses them")
ap.add_argument("--mtl", action="store_true", help="with --mesh FILE.obj: one mesh per `usemtl` group, each with the image its material's map_Kd names (mtllib files beside the "
                    "OBJ; DESIGN.md §25) or a Lambertian of its Kd; a group without either takes --mesh-material")
ap.add_argument("--rough-glass", type=float, default=None, metavar="R", help="with --mesh-material glass: frost the glass, a GGX roughness in [0, 1] (DESIGN.md §30)")
ap.add_argument("--cutout-cutoff", type=float, default=0.5, metavar="X", help="with --mesh FILE.obj --mtl: a group whose material has a map_d, or an RGBA map_Kd, is there where the "
                "mask is not below X (alpha cutouts, DESIGN.md §34; default 0.5)")
ap.add_argument("--solid-glass", action="store_true", help="with --mesh: the transparent --mtl groups, or the prefab glass of --mesh-material, are solid glass (DESIGN.md §32): they "
                    "know inside from outside and tint with thickness.  A group is marked only when its faces close a volume and wind consistently (they are turned outward "
                    "if they wind inward); otherwise a warning, and the group stays the thin glass it was")
ap.add_argument("--glass-tint", default=None, metavar="R,G,B", help="with --solid-glass: the colour white light has after --glass-tint-at units of the glass (default: the material's "
                    "`Tf`, or none)")
ap.add_argument("--glass-tint-at", type=float, default=1.0, metavar="D", help="the thickness at which the glass shows --glass-tint")
ap.add_argument("--texture-wrap", choices=["clamp", "repeat"], default="clamp", help="the wrap mode of the images --texture / --mtl bring (DESIGN.md §25)")
ap.add_argument("--texture-filter", choices=["nearest", "bilinear"], default="nearest", help="their filter")
ap.add_argument("--env", default=None, metavar="FILE.hdr|FILE.npy|FILE.png|FILE.ppm|sky", help="an equirectangular environment map in the place of the scene's background "
                    "(DESIGN.md §23): Radiance RGBE, a float (H, W, 3) numpy array, an 8-bit picture (mapped to [0, 1]) or the procedural sky")
ap.add_argument("--env-rotate", type=float, default=0.0, metavar="DEG", help="with --env: turn the map about y")
ap.add_argument("--env-scale", type=float, default=1.0, metavar="X", help="with --env: multiply the map's radiance, on the host before upload")
ap.add_argument("--camera", choices=["perspective", "orthographic", "fisheye", "panorama"], default=None, help="a lens camera in the place of the prefab one (DESIGN.md §37)")
ap.add_argument("--camera-fov", type=float, default=None, metavar="DEG", help="perspective: the vertical field of view (default: the prefab camera's); fisheye: the angle across the image's height (default 180)")
ap.add_argument("--camera-height", type=float, default=None, metavar="H", help="orthographic: the view window's height in world units")
ap.add_argument("--camera-span", default="360,180", metavar="H,V", help="panorama: the horizontal and vertical span in degrees")
ap.add_argument("--aperture", type=float, default=0.0, metavar="A", help="with --camera: the lens diameter (0: no lens)")
ap.add_argument("--focus-dist", type=float, default=None, metavar="D", help="with --camera: the distance of the focus surface (default: from --lookfrom to --lookat)")
ap.add_argument("--shutter", default=None, metavar="T0,T1", help="with --camera: the shutter interval (default: none, every ray at time 0)")
ap.add_argument("--lookfrom", default=None, metavar="X,Y,Z", help="with --camera: the eye (default: the prefab camera's)")
ap.add_argument("--lookat", default=None, metavar="X,Y,Z", help="with --camera: the point looked at (default: one unit along the prefab camera's direction)")
ap.add_argument("--out", default="render.png", help="FILE.png / .ppm / .jpg: the frame; FILE.hdr / .npy: the linear mean radiance, top row first (one GPU)")
a = ap.parse_args()
light_mode = {"quads": 1, "all": 2, "mesh": 4, "tree": 16, "env": 32, "env+tree": 48}.get(a.light_sampling_mode, 1 if a.light_sampling else 0)   # RT_LIGHT_SAMPLING_*
if a.refine < 0 or (a.until is not None and (a.refine == 0 or a.gpus > 1)):
    ap.error("--until needs --refine STEP > 0 and one GPU (the multi-GPU renderer has no noise figure)")
if (a.denoise or a.aov) and (a.refine == 0 or a.gpus > 1):
    ap.error("--denoise and --aov need --refine STEP > 0 and one GPU (feature buffers accumulate alongside refinement)")
linear_out = a.out.lower().endswith((".hdr", ".npy"))
if linear_out:
    if a.gpus > 1:
        ap.error("--out FILE.hdr / FILE.npy reads the refinement sums of one GPU")
    a.refine = a.refine or a.spp   # the sums are the refinement's: one step of --spp samples unless --refine says otherwise
p = G.load_package()
from ray_tracing_v06_amd import image_io
W, H = a.width, a.height
PREFAB_FOV = {"three_spheres": 90.0, "cornell_box": 40.0, "cornell_lamp": 40.0, "book2_final": 40.0, "book1_final": 20.0, "book2_moving": 20.0}
if a.scene == "three_spheres":
    scene, cam = p.Scene.three_spheres(), p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, W / H)
elif a.scene in ("cornell_box", "cornell_lamp"):
    scene, cam = getattr(p.Scene, a.scene)(), p.PinholeCamera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H)
elif a.scene == "book2_final":
    scene, cam = p.Scene.book2_final(a.seed), p.MotionBlurCamera((478, 278, -600), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
elif a.scene == "book1_final":
    scene, cam = p.Scene.book1_final(a.seed), p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.1, 10.0)
else:
    scene, cam = p.Scene.book2_moving(a.seed), p.MotionBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.0, 1.0)
if a.camera:   # a lens camera at the prefab camera's place unless --lookfrom / --lookat say otherwise
    import math
    vec = lambda text: tuple(float(x) for x in text.split(","))   # noqa: E731
    eye = vec(a.lookfrom) if a.lookfrom else tuple(cam.o)
    w = tuple(cam.w) if cam.type == 1 else tuple(c / math.sqrt(sum(x * x for x in cam.w)) for c in cam.w)
    at = vec(a.lookat) if a.lookat else tuple(e + d for e, d in zip(eye, w))
    focus = a.focus_dist if a.focus_dist is not None else math.dist(eye, at)
    t0, t1 = vec(a.shutter) if a.shutter else (0.0, 0.0)
    lens = (a.aperture, focus, t0, t1)
    if a.camera == "perspective":
        cam = p.api.PerspectiveCamera(eye, at, (0, 1, 0), a.camera_fov if a.camera_fov is not None else PREFAB_FOV[a.scene], W / H, *lens)
    elif a.camera == "orthographic":
        if a.camera_height is None:
            sys.exit("--camera orthographic needs --camera-height H, the window's height in world units")
        cam = p.api.OrthographicCamera(eye, at, (0, 1, 0), a.camera_height, W / H, *lens)
    elif a.camera == "fisheye":
        cam = p.api.FisheyeCamera(eye, at, (0, 1, 0), a.camera_fov if a.camera_fov is not None else 180.0, W / H, *lens)
    else:
        cam = p.api.PanoramaCamera(eye, at, (0, 1, 0), *vec(a.camera_span), *lens)
if (a.texture or a.mtl) and not a.mesh:
    sys.exit("--texture needs --mesh FILE.obj" if a.texture else "--mtl needs --mesh FILE.obj")
if a.mesh:
    from ray_tracing_v06_amd import mesh_io
    vertices, faces = mesh_io.from_spec(a.mesh)
    normals = normal_faces = None
    if a.smooth:
        if a.mesh.startswith("icosphere:"):
            normals = mesh_io.icosphere_normals(int(a.mesh.split(":", 1)[1]))
        elif a.mesh != "tetrahedron":
            _, _, normals, normal_faces = mesh_io.load_obj_normals(a.mesh)
        if normals is None:
            normals = mesh_io.vertex_normals(vertices, faces)
    uvs = uv_faces = None
    read_image = lambda path: (image_io.read_png if path.lower().endswith(".png") else image_io.read_ppm)(path)   # noqa: E731
    # the images of this call go into the scene's texture table once there is more to say than "one image, clamp, nearest" — or when the scene
    # has an image of its own (book2_final's earth stays image 0); otherwise the one image is the world's, as ever
    in_table = a.mtl or a.scene == "book2_final" or (a.texture_wrap, a.texture_filter) != ("clamp", "nearest")

    def image_material(path):
        if in_table:
            return scene.ImageTexture(scene.add_image(read_image(path), a.texture_wrap, a.texture_filter))
        scene.set_image(read_image(path))
        return scene.ImageTexture()
    if a.texture or a.mtl:
        if a.mesh.startswith("icosphere:") or a.mesh == "tetrahedron":
            sys.exit(f"--texture: {a.mesh} has no texture coordinates; give an OBJ file with `vt` lines")
        if a.texture and len(a.texture) > 1 and not a.mtl:
            sys.exit("--texture: more than one image needs --mtl (one per material group of the OBJ)")
        _, _, uvs, uv_faces = mesh_io.load_obj_uvs(a.mesh)
        if uvs is None and a.texture:
            sys.exit(f"--texture: {a.mesh} has no complete set of texture coordinates (`vt` lines and a second index at every face corner)")
    def frosted(mat):   # --rough-glass: the prefab glass with a rough-glass record
        if a.rough_glass is not None:
            scene.set_rough_glass(mat, a.rough_glass)
        return mat

    def solid(mat, group_faces, what, tf=None):
        """--solid-glass: (faces wound outward, whether they were turned) and an interior record on `mat` — or a warning and the faces as they are"""
        if not a.solid_glass:
            return group_faces, False
        try:
            outward = mesh_io.orient_outward(vertices * a.mesh_scale, group_faces)   # (a negative scale turns the winding)
        except ValueError as e:
            print(f"warning: --solid-glass: {what} stays thin glass: {e}", file=sys.stderr, flush=True)
            return group_faces, False
        tint = [float(x) for x in a.glass_tint.split(",")] if a.glass_tint else tf
        scene.set_interior(mat, **(dict(color=[min(max(c, 1e-6), 1.0) for c in tint], at=a.glass_tint_at) if tint else {}))
        return outward, not mesh_io.closed_outward(vertices * a.mesh_scale, group_faces)

    plain = {"white": lambda: scene.Lambertian((0.73, 0.73, 0.73)), "red": lambda: scene.Lambertian((0.65, 0.05, 0.05)), "metal": lambda: scene.Metal((0.8, 0.85, 0.88), 0.0),
             "glass": lambda: frosted(scene.Dielectric((1, 1, 1), 1.5)), "checker": lambda: scene.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), abs(a.mesh_scale) / 4 if a.mesh_scale else 1.0),   # four squares across a unit mesh
             "light": lambda: scene.DiffuseLight((4, 4, 4))}[a.mesh_material]
    place = dict(scale=a.mesh_scale, rotate_y=a.mesh_rotate_y, translate=[float(x) for x in a.mesh_translate.split(",")])
    if a.mtl:   # one mesh per material group, in the order the OBJ first uses them
        import numpy as np
        names, libraries = mesh_io.load_obj_materials(a.mesh)
        library = {}
        for lib in libraries:
            library.update(mesh_io.load_mtl(os.path.join(os.path.dirname(os.path.abspath(a.mesh)), lib)))
        groups = list(dict.fromkeys(names))
        added = 0
        for k, name in enumerate(groups):
            rows = np.array([i for i, n in enumerate(names) if n == name])
            entry = library.get(name, {"Kd": None, "map_Kd": None})
            # glass, before everything else: a dissolve below 0.5 or one of the illumination models with refraction (4, 6, 7, 9) makes the group
            # a white dielectric of index Ni (1.5 when absent or not above 1), whatever its map_Kd and Pm; Pr or map_Pr then frosts it
            is_glass = entry.get("dissolve", 1.0) < 0.5 or entry.get("illum") in (4, 6, 7, 9)
            picture = None if is_glass else a.texture[k] if a.texture and k < len(a.texture) else entry["map_Kd"]
            if picture and uvs is None:
                sys.exit(f"--mtl: material {name!r} has an image and {a.mesh} has no complete set of texture coordinates")
            ior = entry.get("ior")
            mat = (scene.Dielectric((1, 1, 1), ior if ior is not None and ior > 1.0 else 1.5) if is_glass else image_material(picture) if picture
                   else scene.Lambertian(entry["Kd"]) if entry["Kd"] else plain())
            # microfacet surfaces: Pm >= 0.5 makes the group a metal with Kd as F0; Pr or map_Pr gives it a record — a rough conductor on the
            # metal, a coat of specular 0.04 on anything else — and map_Pr scales the roughness by the image's green channel (Pr = 1 when the file has none)
            roughness, roughness_map, metallic = entry.get("roughness"), entry.get("roughness_map"), entry.get("metallic")
            if metallic is not None and metallic >= 0.5 and not is_glass:
                mat, picture = scene.Metal(entry["Kd"] or (0.8, 0.85, 0.88), 0.0), None
            if roughness is not None or roughness_map:
                if is_glass:
                    scene.set_rough_glass(mat, 1.0 if roughness is None else roughness)
                else:
                    scene.set_microfacet(mat, 1.0 if roughness is None else roughness, 0.04)
                if roughness_map:
                    if uvs is None:
                        sys.exit(f"--mtl: material {name!r} has a roughness map and {a.mesh} has no complete set of texture coordinates")
                    scene.set_roughness_map(mat, scene.add_image(read_image(roughness_map), a.texture_wrap, a.texture_filter))
            # alpha cutouts: map_d names the group's opacity image; without one, the alpha channel of an RGBA map_Kd is the mask (R = G = B = alpha),
            # which then agrees with the colour texel for texel; the group is there where the mask is not below --cutout-cutoff
            cutout_map, mask = entry.get("cutout_map"), None
            if cutout_map:
                mask = read_image(cutout_map)
            elif picture and picture.lower().endswith(".png"):
                alpha = image_io.read_png_alpha(picture)
                if alpha is not None and (alpha != 255).any():
                    cutout_map, mask = picture + " (alpha)", np.repeat(alpha[:, :, None], 3, axis=2)
            if mask is not None:
                if uvs is None:
                    sys.exit(f"--mtl: material {name!r} has an opacity map and {a.mesh} has no complete set of texture coordinates")
                scene.set_cutout(mat, scene.add_image(mask, a.texture_wrap, a.texture_filter), a.cutout_cutoff)
            if is_glass and mask is not None and a.solid_glass:
                print(f"warning: --solid-glass: material {name!r} stays thin glass: it has an opacity map, and a holed solid has no inside", file=sys.stderr, flush=True)
            group_faces, turned = solid(mat, faces[rows], f"material {name!r}", entry.get("transmission_filter")) if is_glass and mask is None else (faces[rows], False)
            way = (lambda f: f[:, ::-1]) if turned else (lambda f: f)   # a turned face takes its normals and coordinates in the new order too
            group_normals = dict(normals=normals, normal_faces=way(normal_faces[rows] if normal_faces is not None else faces[rows])) if normals is not None else {}
            group_uvs = dict(uvs=uvs, uv_faces=way(uv_faces[rows])) if picture or roughness_map or mask is not None else {}
            added += scene.MakeMesh(vertices, group_faces, mat, **place, **group_normals, **group_uvs)[1]
            print(json.dumps({"material": name, "triangles": len(rows), "image": picture, "Kd": entry["Kd"], "roughness": roughness, "roughness_map": roughness_map,
                              "metallic": metallic, "glass": is_glass, "cutout_map": cutout_map}), flush=True)
    else:
        mat = image_material(a.texture[0]) if a.texture else plain()
        turned = False
        if a.mesh_material == "glass" and not a.texture:
            faces, turned = solid(mat, faces, a.mesh)
        if turned:
            normal_faces, uv_faces = (None if f is None else f[:, ::-1] for f in (normal_faces, uv_faces))
        first, added = scene.MakeMesh(vertices, faces, mat, **place, normals=normals, normal_faces=normal_faces, uvs=uvs, uv_faces=uv_faces)
    if a.scene == "three_spheres":
        scene.MakeHittableList()   # the prefab's own world kind
    else:
        scene.BuildBVH_TopDown()
    print(json.dumps({"mesh": a.mesh, "triangles": added, "skipped_degenerate": len(faces) - added}), flush=True)
if a.env:
    import numpy as np
    low = a.env.lower()
    if a.env == "sky":
        env = image_io.sky_environment(1024, 512)
    elif low.endswith(".hdr"):
        env = image_io.read_hdr(a.env)
    elif low.endswith(".npy"):
        env = np.load(a.env)
    elif low.endswith((".png", ".ppm")):
        env = (image_io.read_png if low.endswith(".png") else image_io.read_ppm)(a.env).astype(np.float32) / np.float32(255.0)
    else:
        sys.exit("--env: a .hdr, .npy, .png or .ppm file, or `sky`")
    scene.set_environment(np.asarray(env, dtype=np.float32) * np.float32(a.env_scale), rotate_y=a.env_rotate)
samples = a.spp
if a.refine:
    import time
    step_spp = min(a.refine, a.spp)   # what one pass is sized for; the steps go on to --spp
    r = (p.MultiRenderer.MakeRenderer(W, H, step_spp, a.depth, cam, scene.getWorldPtr(), a.gpus, seed=a.seed) if a.gpus > 1
         else p.Renderer.MakeRenderer(W, H, step_spp, a.depth, cam, scene.getWorldPtr(), seed=a.seed, device=a.device))
    if light_mode:
        r.light_sampling(light_mode)
    if a.denoise or a.aov:   # a world with a cutout table or a medium takes the full feature mode, one with a noise or an image material the
        import ctypes        # textured mode (§27); every other one the plain mode, as ever
        import numpy as np
        flat = scene.getWorldPtr()
        kinds = np.frombuffer((ctypes.c_char * (flat.n_materials * p.capi.MAT_DT.itemsize)).from_address(flat.materials), dtype=p.capi.MAT_DT)["type"]
        mode = p.api.feature_mode_for(kinds, scene.cutouts() is not None)
        r.enable_aov(textured=mode == "textured", full=mode == "full")
    samples, ms = 0, 0.0
    while samples < a.spp:
        n = min(a.refine, a.spp - samples)
        t0 = time.perf_counter()
        r.refine(n)
        ms += (time.perf_counter() - t0) * 1e3
        samples += n
        noise = r.noise() if a.gpus == 1 and samples >= 2 else None
        print(json.dumps({"samples": samples, "noise": noise, "elapsed_ms": round(ms, 3)}), flush=True)
        if a.until is not None and noise is not None and noise < a.until:
            break
elif a.gpus > 1:
    r = p.MultiRenderer.MakeRenderer(W, H, a.spp, a.depth, cam, scene.getWorldPtr(), a.gpus, seed=a.seed)
    if light_mode:
        r.light_sampling(light_mode)
    r.Render()
    ms = r.times()[0]     # host wall-clock of Render(): all shards, the exchange, the assembly
else:
    r = p.Renderer.MakeRenderer(W, H, a.spp, a.depth, cam, scene.getWorldPtr(), seed=a.seed, device=a.device)
    if light_mode:
        r.light_sampling(light_mode)
    r.Render()
    ms = r.last_kernel_ms()
fb = r.DownloadRenderbuffer()
# .jpg = the reference app's own format (stbi_write_jpg quality 95, FirstApp.cpp:120); .ppm / .png are lossless
writer = image_io.write_ppm if a.out.endswith(".ppm") else image_io.write_jpg if a.out.endswith((".jpg", ".jpeg")) else image_io.write_png
if linear_out:   # the mean radiance as it was summed: no clamp, no gamma; the frame's row 0 is the bottom, a picture's and an environment map's the top
    import numpy as np
    mean = (r.refine_sums()[::-1, :, 0:3] / np.float32(samples)).astype(np.float32)
    if a.out.lower().endswith(".npy"):
        np.save(a.out, mean)
    else:
        image_io.write_hdr(a.out, np.where(np.isfinite(mean) & (mean > 0), mean, np.float32(0.0)))   # RGBE holds finite values >= 0
    writer = image_io.write_png   # --denoise writes its .png beside it
else:
    writer(a.out, fb)
extra = {"aov_mode": r.aov_mode()} if a.denoise or a.aov else {}
if a.denoise:   # (with --refine only: `time` is imported there)
    t0 = time.perf_counter()
    den = r.denoise()
    stem, ext = os.path.splitext(a.out)
    ext = ".png" if linear_out else ext
    extra["denoised"] = stem + "_denoised" + ext
    extra["denoise_ms"] = round((time.perf_counter() - t0) * 1e3, 3)   # filter + download, host wall-clock
    writer(extra["denoised"], den)
if a.aov:
    import numpy as np
    f = r.aov()
    one = np.ones((H, W, 1), dtype=np.float32)
    near = f["depth"][f["coverage"] > 0]
    scale = np.float32(near.min()) if near.size else np.float32(1.0)
    depth = np.where(f["coverage"] > 0, scale / np.maximum(f["depth"], scale), np.float32(0.0)).astype(np.float32)
    image_io.write_png(a.aov + "_normal.png", np.concatenate([f["normal"] * np.float32(0.5) + np.float32(0.5), one], axis=2))
    image_io.write_png(a.aov + "_depth.png", np.concatenate([np.repeat(depth[..., None], 3, axis=2), one], axis=2))
    image_io.write_png(a.aov + "_albedo.png", np.concatenate([f["albedo"], one], axis=2))
    extra["aov"] = [a.aov + s for s in ("_normal.png", "_depth.png", "_albedo.png")]
print(json.dumps({**extra, "scene": a.scene, "width": W, "height": H, "spp": samples, "max_depth": a.depth, "render_ms": round(ms, 3),
                  "msamples_per_s": round(W * H * samples / ms / 1e3, 1), "gpus": a.gpus, "light_sampling": light_mode > 0, "light_sampling_mode": light_mode, "camera": a.camera or "prefab", "out": a.out}))
