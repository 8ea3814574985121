#!/usr/bin/env python3
"""Differential fuzz campaign: random worlds (spheres, moving spheres, quads, triangles and meshes, lights, media, textures; every builder; LDS
and global-memory paths; three cameras) rendered on the GPU and by the CPU oracle, compared bit for bit.
    python tools/fuzz_campaign.py --seeds 200 [--first 0] [--no-triangles] [--mesh-lights] [--light-tree] [--texture-coords] [--textures] [--env-tree] [--surfaces [--live]] [--interiors] [--cutouts [--live] [--aov-full]]
Prints one line per failure and a summary; exit code 1 if anything differed.  The triangles of a world come from a generator of their own, so the rest of a seed's
world is what it was before the fuzzer made triangles, and --no-triangles renders exactly those earlier worlds.  Importing this file starts nothing:
world_of_seed() builds a seed's world on the host, without a device.  --mesh-lights (off by default: the recorded campaigns ran without it) also renders every
world that RT_LIGHT_SAMPLING_MESH accepts in that mode; it draws nothing, so the worlds, frames and cameras of a seed stay what they are.  --texture-coords
 gives random triangles of every world with an image and triangles random texture coordinates from [-0.5, 1.5) — wider than the unit square —,
drawn from the seed's generator AFTER every other draw of the case, so committed seeds give the worlds, frames and cameras they gave.  --env-tree
puts every world with quads under the procedural sky as its LAST check — it draws nothing and the scene is not used again — and renders it in light-sampling
mode 48: both memory forms, and the twin (tests/_env_tree_twin.py) where it follows.  --surfaces also renders every world under the inert normal-map and
microfacet tables of tests/_surface_worlds.py — on a second scene built from the seed, so it draws nothing and leaves the seed's own scene alone — and holds both
kernel families, in both memory forms, to the oracle's frame the campaign has computed.  --interiors builds the seed's world once more with
glass solids in it — a sphere, a box and a closed mesh, placed, sized and given random interior records by a generator of its own — and holds the INTR family to
itself (both memory forms; every record off against no table); and, per seed, it renders a second world of static spheres, parallelograms and triangles with such
solids, built so that tests/_interior_twin.py follows its every sample, and holds both memory forms to the twin on every pixel.  --cutouts
renders, per seed, such a second world without the solids, with random masks — lattices and random opacities under random wrap modes, filters and cutoffs — on
random materials of its parallelograms and triangles, half the time with random texture coordinates on a mesh, and holds both memory forms of the CUT family to
the walk of tests/_cutout_twin.py on every pixel; with every record off the frame must be the frame without a table.  --cutouts --live renders,
per seed, the live world of --surfaces --live under tests/_live_worlds.random_masks(seed) — random masks on materials of every kind that takes one, one image
material masked by an alpha of its own picture's size and modes — in both memory forms against the composed twin, which must follow every sample, every record
off against no table, and with --aov-full its feature sums of mode RT_AOV_FULL against the feature twin."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G
import _env_tree_twin as VT
import _env_twin as ET
import _light_tree_twin as LT
import _mesh_light_twin as MT
import _nee_twin as T
import _oracle as O
import _tri_twin as TT
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, bits_equal

TRIANGLE_SHARE = 0.6   # of the worlds with quads; the others keep the kernels without the triangle family under the campaign


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--variants", action="store_true", help="pick a random kernel variant (0..5) per world — variant 5 (ray exchange) with random roles / thresholds / ring pairs —, now and then a forced multi-pass cut; unsupported combinations are skipped")
    ap.add_argument("--force-variant", type=int, default=None, help="render every world with this kernel variant; 6 (tolerance mode) is held to |delta| < 1e-3 and its differing frames are counted, not failed")
    ap.add_argument("--no-triangles", action="store_true", help="the worlds as they were before the fuzzer made triangles, byte for byte")
    ap.add_argument("--light-tree", action="store_true", help="also render the worlds that light-sampling mode 16 (the light tree, chosen by area) accepts in that mode: both memory forms, and the twin (tests/_light_tree_twin.py) where it follows")
    ap.add_argument("--env-tree", action="store_true", help="also render the worlds with quads, put under the procedural sky, in light-sampling mode 48 (the map and the light tree together, image hits sampled): both memory forms, and the twin (tests/_env_tree_twin.py) where it follows")
    ap.add_argument("--mesh-lights", action="store_true", help="also render the worlds that light-sampling mode 4 (triangle and mesh lights) accepts in that mode: both memory forms, and the twin where it follows")
    ap.add_argument("--textures", action="store_true", help="also render the worlds with an image under a texture table of several random images and random modes: the world's image under clamp / nearest must be the oracle's frame, and under another mode pair both memory forms must agree")
    ap.add_argument("--texture-coords", action="store_true", help="also render the worlds with an image and triangles under a table of random texture coordinates on random triangles: both memory forms must agree, and the identity table must be the oracle's frame")
    ap.add_argument("--surfaces", action="store_true", help="also render every world under inert normal-map and microfacet tables (flat maps; records that are all off on the materials in use): the NMAP and the MFAC kernel family, both memory forms, must give the oracle's frame; worlds the families refuse (a lane walk, a kernel variant other than 2 and 3) are counted as skipped")
    ap.add_argument("--live", action="store_true", help="with --surfaces: also render, per seed, a world of tests/_surface_worlds.random_surface_world(seed, live=True) — live normal-map, microfacet, rough-glass and interior records beside a constant medium, a noise material and moving spheres under a random camera kind — in both memory forms against the extended whole-sample twin, which must follow every sample; lane walks and kernel variants other than 2 and 3 are counted as skipped")
    ap.add_argument("--cutouts", action="store_true", help="with --live: also render, per seed, the live world of --surfaces --live under random masks (tests/_live_worlds.random_masks) against the composed twin, "
                    "and with --aov-full its feature sums against the feature twin; lane walks and kernel variants other than 2 and 3 are counted as skipped.  Without --live: also render, per seed, a world of its own with random masks on random parallelogram and triangle materials: the CUT kernel family in both memory forms against "
                    "the twin's walk (tests/_cutout_twin.py), every record off against no table")
    ap.add_argument("--aov-full", action="store_true", help="with --cutouts: also accumulate that world's feature buffers in mode RT_AOV_FULL (DESIGN.md §35), in both memory forms, and hold the sums of every "
                    "pixel to tests/_aov_full_twin.py")
    ap.add_argument("--interiors", action="store_true", help="also render every stack-walked or list world with random glass solids under random interior records: the INTR kernel family in both memory forms, every record off "
                    "against no table, and the twin (tests/_interior_twin.py) where it follows")
    return ap.parse_args(argv)


def image(h, w, rng):
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)


def make_world(p, rng, tri_rng=None, force_variant=None):
    """the world of one seed: everything but the triangles is drawn from rng, the triangles (kinds >= 1, tri_rng given) from tri_rng alone"""
    s = p.Scene()
    kinds = rng.integers(0, 4)   # 0 spheres only (reference features), 1 + quads/lights/background, 2 + media, 3 + textures
    if force_variant == 6:
        kinds = 0   # the tolerance mode exists for sphere worlds of the reference's feature set only
    mats = [s.Lambertian(rng.random(3)), s.Metal(rng.random(3), float(rng.choice([0.0, 0.1, 0.7, 1.0]))),
            s.Dielectric((1, 1, 1), float(rng.choice([1.5, 1.33, 1 / 1.5, 2.4]))),
            s.LambertianTexture(rng.random(3), rng.random(3), float(rng.choice([0.2, 0.5, 1.3])))]
    if kinds >= 1:
        mats.append(s.DiffuseLight(rng.random(3) * float(rng.choice([2.0, 8.0, 20.0]))))
    if kinds >= 3:
        s.set_perlin(int(rng.integers(0, 1 << 30)))
        s.set_image(image(int(rng.integers(1, 40)), int(rng.integers(1, 60)), rng))
        mats += [s.NoiseTexture(float(rng.choice([0.2, 1.0, 4.0])), rng.random(3)), s.ImageTexture()]
    surf = list(mats)
    media = []
    if kinds >= 2:
        media = [s.Isotropic(rng.random(3), float(rng.choice([0.01, 0.3, 2.0])))]
    big = rng.random() < 0.15 and force_variant != 6   # (and for LDS-resident worlds only)
    n = int(rng.integers(1500, 2600)) if big else int(rng.integers(1, 70))
    spread = 30.0 if big else 6.0
    for i in range(n):
        c = ((rng.random(3) * 2 - 1) * np.array([spread, 2, spread])).astype(np.float32)
        r = float(rng.choice([0.05, 0.2, 0.6])) if big else float(rng.choice([0.05, 0.3, 0.8, 2.5]))
        use_medium = media and rng.random() < 0.1
        m = media[0] if use_medium else surf[int(rng.integers(0, len(surf)))]
        if use_medium:
            r *= 3
        if rng.random() < 0.25:
            s.MakeMovingSphere(c, c + (rng.random(3).astype(np.float32) - 0.5), r, m)
        else:
            s.MakeSphere(c, r, m)
    if rng.random() < 0.5:
        s.MakeSphere((0, -500.0, 0), 498.0, surf[int(rng.integers(0, 4))])
    if kinds >= 1:
        quad_mats = list(surf)   # incl. the image texture (round 2: (u, v) = the planar coordinates of the hit)
        for _ in range(int(rng.integers(1, 25))):
            Q = ((rng.random(3) * 2 - 1) * np.array([spread, 3, spread])).astype(np.float32)
            if rng.random() < 0.4:
                u, v = np.float32([rng.random() * 4 + 0.3, 0, 0]), np.float32([0, 0, rng.random() * 4 + 0.3])
            else:
                u, v = (rng.standard_normal(3) * 2).astype(np.float32), (rng.standard_normal(3) * 2).astype(np.float32)
            s.MakeQuad(Q, u, v, quad_mats[int(rng.integers(0, len(quad_mats)))])
        if rng.random() < 0.3:
            s.MakeBox((-1, 0, -1), (1.5, 2, 1), quad_mats[0], float(rng.uniform(-40, 40)), (rng.random(3) * 4).astype(np.float32))
        if rng.random() < 0.6:
            s.set_background(tuple(float(x) for x in rng.random(3) * 0.4))
    if kinds >= 1 and tri_rng is not None and tri_rng.random() < TRIANGLE_SHARE:   # free triangles and now and then a mesh, as the random worlds of tests/_tri_worlds.py have them
        TW.random_triangles(s, tri_rng, quad_mats, spread=spread, meshes=int(tri_rng.random() < 0.3))
    # big worlds: the two O(n log n) builders, and (round 2) now and then a HittableList — the global-memory form of the list kernel
    builder = int(rng.integers(0, 4)) if not big else (3 if rng.random() < 0.08 else int(rng.integers(0, 2)))
    [s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList][builder]()
    if builder != 3 and rng.random() < 0.08:
        s.set_traversal(1 + int(rng.integers(0, 2)))   # the distance-sorted queue or the 4-wide walk: an overflow of the 32 entries is a refusal, not a failure
    return s, kinds, builder, big


def world_of_seed(p, seed, triangles=True, force_variant=None):
    """(scene, kinds, builder, big, rng): rng is the seed's generator after the world, from which the frame and the camera are drawn next"""
    rng = np.random.default_rng(900000 + seed)
    tri_rng = np.random.default_rng(700000 + seed) if triangles else None
    return make_world(p, rng, tri_rng, force_variant) + (rng,)


def light_sampling_check(p, s, w, cam, ck, W, H, depth, variant, mode=1):
    """A world rt_world_quad_lights accepts (mode 4, --mesh-lights: rt_world_light_table, and tests/_mesh_light_twin.py is the twin), with sampling on, at 4 spp on at most 48 x 32 pixels: the renderer's own form and the global-memory form must agree in
    every bit, and both must be the twin on every pixel it follows (pinhole cameras): tests/_nee_twin.py, or tests/_tri_twin.py for a world with triangles (static
    spheres and the stack walk only: another world with triangles is held across the two forms alone).  None: not applicable; else (ok, forms)."""
    W, H, spp = min(W, 48), min(H, 32), 4
    sums, forms = [], []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
            if (mode == 1 and not r.light_sampling_info()["lights"]) or r.kernel_info()["variant"] not in (2, 3):
                return None
            r.light_sampling(mode)
        except p.capi.RtError:
            return None   # no kernel for the world, or no light-sampling form for it
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        forms.append(r.kernel_form())
        r.refine(spp)
        sums.append(r.refine_sums())
        r.close()
    ok = bits_equal(sums[0], sums[1])
    if ck == 0:
        if mode in (4, 16):   # 16, --light-tree: tests/_light_tree_twin.py
            if w.traversal != 0 or (s.arrays()[1]["mat"] >> 31).any():
                return ok, forms
            samples, followed = (LT if mode == 16 else MT).frame_samples(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, depth, 1984, mode=mode)
        elif not s.n_triangles():
            samples, followed = T.frame_samples(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, depth, 1984, light_sampling=True)
        elif w.traversal == 0 and not (s.arrays()[1]["mat"] >> 31).any():
            samples, followed = TT.frame_samples(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, depth, 1984, mode=1)
        else:
            return ok, forms
        px = followed.all(axis=2)
        ok = ok and bits_equal(sums[0][px], T.in_order_sums(np.where(followed[..., None], samples, 0))[px])
    return ok, forms


def env_tree_check(p, s, cam, ck, W, H, depth, variant):
    """The world of a seed under image_io.sky_environment(32, 16) turned by 108 degrees (background mode 2), in mode 48 at 4 spp on at most 48 x 32
    pixels: the renderer's own form and the global-memory form must agree in every bit, and both must be the twin on every pixel it follows (a pinhole camera,
    the stack walk, no moving sphere; dielectrics and noise textures end the twin's following of a sample, image textures do not).  Changes the scene's
    background: the caller runs it last.  None: not applicable (a medium, a lane walk, a kernel without the form); else (ok, forms, lights)."""
    from ray_tracing_v06_amd import image_io
    s.set_environment(image_io.sky_environment(32, 16), rotate_y=108.0)
    w = s.getWorldPtr()
    W, H, spp = min(W, 48), min(H, 32), 4
    sums, forms, lights = [], [], 0
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
            if r.kernel_info()["variant"] not in (2, 3):
                return None
            r.light_sampling("env+tree")
        except p.capi.RtError:
            return None   # no kernel for the world under a map, or a refusal of the mode (a medium, a lane walk, a light lost in the running sum)
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        forms.append(r.kernel_form())
        lights = r.light_sampling_info()["lights"]
        r.refine(spp)
        sums.append(r.refine_sums())
        r.close()
    ok = bits_equal(sums[0], sums[1])
    if ck == 0 and w.traversal == 0 and not (s.arrays()[1]["mat"] >> 31).any():
        env_map, u0 = s.environment()
        world = as_oracle_world(w)
        tex = None
        if w.image_width:   # the world's image, entry 0 under clamp / nearest, and the scene's texture coordinates if it has any
            image0 = s.textures()[1][: w.image_width * w.image_height].reshape(w.image_height, w.image_width, 3)
            uv = s.texture_coords()
            tex = (uv if len(uv) else None, [(image0, 0, 0)])
        samples, followed = VT.frame_samples(world, as_oracle_camera(cam), W, H, spp, depth, 1984, ET.sky_environment(env_map, u0),
                                             light=(p.api.environment_distribution(env_map), u0), tree=VT.table_of(world), tex=tex)
        px = followed.all(axis=2)
        ok = ok and bits_equal(sums[0][px], T.in_order_sums(np.where(followed[..., None], samples, 0))[px])
    return ok, forms, lights


def texture_coords_check(p, s, w, cam, W, H, spp, depth, variant, rng, ref):
    """A world with an image and triangles on a stack-walk or list kernel: (1) under the identity table the frame is `ref`, the oracle's; (2) under a table of
    random coordinates on a random half of the triangles the renderer's own form and the global-memory form agree in every bit, and the table shows wherever an
    image-textured triangle was given coordinates and is seen.  The oracle does not know the rule (tests/test_gpu_texture_coords.py holds it absolutely).
    None: not applicable; else (ok, forms, mapped image-textured triangles)."""
    n = s.n_triangles()
    if not n or not w.image_width:
        return None
    table = np.tile(np.float32([0, 0, 1, 0, 0, 1]), (n, 1))
    chosen = rng.random(n) < 0.5                                                   # drawn after every other draw of the case
    table[chosen] = (rng.random((int(chosen.sum()), 6)) * 2.0 - 0.5).astype(np.float32)
    frames, forms = [], []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
            r.texture_coords(np.tile(np.float32([0, 0, 1, 0, 0, 1]), (n, 1)))
        except p.capi.RtError:
            return None   # no kernel for the world, or one that reads no table (queue / wide4 walks)
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        forms.append(r.kernel_form())
        r.Render()
        identity = r.DownloadRenderbuffer()
        r.texture_coords(table)
        r.Render()
        frames.append(r.DownloadRenderbuffer())
        r.close()
        if not bits_equal(identity, ref):
            return False, forms, 0
    quads, mats = s.quads(), s.arrays()[2]
    tris = quads[quads["kind"] == 1]
    mapped = int((chosen & (mats["type"][tris["mat"]] == 7)).sum())   # RT_MAT_LAMBERTIAN_IMAGE
    return bits_equal(frames[0], frames[1]), forms, mapped


def textures_check(p, s, w, cam, W, H, spp, depth, variant, rng, ref):
    """A world with an image on a streaming kernel, under a texture table of several random images and random modes: (1) entry 0 = the world's
    image under clamp / nearest, one to three random further entries behind it: the frame is `ref`, the oracle's, in the renderer's own form and in the
    global-memory form; (2) entry 0 under a random other mode pair: the two forms agree in every bit.  The worlds' materials all name image 0 (the oracle knows no
    other; tests/test_gpu_textures.py holds the further entries absolutely), so the further entries test the table's layout, not its routing.
    None: not applicable; else (ok, forms, the mode pair of (2))."""
    if not w.image_width:
        return None
    image0 = s.textures()[1][: w.image_width * w.image_height].reshape(w.image_height, w.image_width, 3)   # entry 0's texels come first
    more = [(rng.integers(0, 256, (int(rng.integers(1, 20)), int(rng.integers(1, 20)), 3)).astype(np.uint8), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
            for _ in range(int(rng.integers(1, 4)))]                                # drawn after every other draw of the case
    modes = [(0, 1), (1, 0), (1, 1)][int(rng.integers(0, 3))]
    frames, forms = [], []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
            r.textures([(image0, 0, 0)] + more)
        except p.capi.RtError:
            return None   # no kernel for the world
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        forms.append(r.kernel_form())
        r.Render()
        plain = r.DownloadRenderbuffer()
        r.textures([(image0, *modes)] + more)
        r.Render()
        frames.append(r.DownloadRenderbuffer())
        r.close()
        if not bits_equal(plain, ref):
            return False, forms, modes
    return bits_equal(frames[0], frames[1]), forms, modes


def surfaces_check(p, seed, args, cam, W, H, spp, depth, variant, ref):
    """The seed's world once more, built afresh (the tables add images and materials to a scene), under tests/_surface_worlds.inert_tables: a normal-map table
    of flat maps alone (the NMAP family) and with a microfacet table whose records on the materials in use are off (the MFAC family), each in the renderer's own
    form and in the global-memory form.  Every frame must be `ref`, the oracle's.  None: not applicable (no material in use takes a record, a lane walk, a
    variant without the families); else (ok, forms)."""
    import _surface_worlds as SW
    forms, ok = [], True
    for family in ("NMAP", "MFAC"):
        s = world_of_seed(p, seed, not args.no_triangles, args.force_variant)[0]
        if s.getWorldPtr().traversal != 0 or not SW.takes_a_record(s):
            return None
        SW.inert_tables(s, microfacets=family == "MFAC")
        w = s.getWorldPtr()
        for env in ({}, {"RT06_FORCE_BIG": "1"}):
            os.environ.pop("RT06_FORCE_BIG", None)
            os.environ.update(env)
            try:
                r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
            except p.capi.RtError:
                return None   # no kernel of the families for the world
            finally:
                os.environ.pop("RT06_FORCE_BIG", None)
            if r.kernel_info()["variant"] not in (2, 3) or not (r.kernel_microfacet() if family == "MFAC" else r.kernel_normal_map()):
                r.close()
                return None
            forms.append((family, r.kernel_form()))
            r.Render()
            ok = bits_equal(r.DownloadRenderbuffer(), ref) and ok
            r.close()
    return ok, forms


def live_check(p, seed, variant):
    """tests/_live_worlds.random_live_sums(seed) on the GPU, in the renderer's own form and the global-memory form, against the extended twin: the
    sums of every pixel must be the twin's, and the twin must follow every sample.  None: a variant without the families; else (ok, forms, not followed)."""
    import _live_worlds as LW
    s, cam, (W, H, spp, depth), want, followed, recipe = LW.random_live_sums(p, seed)
    ok, forms = bool(followed.all()), []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, s.getWorldPtr(), seed=LW.SEED, variant=variant)
        except p.capi.RtError:
            return None
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        if r.kernel_info()["variant"] not in (2, 3) or not r.kernel_interior():
            r.close()
            return None
        forms.append(r.kernel_form())
        r.refine(spp)
        ok = bits_equal(r.refine_sums(), want) and ok
        r.close()
    return ok, forms, int((~followed).sum())


def live_cutout_check(p, seed, variant, aov_full):
    """tests/_live_worlds.random_live_sums(seed, masks=True) on the GPU, in the renderer's own form and the global-memory form, against the composed
    twin — the cutout rule in the leaf phase, then smooth normal and normal map —, which must follow every sample; in the second form every record off against no
    table; aov_full: the feature sums of mode RT_AOV_FULL in both forms against tests/_aov_full_twin.py under the world's normal-map table.  None: a variant
    without the family; else (ok, forms, not followed, candidates the rule turned down)."""
    import _aov_full_twin as FT
    import _cutout_twin as CT
    import _live_worlds as LW
    import _noise_twin as NZ
    stats = CT.new_stats()
    s, cam, (W, H, spp, depth), want, followed, recipe = LW.random_live_sums(p, seed, stats, masks=True)
    w, table = s.getWorldPtr(), s.cutouts()
    ok, forms = bool(followed.all()), []
    features = None
    if aov_full:
        world, uv, vn = as_oracle_world(w), s.texture_coords(), s.vertex_normals()
        tab = NZ.tables(world)
        features = FT.sums(world, as_oracle_camera(cam), W, H, spp, LW.SEED, uv=uv if uv is not None and len(uv) else None, cutouts=table,
                           table=LW.AT.twin_table(s.textures()), noise=lambda a, k, pts: NZ.value(tab, np.asarray(a, np.float32), np.float32(k), pts),
                           vn=vn if vn is not None and len(vn) else None, nmaps=s.normal_maps())
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, seed=LW.SEED, variant=variant)
        except p.capi.RtError:
            return None
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        if r.kernel_info()["variant"] not in (2, 3) or not r.kernel_cutout():
            r.close()
            return None
        forms.append(r.kernel_form())
        r.refine(spp)
        ok = bits_equal(r.refine_sums(), want) and ok
        if aov_full:   # a renderer of its own, so that the colour frames above and below are those of a renderer without feature buffers
            os.environ.update(env)
            try:
                f = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, seed=LW.SEED, variant=variant)
            finally:
                os.environ.pop("RT06_FORCE_BIG", None)
            f.enable_aov(full=True)
            f.refine(spp)
            ok = f.aov_mode() == "full" and f.kernel_cutout() and bits_equal(f.aov_sums(), features) and bits_equal(f.refine_sums(), want) and ok
            f.close()
        if env:
            r.cutouts(np.zeros(len(table), p.capi.CUTOUT_DT))
            r.refine(spp)
            off = r.refine_sums()
            ok = r.kernel_cutout() and ok
            r.cutouts(None)
            r.refine(spp)
            ok = not r.kernel_cutout() and bits_equal(off, r.refine_sums()) and ok
        r.close()
    return ok, forms, int((~followed).sum()), stats["rejected"]


def glass_solids(s, rng):
    """a glass sphere, a glass box and a closed glass mesh (half the time with vertex normals) into scene s, with random interior records — at least one — and
    now and then a frosted one, all drawn from rng"""
    from ray_tracing_v06_amd import mesh_io
    glass = [s.Dielectric((1, 1, 1), float(rng.choice([1.33, 1.5, 2.4]))) for _ in range(3)]
    s.MakeSphere((rng.random(3) * 2 - 1) * (4, 1, 4), float(rng.uniform(0.3, 1.2)), glass[0])
    lo = (rng.random(3) * 2 - 1) * (4, 1, 4)
    s.MakeBox(lo, lo + rng.uniform(0.3, 2.0, 3), glass[1], rotate_y=float(rng.uniform(0, 90)))
    v, f = mesh_io.icosphere(int(rng.integers(0, 2))) if rng.random() < 0.7 else mesh_io.tetrahedron()
    assert mesh_io.closed_outward(v, f)
    s.MakeMesh(v, f, glass[2], float(rng.uniform(0.4, 1.2)), float(rng.uniform(0, 90)), (rng.random(3) * 2 - 1) * (4, 1, 4),
               **(dict(normals=mesh_io.vertex_normals(v, f)) if rng.random() < 0.5 else {}))
    for m in glass:
        if rng.random() < 0.85:
            s.set_interior(m, sigma=rng.choice([0.0, 0.1, 1.0, 30.0], 3) * rng.random(3))
    if rng.random() < 0.3:
        s.set_rough_glass(glass[int(rng.integers(0, 3))], float(rng.random()))
    if s.interiors() is None:
        s.set_interior(glass[1], sigma=(0.5, 0.25, 1.0))


def interiors_check(p, seed, args, cam, W, H, spp, depth, variant):
    """The seed's world once more, built afresh, with glass_solids() in it (a generator of its own: the seed's stays what it is).  The INTR form of the renderer's
    kernel and its global-memory form must agree, and with every record off the frame must be the frame without a table.  None: not applicable (a lane walk, a
    variant without the family); else (ok, forms)."""
    s = world_of_seed(p, seed, not args.no_triangles, args.force_variant)[0]
    kind = s.getWorldPtr().kind   # (adding to the scene takes its world away until the next build)
    if s.getWorldPtr().traversal != 0 or kind not in (0, 1):
        return None
    glass_solids(s, np.random.default_rng(seed + (32 << 20)))
    (s.MakeHittableList if kind == 1 else s.BuildBVH_SAH)()
    w, table = s.getWorldPtr(), s.interiors()
    sums, forms = [], []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
        except p.capi.RtError:
            return None   # no kernel of the family for the world
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        if r.kernel_info()["variant"] not in (2, 3) or not r.kernel_interior():
            r.close()
            return None
        forms.append(r.kernel_form())
        r.refine(spp)
        sums.append(r.refine_sums())
    r.interiors(np.zeros(len(table), p.capi.INTERIOR_DT))
    r.refine(spp)
    off = r.refine_sums()
    r.interiors(None)
    r.refine(spp)
    ok = bits_equal(sums[0], sums[1]) and bits_equal(off, r.refine_sums())
    r.close()
    return ok, forms


def interiors_twin_world(p, seed):
    """(scene, pinhole camera, W, H, spp, depth) of a world the twin of tests/_interior_twin.py follows throughout: static spheres, parallelograms, a box and
    free triangles of Lambertian, metal, glass and — half the time — light materials under a constant background or the gradient, with glass_solids() in it; a
    BVH by any builder or a list.  The seed's world proper cannot serve: a quarter of its spheres move, and the twin's walk restates static ones."""
    rng = np.random.default_rng(seed + (33 << 20))
    s = p.Scene()
    mats = [s.Lambertian(rng.random(3)), s.Metal(rng.random(3), float(rng.choice([0.0, 0.1, 0.7]))), s.Dielectric((1, 1, 1), float(rng.choice([1.5, 1.33])))]
    if rng.random() < 0.5:
        mats.append(s.DiffuseLight(rng.random(3) * float(rng.choice([2.0, 8.0]))))
    pick = lambda: mats[int(rng.integers(0, len(mats)))]   # noqa: E731
    for _ in range(int(rng.integers(1, 12))):
        s.MakeSphere(((rng.random(3) * 2 - 1) * np.array([6, 2, 6])).astype(np.float32), float(rng.choice([0.3, 0.8, 2.5])), pick())
    for _ in range(int(rng.integers(1, 8))):
        Q = ((rng.random(3) * 2 - 1) * np.array([6, 3, 6])).astype(np.float32)
        s.MakeQuad(Q, (rng.standard_normal(3) * 2).astype(np.float32), (rng.standard_normal(3) * 2).astype(np.float32), pick())
    for _ in range(int(rng.integers(0, 6))):
        a = ((rng.random(3) * 2 - 1) * np.array([6, 3, 6])).astype(np.float32)
        s.MakeTriangle(a, a + (rng.standard_normal(3) * 2).astype(np.float32), a + (rng.standard_normal(3) * 2).astype(np.float32), pick())
    if rng.random() < 0.5:
        s.MakeSphere((0, -500.0, 0), 498.0, mats[0])
    if rng.random() < 0.6:
        s.set_background(tuple(float(x) for x in rng.random(3)))
    glass_solids(s, rng)
    [s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList][int(rng.integers(0, 4))]()
    W, H = int(rng.integers(17, 49)), int(rng.integers(9, 33))
    eye = ((rng.random(3) * 2 - 1) * np.array([9, 4, 9])).astype(np.float32)
    cam = p.PinholeCamera(eye, (0, 0, 0), (0, 1, 0), float(rng.uniform(20, 100)), W / H)
    return s, cam, W, H, int(rng.integers(1, 9)), int(rng.choice([2, 5, 8, 50]))


def cutouts_twin_world(p, seed):
    """(scene, pinhole camera, W, H, spp, depth) of a world the walk of tests/_cutout_twin.py follows throughout: static spheres, parallelograms, free triangles
    and a mesh (half the time with texture coordinates wider than the unit square) of Lambertian, metal, glass and — half the time — light materials, with one to
    three masks on random materials that take one"""
    from ray_tracing_v06_amd import image_io, mesh_io
    rng = np.random.default_rng(seed + (34 << 20))
    s = p.Scene()
    mats = [s.Lambertian(rng.random(3)), s.Metal(rng.random(3), float(rng.choice([0.0, 0.1, 0.7]))), s.Dielectric((1, 1, 1), float(rng.choice([1.5, 1.33]))),
            s.Lambertian(rng.random(3)), s.LambertianTexture(rng.random(3), rng.random(3), float(rng.uniform(0.5, 3.0)))]
    maskable = list(mats)
    if rng.random() < 0.5:
        mats.append(s.DiffuseLight(rng.random(3) * float(rng.choice([2.0, 8.0]))))
    pick = lambda: mats[int(rng.integers(0, len(mats)))]   # noqa: E731
    for _ in range(int(rng.integers(1, 8))):
        s.MakeSphere(((rng.random(3) * 2 - 1) * np.array([6, 2, 6])).astype(np.float32), float(rng.choice([0.3, 0.8, 2.5])), pick())
    for _ in range(int(rng.integers(2, 9))):
        Q = ((rng.random(3) * 2 - 1) * np.array([6, 3, 6])).astype(np.float32)
        s.MakeQuad(Q, (rng.standard_normal(3) * 3).astype(np.float32), (rng.standard_normal(3) * 3).astype(np.float32), pick())
    for _ in range(int(rng.integers(1, 6))):
        a = ((rng.random(3) * 2 - 1) * np.array([6, 3, 6])).astype(np.float32)
        s.MakeTriangle(a, a + (rng.standard_normal(3) * 3).astype(np.float32), a + (rng.standard_normal(3) * 3).astype(np.float32), pick())
    v, f = mesh_io.icosphere(int(rng.integers(0, 2)))
    s.MakeMesh(v, f, pick(), float(rng.uniform(0.8, 2.5)), float(rng.uniform(0, 90)), (rng.random(3) * 2 - 1) * (4, 1, 4),
               **(dict(uvs=(rng.random((len(v), 2)) * 2 - 0.5).astype(np.float32)) if rng.random() < 0.5 else {}))
    if rng.random() < 0.5:
        s.MakeSphere((0, -500.0, 0), 498.0, mats[0])
    if rng.random() < 0.6:
        s.set_background(tuple(float(x) for x in rng.random(3)))
    for _ in range(int(rng.integers(1, 4))):
        if rng.random() < 0.5:
            mask = image_io.lattice_mask(int(rng.integers(1, 33)), int(rng.integers(1, 33)), int(rng.integers(0, 6)), int(rng.integers(0, 6)), float(rng.random()))
        else:
            mask = np.repeat(rng.integers(0, 256, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 1)).astype(np.uint8), 3, axis=2)
        image = s.add_image(mask, wrap=str(rng.choice(["clamp", "repeat"])), filter=str(rng.choice(["nearest", "bilinear"])))
        s.set_cutout(maskable[int(rng.integers(0, len(maskable)))], image, float(rng.choice([0.0, 0.25, 0.5, 0.75, 1.0, rng.random()])))
    [s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList][int(rng.integers(0, 4))]()
    W, H = int(rng.integers(17, 49)), int(rng.integers(9, 33))
    eye = ((rng.random(3) * 2 - 1) * np.array([9, 4, 9])).astype(np.float32)
    cam = p.PinholeCamera(eye, (0, 0, 0), (0, 1, 0), float(rng.uniform(20, 100)), W / H)
    return s, cam, W, H, int(rng.integers(1, 9)), int(rng.choice([2, 5, 8, 50]))


def cutouts_twin_check(p, seed):
    """cutouts_twin_world(seed) on the GPU, in the renderer's own form and the global-memory form, against the twin's walk under the rule: the sums of every
    pixel must be the twin's, the twin must follow every sample (the world is built so), and with every record off the frame must be the frame without a
    table.  (ok, forms, pixels held, candidates the rule turned down)"""
    import _cutout_twin as CT
    import _cutout_worlds as CW
    import _path_twin as PT
    s, cam, W, H, spp, depth = cutouts_twin_world(p, seed)
    w, table = s.getWorldPtr(), s.cutouts()
    world = as_oracle_world(w)
    uv = s.texture_coords()
    uv = uv if uv is not None and len(uv) else None
    images = CW.twin_table(s)
    stats = CT.new_stats()
    trace = CT.walk_of(uv, table, images, stats)
    samples, followed = PT.frame_samples(lambda g, k: PT.radiance(world, as_oracle_camera(cam), W, H, depth, 1984, g, k, trace, sky=PT.own_sky(world), tex=(uv, images),
                                                                 glass=True), W, H, spp)
    want = VT.in_order_sums(samples)
    ok, forms = bool(followed.all()), []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=0)
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        ok = ok and r.kernel_cutout()
        forms.append(r.kernel_form())
        r.refine(spp)
        ok = ok and bits_equal(r.refine_sums(), want)
        if env:
            r.cutouts(np.zeros(len(table), p.capi.CUTOUT_DT))
            r.refine(spp)
            off = r.refine_sums()
            r.cutouts(None)
            r.refine(spp)
            ok = ok and bits_equal(off, r.refine_sums())
        r.close()
    return ok, forms, W * H, stats["rejected"]


def aov_full_check(p, seed):
    """cutouts_twin_world(seed) with feature buffers in mode RT_AOV_FULL, in the renderer's own form and the global-memory form: the feature sums of
    every pixel must be those of tests/_aov_full_twin.py, whose first trace is the cutout walk's.  (ok, pixels held, candidates the rule turned down)"""
    import _aov_full_twin as FT
    import _cutout_worlds as CW
    s, cam, W, H, spp, _ = cutouts_twin_world(p, seed)
    w, table = s.getWorldPtr(), s.cutouts()
    uv, vn = s.texture_coords(), s.vertex_normals()
    stats = FT.new_stats()
    want = FT.sums(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, 1984, uv=uv if uv is not None and len(uv) else None, cutouts=table, table=CW.twin_table(s),
                   vn=vn if vn is not None and len(vn) else None, stats=stats)
    ok = True
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, 2, cam, w, variant=0)
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        r.enable_aov(full=True)
        r.refine(spp)
        ok = ok and r.kernel_cutout() and r.aov_mode() == "full" and bits_equal(r.aov_sums(), want)
        r.close()
    return ok, W * H, stats["rejected"]


def interiors_twin_check(p, seed):
    """interiors_twin_world(seed) on the GPU, in the renderer's own form and the global-memory form, against the twin under the whole rule: the sums of every
    pixel must be the twin's, and the twin must follow every sample (the world is built so).  (ok, forms, pixels held)"""
    import _interior_twin as IT
    import _nee_twin as NT
    import _path_twin as PT
    import _smooth_twin as ST
    s, cam, W, H, spp, depth = interiors_twin_world(p, seed)
    w, table = s.getWorldPtr(), s.interiors()
    world = as_oracle_world(w)
    assert not (IT.world_arrays(world)[0]["mat"] & np.uint32(NT.PRIM_MOVING)).any()   # stated, not caught: the walk restates static spheres
    vn = s.vertex_normals()
    trace = ST.smooth_walk(vn) if vn is not None and len(vn) else TT.closest_intersection
    samples, followed = PT.frame_samples(lambda g, k: IT.radiance(world, as_oracle_camera(cam), W, H, depth, 1984, g, k, PT.own_sky(world), table, None, None,
                                                                 s.microfacets(), None, trace), W, H, spp)
    want = IT.in_order_sums(samples)
    ok, forms = bool(followed.all()), []
    for env in ({}, {"RT06_FORCE_BIG": "1"}):
        os.environ.pop("RT06_FORCE_BIG", None)
        os.environ.update(env)
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=0)
        finally:
            os.environ.pop("RT06_FORCE_BIG", None)
        ok = ok and r.kernel_interior()
        forms.append(r.kernel_form())
        r.refine(spp)
        ok = ok and bits_equal(r.refine_sums(), want)
        r.close()
    return ok, forms, W * H


def main(argv=None):
    args = parse_args(argv)
    p = G.load_package()
    fails = 0
    t0 = time.time()
    stats = {"lds": 0, "global": 0, "baseline": 0, "xchg": 0, "triangle_worlds": 0, "tri_kernels": 0}
    if args.surfaces:
        stats.update({"surface_worlds": 0, "surface_kernels": 0, "surface_skipped": 0})
    if args.cutouts and args.live:
        stats.update({"live_cutout_worlds": 0, "live_cutout_not_followed": 0})
    for seed in range(args.first, args.first + args.seeds):
        s, kinds, builder, big, rng = world_of_seed(p, seed, not args.no_triangles, args.force_variant)
        W, H = int(rng.integers(17, 120)), int(rng.integers(9, 80))
        spp, depth = int(rng.integers(1, 20)), int(rng.choice([1, 2, 5, 50]))
        eye = ((rng.random(3) * 2 - 1) * np.array([9, 4, 9])).astype(np.float32)
        if rng.random() < 0.1:
            eye[int(rng.integers(0, 3))] = float(rng.choice([0.0, 1e-30, -1e-25]))   # rays outside the fast-division class
        ck = int(rng.integers(0, 3))
        if ck == 0:
            cam = p.PinholeCamera(eye, (0, 0, 0), (0, 1, 0), float(rng.uniform(20, 100)), W / H)
        elif ck == 1:
            cam = p.DefocusBlurCamera(eye, (0, 0, 0), (0, 1, 0), float(rng.uniform(20, 100)), W / H, float(rng.uniform(0, 0.5)), float(rng.uniform(2, 12)))
        else:
            cam = p.MotionBlurCamera(eye, (0, 0, 0), (0, 1, 0), float(rng.uniform(20, 100)), W / H, 0.0, 1.0)
        w = s.getWorldPtr()
        variant = int(rng.integers(0, 6)) if args.variants else 0
        if args.force_variant is not None:
            variant = args.force_variant
        for k in ("RT06_XCHG", "RT06_PASS_SPP"):
            os.environ.pop(k, None)
        if args.variants and variant == 5:   # tracers, extra rays, exchange / shade thresholds, patience, priority, keep, ring pairs
            os.environ["RT06_XCHG"] = ",".join(str(int(x)) for x in (rng.integers(1, 12), rng.integers(0, 300), rng.integers(1, 65), rng.integers(1, 65),
                                                                       rng.integers(0, 12), rng.integers(0, 2), rng.integers(1, 65), rng.integers(1, 3)))
        if args.variants and rng.random() < 0.15:
            os.environ["RT06_PASS_SPP"] = str(int(rng.integers(1, 6)))
        try:
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
        except p.capi.RtError:
            stats["refused"] = stats.get("refused", 0) + 1   # e.g. variant 4 on an extended world, variant 3 on a HittableList
            continue
        info = r.kernel_info()
        tri_kernel = r.kernel_triangles()
        try:
            r.Render()
            img = r.DownloadRenderbuffer()
        except p.capi.RtError as e:
            if e.code != 4:
                raise
            stats["queue_overflow"] = stats.get("queue_overflow", 0) + 1
            r.close()
            continue
        r.close()
        if big and builder == 3:
            W, H, spp = min(W, 40), min(H, 24), min(spp, 3)   # (a 2000-sphere list costs the CPU oracle 2000 sphere tests per ray)
            r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, variant=variant)
            r.Render(); img = r.DownloadRenderbuffer(); r.close()
        ref, _ = O.render(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, depth)
        stats["baseline" if info["variant"] == 1 else ("xchg" if info["variant"] == 5 else ("lds" if info["lds_resident"] else "global"))] += 1
        if s.n_triangles():
            stats["triangle_worlds"] += 1
            stats["tri_kernels"] += int(tri_kernel)
        if w.traversal:
            stats[("queue", "wide4")[w.traversal - 1]] = stats.get(("queue", "wide4")[w.traversal - 1], 0) + 1
        if info["variant"] == 6:   # tolerance mode: inside |delta| < 1e-3; frames that are not the oracle's bits are counted
            same = bits_equal(img, ref)
            stats["tol_frames_not_bit_identical"] = stats.get("tol_frames_not_bit_identical", 0) + (0 if same else 1)
            dmax = 0.0 if same else float(np.nanmax(np.abs(img - ref)))
            stats["tol_max_abs_delta"] = max(stats.get("tol_max_abs_delta", 0.0), dmax)
            ok = np.array_equal(np.isnan(img), np.isnan(ref)) and dmax < 1e-3
        elif info["variant"] == 1:
            ok = np.array_equal(np.isnan(img), np.isnan(ref)) and float(np.nanmax(np.abs(img - ref))) <= 1e-5 * max(1.0, float(np.nanmax(ref)))
        else:
            ok = bits_equal(img, ref)
        if not ok:
            fails += 1
            bad = int((img.view(np.uint32) != ref.view(np.uint32)).sum())
            print(f"FAIL seed {seed}: kinds {kinds} triangles {s.n_triangles()} builder {builder} big {big} cam {ck} {W}x{H}x{spp} depth {depth} info {info}: {bad} words differ", flush=True)
        if ok and kinds >= 1 and info["variant"] in (2, 3):   # light sampling as one more feature of the case
            ls = light_sampling_check(p, s, w, cam, ck, W, H, depth, variant)
            if ls is not None:
                stats["light_sampling"] = stats.get("light_sampling", 0) + 1
                if not ls[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with light sampling: kinds {kinds} builder {builder} big {big} cam {ck} depth {depth} forms {ls[1]}", flush=True)
            ls = light_sampling_check(p, s, w, cam, ck, W, H, depth, variant, mode=4) if args.mesh_lights else None
            if ls is not None:
                stats["mesh_light_sampling"] = stats.get("mesh_light_sampling", 0) + 1
                if not ls[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with light sampling mode 4: kinds {kinds} triangles {s.n_triangles()} builder {builder} big {big} cam {ck} depth {depth} forms {ls[1]}", flush=True)
            ls = light_sampling_check(p, s, w, cam, ck, W, H, depth, variant, mode=16) if args.light_tree else None
            if ls is not None:
                stats["light_tree_sampling"] = stats.get("light_tree_sampling", 0) + 1
                if not ls[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with light sampling mode 16: kinds {kinds} triangles {s.n_triangles()} builder {builder} big {big} cam {ck} depth {depth} forms {ls[1]}", flush=True)
        if args.texture_coords and ok and info["variant"] in (2, 3) and not (big and builder == 3):
            tc = texture_coords_check(p, s, w, cam, W, H, spp, depth, variant, rng, ref)
            if tc is not None:
                stats["texture_coords"] = stats.get("texture_coords", 0) + 1
                stats["texture_coords_mapped_image_triangles"] = stats.get("texture_coords_mapped_image_triangles", 0) + tc[2]
                if not tc[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with texture coordinates: kinds {kinds} triangles {s.n_triangles()} builder {builder} big {big} cam {ck} depth {depth} forms {tc[1]}", flush=True)
        if args.textures and ok and info["variant"] in (2, 3) and not (big and builder == 3):
            tx = textures_check(p, s, w, cam, W, H, spp, depth, variant, rng, ref)
            if tx is not None:
                stats["textures"] = stats.get("textures", 0) + 1
                if not tx[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with a texture table: kinds {kinds} builder {builder} big {big} cam {ck} depth {depth} modes {tx[2]} forms {tx[1]}", flush=True)
        if args.surfaces and ok:
            sf = surfaces_check(p, seed, args, cam, W, H, spp, depth, variant, ref) if info["variant"] in (2, 3) and not (big and builder == 3) else None
            if sf is None:
                stats["surface_skipped"] += 1
            else:
                stats["surface_worlds"] += 1
                stats["surface_kernels"] += len(sf[1])
                if not sf[0]:
                    fails += 1
                    print(f"FAIL seed {seed} under inert surface tables: kinds {kinds} triangles {s.n_triangles()} builder {builder} big {big} cam {ck} {W}x{H}x{spp} depth {depth} forms {sf[1]}", flush=True)
        if args.surfaces and args.live:   # a world of its own per seed, which the extended twin follows throughout
            lv = live_check(p, seed, variant) if w.traversal == 0 and info["variant"] in (2, 3) else None
            if lv is None:
                stats["live_skipped"] = stats.get("live_skipped", 0) + 1
            else:
                stats["live_worlds"] = stats.get("live_worlds", 0) + 1
                stats["live_kernels"] = stats.get("live_kernels", 0) + len(lv[1])
                stats["live_not_followed"] = stats.get("live_not_followed", 0) + lv[2]
                if not lv[0]:
                    fails += 1
                    print(f"FAIL seed {seed}: the live surface world: forms {lv[1]}, {lv[2]} samples not followed", flush=True)
        if args.interiors and ok and info["variant"] in (2, 3) and not big:
            it = interiors_check(p, seed, args, cam, W, H, spp, depth, variant)
            if it is not None:
                stats["interior_worlds"] = stats.get("interior_worlds", 0) + 1
                if not it[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with solid glass: kinds {kinds} triangles {s.n_triangles()} builder {builder} cam {ck} {W}x{H}x{spp} depth {depth} forms {it[1]}", flush=True)
        if args.interiors:   # a world of its own per seed, which the twin follows throughout
            tw = interiors_twin_check(p, seed)
            stats["interior_twin_worlds"] = stats.get("interior_twin_worlds", 0) + 1
            stats["interior_pixels_held_to_the_twin"] = stats.get("interior_pixels_held_to_the_twin", 0) + tw[2]
            if not tw[0]:
                fails += 1
                print(f"FAIL seed {seed}: the solid-glass twin world: forms {tw[1]}", flush=True)
        if args.cutouts:   # likewise
            tw = cutouts_twin_check(p, seed)
            stats["cutout_twin_worlds"] = stats.get("cutout_twin_worlds", 0) + 1
            stats["cutout_pixels_held_to_the_twin"] = stats.get("cutout_pixels_held_to_the_twin", 0) + tw[2]
            stats["cutout_candidates_turned_down"] = stats.get("cutout_candidates_turned_down", 0) + tw[3]
            if not tw[0]:
                fails += 1
                print(f"FAIL seed {seed}: the cutout twin world: forms {tw[1]}", flush=True)
        if args.cutouts and args.live:   # the live world of the seed under random masks
            lc = live_cutout_check(p, seed, variant, args.aov_full) if w.traversal == 0 and info["variant"] in (2, 3) else None
            if lc is None:
                stats["live_cutout_skipped"] = stats.get("live_cutout_skipped", 0) + 1
            else:
                stats["live_cutout_worlds"] = stats.get("live_cutout_worlds", 0) + 1
                stats["live_cutout_kernels"] = stats.get("live_cutout_kernels", 0) + len(lc[1])
                stats["live_cutout_not_followed"] = stats.get("live_cutout_not_followed", 0) + lc[2]
                stats["live_cutout_candidates_turned_down"] = stats.get("live_cutout_candidates_turned_down", 0) + lc[3]
                if not lc[0]:
                    fails += 1
                    print(f"FAIL seed {seed}: the live world under masks: forms {lc[1]}, {lc[2]} samples not followed", flush=True)
        if args.cutouts and args.aov_full:   # the same world under feature buffers
            fa = aov_full_check(p, seed)
            stats["aov_full_worlds"] = stats.get("aov_full_worlds", 0) + 1
            stats["aov_full_pixels_held_to_the_twin"] = stats.get("aov_full_pixels_held_to_the_twin", 0) + fa[1]
            stats["aov_full_candidates_turned_down"] = stats.get("aov_full_candidates_turned_down", 0) + fa[2]
            if not fa[0]:
                fails += 1
                print(f"FAIL seed {seed}: the feature sums of mode RT_AOV_FULL on the cutout twin world", flush=True)
        if args.env_tree and ok and kinds >= 1 and info["variant"] in (2, 3) and not (big and builder == 3):   # last: it changes the scene's background
            et = env_tree_check(p, s, cam, ck, W, H, depth, variant)
            if et is not None:
                stats["env_tree_sampling"] = stats.get("env_tree_sampling", 0) + 1
                stats["env_tree_without_lights"] = stats.get("env_tree_without_lights", 0) + int(et[2] == 0)
                if not et[0]:
                    fails += 1
                    print(f"FAIL seed {seed} with light sampling mode 48: kinds {kinds} triangles {s.n_triangles()} builder {builder} big {big} cam {ck} depth {depth} lights {et[2]} forms {et[1]}", flush=True)
        if (seed - args.first) % 25 == 24:
            print(f"... {seed - args.first + 1} worlds, {fails} failures, {time.time() - t0:.0f}s, paths {stats}", flush=True)
    print(f"DONE: {args.seeds} worlds, {fails} failures, paths {stats}, {time.time() - t0:.0f}s")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
