"""The rooms of the tests of the feature pass's third mode (RT_AOV_FULL) — test infrastructure only.

room(): one recipe for three rooms.  The cutout room: a floor, a checker wall that covers half of the view, two spheres, and in front of them three masked
surfaces — a lattice-masked parallelogram (the fence), a card of two triangles with texture coordinates (and, `normals`, vertex normals) and a plain
triangle —, half of each against the wall and the spheres, half against the open background, so that a ray through a hole either hits something farther or
misses.  The fog room: the same floor, wall and spheres behind a constant medium, a sphere large enough that the camera looks through it at all of them.  The
mixed room: both.  `walk` builds the world as a list, as a BVH walked by the stack, the queue or four wide.  fog_tree(): spheres and a medium under a bvh_node
tree, which no streaming kernel takes.  Every world is built through the product's host vocabulary, which needs no device.
"""
import numpy as np

import _cutout_worlds as CW

F = np.float32
SEED = CW.SEED
W, H, SPP, DEPTH = 24, 16, 8, 6
EYE = (0.0, 2.0, 9.0)
BACKGROUND = (0.6, 0.7, 0.9)
FOG_ALBEDO = (0.8, 0.85, 0.9)
WALKS = {"stack": 0, "list": 0, "queue": 1, "wide4": 2}


def camera(p, w=W, h=H):
    return p.PinholeCamera(EYE, (0.0, 1.8, -4.0), (0, 1, 0), 50.0, w / h)


def room(p, walk="stack", masks=True, fog=False, uvs=True, normals=False, opaque=False, env=False):
    """masks: the three masked surfaces (opaque: each under the all-white mask, the solid cards); fog: the medium; env: under the sky map of tests/_env_worlds.py
    instead of the constant background (tools/aov_full_cost.py).  The card's triangles are the world's last."""
    s = p.Scene()
    images = {name: s.add_image(img, wrap=wrap, filter=filt) for name, (img, wrap, filt) in CW.masks().items()}
    floor, wall = s.Lambertian((0.6, 0.55, 0.5)), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 1.3)
    fence_mat, card_mat, wedge_mat = s.Lambertian((0.7, 0.5, 0.3)), s.Lambertian((0.3, 0.7, 0.3)), s.Metal((0.8, 0.6, 0.5), 0.1)
    glass, metal = s.Dielectric((1, 1, 1), 1.5), s.Metal((0.8, 0.8, 0.9), 0.05)
    s.MakeQuad((-10, 0, -6), (20, 0, 0), (0, 0, 10), floor)
    s.MakeQuad((-7, 0, -4), (7, 0, 0), (0, 9, 0), wall)   # the left half of the view; the right half is open
    s.MakeSphere((-2.6, 1.0, -1.0), 1.0, glass)
    s.MakeSphere((2.2, 1.0, -2.0), 1.0, metal)
    if fog:
        s.MakeSphere((0.0, 2.0, 2.5), 3.0, s.add_material(p.capi.MAT_ISOTROPIC, FOG_ALBEDO, 0.25))
    if masks:
        s.MakeQuad((-3.5, 0.3, 4.0), (7, 0, 0), (0, 1.6, 0), fence_mat)
        s.MakeTriangle((-3.2, 2.2, 4.5), (0.6, 2.2, 4.5), (-1.3, 4.6, 4.5), wedge_mat)
        v = np.array([(0.3, 2.1, 5.0), (3.4, 2.1, 5.0), (3.4, 4.6, 5.0), (0.3, 4.6, 5.0)], F)
        f = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
        bent = np.array([(-0.5, -0.4, 1.0), (0.5, -0.4, 1.0), (0.5, 0.4, 1.0), (-0.5, 0.4, 1.0)], F)
        s.MakeMesh(v, f, card_mat, uvs=np.array([(0, 0), (2, 0), (2, 2), (0, 2)], F) if uvs else None, normals=bent if normals else None)
        white = images["white"]
        s.set_cutout(fence_mat, white if opaque else images["fence"]).set_cutout(card_mat, white if opaque else images["card"], 0.5)
        s.set_cutout(wedge_mat, white if opaque else images["wedge"], 0.25)
    if env:
        import _env_worlds as EW
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(BACKGROUND)
    if walk == "list":
        s.MakeHittableList()
    else:
        s.set_traversal(WALKS[walk])
        s.BuildBVH_SAH()
    s.names = dict(images=images, fence=fence_mat, card=card_mat, wedge=wedge_mat)
    return s


def fog_tree(p, n=8, seed=5):
    """spheres and one medium under a bvh_node tree: beyond the reference's feature set, so it renders on the baseline kernel alone"""
    rng = np.random.default_rng(seed)
    s = p.Scene()
    refs = [s.prim_ref(s.MakeSphere((0, 0, -6), 2.5, s.add_material(p.capi.MAT_ISOTROPIC, FOG_ALBEDO, 0.3)))]
    for _ in range(n):
        c = (rng.random(3, dtype=F) * 2 - 1) * 3
        c[2] -= 9
        refs.append(s.prim_ref(s.MakeSphere(c, float(rng.random() * 0.8 + 0.3), s.Lambertian(rng.random(3, dtype=F)))))
    while len(refs) > 1:
        nxt = [s.bvh_node(refs[i], refs[i + 1]) for i in range(0, len(refs) - 1, 2)]
        if len(refs) % 2:
            nxt.append(refs[-1])
        refs = nxt
    s.set_world_node_tree(refs[0])
    return s


def tables(scene):
    """what a renderer made from the scene's world holds, as the twin takes it: dict(uv, vn, cutouts, table)"""
    uv, vn = scene.texture_coords(), scene.vertex_normals()
    cut = scene.cutouts()
    return dict(uv=uv if uv is not None and len(uv) else None, vn=vn if vn is not None and len(vn) else None,
                cutouts=None if cut is None else np.asarray(cut).copy(), table=CW.twin_table(scene))

