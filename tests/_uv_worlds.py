"""The worlds of the texture-coordinate tests — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device.  The base is _tri_worlds' room at _smooth_worlds' frame (48 x 32, 8 spp,
depth 6).  uv_room() adds a uv_sphere(8, 4) with random texture coordinates; palette_room() / its stand-in are the pair of item "constant-UV faces": a mesh
whose every face has three equal coordinates at a texel centre of a 4 x 4 palette, and the same mesh with one plain Lambertian per face; open_pair() is the
open world that is held absolutely: two image-textured triangles under a white background.
"""
import numpy as np

import _tri_worlds as TW

SEED = 1984
W, H = 48, 32
SPP, DEPTH = 8, 6
ALBEDO_SCALE = np.float32(float.fromhex("0x1.010102p-8"))
EXT2_FORMS = [f for f in TW.FORMS if f[2] == 2]   # the eight TRI && EXT 2 keys


def palette():
    """a 4 x 4 image of sixteen different colours, uint8 [4][4][3]"""
    return np.random.default_rng(2201).integers(30, 256, (4, 4, 3)).astype(np.uint8)


def camera(p):
    return TW.camera(p, W, H)


def random_uvs(n, seed=7):
    """n coordinates from [-0.25, 1.25): wider than the unit square, so both clamps are met"""
    return (np.random.default_rng(seed).random((n, 2), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


SPHERE_AT = dict(scale=1.4, rotate_y=25.0, translate=(5, 5.0, 6.5))


def uv_room(p, normals=False, uvs="random", image=True, more=None, **room):
    """tri_room(textured=True) — its image-textured triangle on the back wall keeps the identity record — plus a uv_sphere(8, 4) (48 triangles) of the image
    material with random coordinates per vertex ("random"), its own ("sphere") or none (None); normals: with its exact vertex normals;
    image=False: the sphere is a plain Lambertian and the image is on a PARALLELOGRAM of the back wall instead of the room's triangle — still an EXT 2 world,
    whose triangles never read a table"""
    def add(s):
        m = TW.mesh_io()
        v, f, n, t = m.uv_sphere(8, 4)
        mat = s.ImageTexture() if image else s.Lambertian((0.3, 0.5, 0.8))
        kw = {}
        if normals:
            kw["normals"] = n
        if uvs is not None:
            kw["uvs"] = random_uvs(len(v)) if uvs == "random" else t
        s.MakeMesh(v, f, mat, SPHERE_AT["scale"], SPHERE_AT["rotate_y"], SPHERE_AT["translate"], **kw)
        if not image:
            from _nee_worlds import small_image
            s.set_image(small_image())
            s.MakeQuad((0.8, 5.2, 9.9), (2.5, 0, 0), (0, 2.5, 0), s.ImageTexture())
        if more is not None:
            more(s)
    return TW.tri_room(p, textured=image, more=add, **room)


# ---- constant-UV faces and their stand-in ----------------------------------------------------------------------------------------------------------------
def _palette_mesh():
    m = TW.mesh_io()
    v, f = m.icosphere(0)   # 20 faces
    texels = np.random.default_rng(5).integers(0, 4, (len(f), 2))   # (column, row from the BOTTOM) per face
    centres = ((texels.astype(np.float32) + np.float32(0.5)) / np.float32(4)).astype(np.float32)   # k / 4 + 1 / 8: exact in float32
    return v, f, texels, centres


def palette_room(p, stand_in=False, normals=False, textured=True, **room):
    """the room plus an icosphere(0) whose face k has three equal texture coordinates, the centre of texel texels[k] of the 4 x 4 palette — or, stand_in, one
    Lambertian of that texel's colour (px * 0x1.010102p-8, image_texel's own product) per face.  Type 7 and type 0 make the same draws, and a texel centre is
    2^20 ulps from a boundary, so the two worlds render the same frame.  textured: the room's own identity triangle on the back wall (an EXT 2 world either way
    then); without it the stand-in is an EXT 1 world.  normals: the mesh's exact vertex normals on both."""
    v, f, texels, centres = _palette_mesh()
    img = palette()

    def add(s):
        s.set_image(img)
        nrm = TW.mesh_io().icosphere_normals(0) if normals else None
        at = (1.3, 15.0, (5, 5.2, 6.5))
        if stand_in:
            for k in range(len(f)):
                px = img[3 - texels[k, 1], texels[k, 0]].astype(np.float32) * ALBEDO_SCALE
                s.MakeMesh(v, f[k:k + 1], s.Lambertian(px), *at, **({"normals": nrm} if normals else {}))
        else:
            s.MakeMesh(v, f, s.ImageTexture(), *at, uvs=np.repeat(centres, 3, axis=0), uv_faces=np.arange(3 * len(f)).reshape(-1, 3),
                       **({"normals": nrm} if normals else {}))
    if not textured and not stand_in:   # the image world without the room's identity triangle: tri_room sets no image, add() does
        return TW.tri_room(p, textured=False, more=add, **room)
    return TW.tri_room(p, textured=textured, more=add, **room)


def palette_expected_texels():
    """(texels (20, 2): column and row-from-the-bottom per face, centres (20, 2) float32)"""
    _, _, texels, centres = _palette_mesh()
    return texels, centres


# ---- the open world held absolutely ----------------------------------------------------------------------------------------------------------------------
def pair_image():
    return np.random.default_rng(77).integers(0, 256, (3, 5, 3)).astype(np.uint8)   # 5 x 3: neither side a power of two


def open_pair(p, as_list=False):
    """a white constant background and one parallelogram cut into its two triangles, image-textured, facing the camera, with random coordinates from
    [-0.25, 1.25) per corner (six different ones: the two triangles do not agree along the diagonal)"""
    s = p.Scene()
    s.set_image(pair_image())
    s.set_background((1, 1, 1))
    mat = s.ImageTexture()
    t = random_uvs(6, seed=19)
    s.MakeTriangle((0.5, 0.5, 5), (9.5, 0.5, 5), (0.5, 8.5, 5), mat, uvs=t[0:3])
    s.MakeTriangle((9.5, 8.5, 5), (0.5, 8.5, 5), (9.5, 0.5, 5), mat, uvs=t[3:6])
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


# ---- crafted hits: one triangle, a record and a point per case --------------------------------------------------------------------------------------------
TRI = ((0, 0, 0), (2, 0, 0), (0, 2, 0))
GENERAL = ((0.125, 0.25), (0.875, 0.375), (0.5, 0.9375))
WIDE = ((-0.25, -0.125), (1.25, 0.5), (0.5, 1.5))
EDGES = ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0))   # exactly 0.0 and 1.0
EQUAL = ((0.625, 0.375),) * 3
IDENTITY = ((0, 0), (1, 0), (0, 1))
POINTS = (("vertex a", (0, 0)), ("vertex b", (2, 0)), ("vertex c", (0, 2)), ("midpoint ab", (1, 0)), ("midpoint ac", (0, 1)), ("midpoint bc", (1, 1)),
          ("alpha + beta == 1", (0.5, 1.5)), ("inside", (0.5, 0.25)))


def crafted_cases():
    """[(name, record (3, 2), point of the plane z = 0 aimed at)]: every point under every record"""
    return [(f"{rn}: {pn}", rec, pt) for rn, rec in (("general", GENERAL), ("below 0 and above 1", WIDE), ("exactly 0.0 and 1.0", EDGES), ("three equal", EQUAL),
                                                      ("identity", IDENTITY)) for pn, pt in POINTS]


def crafted_arrays(p):
    """the cases as rt_tri_uv_batch takes them: (names, tris (capi.QUAD_DT), uv (n, 3, 2), rays (n, 6), t (n,)); every ray comes straight down z from z = 3"""
    cases = crafted_cases()
    s = p.Scene()
    s.MakeTriangle(*TRI, s.Lambertian((0.5, 0.5, 0.5)))
    s.MakeHittableList()
    tri = s.quads()[0]
    n = len(cases)
    tris = np.repeat(tri[None], n)
    uv, rays, t = np.zeros((n, 3, 2), np.float32), np.zeros((n, 6), np.float32), np.ones(n, np.float32)
    for i, (_, rec, (x, y)) in enumerate(cases):
        uv[i] = np.asarray(rec, np.float32)
        rays[i] = (x, y, 3.0, 0.0, 0.0, -3.0)   # the target is at t = 1 exactly
    return [c[0] for c in cases], tris, uv, rays, t


def crafted_world(p, as_list, with_quad=False):
    """the crafted triangle with a sphere far behind it (so that a list's bounds do not end in the triangle's plane); with_quad: plus an image-textured
    parallelogram in FRONT of its right part (x >= 0.75), which must keep its planar coordinates whatever the table says"""
    s = p.Scene()
    s.set_image(palette())
    m = s.ImageTexture()
    s.MakeTriangle(*TRI, m)
    s.MakeSphere((0.5, 0.5, -30), 3.0, s.Lambertian((0.5, 0.5, 0.5)))
    if with_quad:
        s.MakeQuad((0.75, -0.5, 1), (1.75, 0, 0), (0, 3, 0), m)
    s.MakeHittableList() if as_list else s.BuildBVH_TopDown()
    return s
