"""The images, coordinates and worlds of the texture-table tests — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device.  Frames are 48 x 32, 8 samples, depth <= 8; images are 1 x 1, 2 x 2, 5 x 3,
8 x 4 and 16 x 16: the small odd sizes are where the wrap and cap arithmetic goes wrong, three images of different sizes where the index and first-texel
arithmetic does.  routing_room() / its stand-in: a sphere, a parallelogram and a UV-mapped mesh under three CONSTANT images, against plain Lambertians of those
colours.  open_world(k): the world held absolutely — only image-textured surfaces under a white background, three non-constant images, each surface kind under
another mode pair per k.  riders_room(): vertex normals, texture coordinates, an environment map and the table together.
"""
import numpy as np

import _tex_twin as XT
import _tri_worlds as TW
import _uv_worlds as UW

SEED = 1984
W, H = UW.W, UW.H
SPP, DEPTH = 8, 8
F = np.float32
SIZES = [(1, 1), (2, 2), (5, 3), (8, 4), (16, 16)]   # (width, height)
EXT2_FORMS = UW.EXT2_FORMS
MODE_NAMES = {(0, 0): ("clamp", "nearest"), (0, 1): ("clamp", "bilinear"), (1, 0): ("repeat", "nearest"), (1, 1): ("repeat", "bilinear")}


def image(width, height, seed=0):
    """a random image uint8 [height][width][3]"""
    return np.random.default_rng(1000 * width + height + seed).integers(0, 256, (height, width, 3)).astype(np.uint8)


def constant(width, height, colour):
    return np.broadcast_to(np.asarray(colour, np.uint8), (height, width, 3)).copy()


def coords(width, height):
    """the coordinates of the rule's tests, one list used for u and (rolled) for v: +-0, 1, exact texel borders and centres, values just inside and outside
    [0, 1], -3.25 and 7.5, 1e30, +-inf, NaN and denormals"""
    c = [0.0, -0.0, 1.0, -3.25, 7.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, -1e-39, 0.5, 0.25, 0.75, 1.5, -0.5, 2.0, -1.0]
    one = F(1)
    c += [np.nextafter(F(0), one), np.nextafter(F(0), -one), np.nextafter(one, F(0)), np.nextafter(one, F(2)), np.nextafter(F(0.5), one), np.nextafter(F(0.5), F(0))]
    for n in (width, height):
        for k in range(n + 1):
            b = F(k) / F(n)
            c += [b, np.nextafter(b, F(-1)), np.nextafter(b, F(2)), (F(k) + F(0.5)) / F(n), b + F(3), b - F(2)]
    c = np.array(c, F)
    rnd = (np.random.default_rng(width * 31 + height).random(64, dtype=F) * F(5) - F(2)).astype(F)
    u = np.concatenate([c, rnd])
    g = np.meshgrid(u, u, indexing="ij")
    return g[0].reshape(-1).astype(F), g[1].reshape(-1).astype(F)


def camera(p):
    return UW.camera(p)


# ---- routing: three constant images against a stand-in of plain Lambertians --------------------------------------------------------------------------------
ROUTING = [((200, 40, 30), (1, 1), ("clamp", "bilinear")), ((20, 180, 60), (5, 3), ("repeat", "nearest")), ((40, 70, 230), (8, 4), ("repeat", "bilinear"))]
MESH_AT = dict(scale=1.4, rotate_y=25.0, translate=(5, 5.0, 6.5))


def routing_room(p, stand_in=False, order=(0, 1, 2), use=(0, 1, 2), as_list=False, **room):
    """_tri_worlds' room (its metal icosphere, tetrahedron and checker triangle) plus a glass sphere and three textured things: a sphere on ROUTING[use[0]], a
    parallelogram on ROUTING[use[1]] and a uv_sphere(8, 4) with random coordinates from [-0.25, 1.25) on ROUTING[use[2]].  The images are added in `order`
    (the table's entries 1, 2, 3) and the materials numbered to match; entry 0 stays empty.  stand_in: plain Lambertians of the texel's colour instead —
    byte * 0x1.010102p-8 is an fp32 value, and a constant image is exactly constant under every mode, so the two worlds render one frame."""
    def add(s):
        index = {}
        if not stand_in:
            for k in order:
                colour, (w, h), (wrap, filt) = ROUTING[k]
                index[k] = s.add_image(constant(w, h, colour), wrap, filt)

        def mat(k):
            if stand_in:
                return s.Lambertian(np.asarray(ROUTING[k][0], np.uint8).astype(F) * UW.ALBEDO_SCALE)
            return s.ImageTexture(index[k])
        s.MakeSphere((2.2, 1.3, 3.5), 1.3, mat(use[0]))
        s.MakeQuad((6.5, 4.0, 9.9), (2.5, 0, 0), (0, 3.0, 0), mat(use[1]))
        v, f, _, _ = TW.mesh_io().uv_sphere(8, 4)
        s.MakeMesh(v, f, mat(use[2]), MESH_AT["scale"], MESH_AT["rotate_y"], MESH_AT["translate"], **({} if stand_in else {"uvs": UW.random_uvs(len(v))}))
        s.MakeSphere((8.2, 1.0, 3.0), 1.0, s.Dielectric((1, 1, 1), 1.5))
    return TW.tri_room(p, as_list=as_list, more=add, **room)


# ---- general content, held absolutely -----------------------------------------------------------------------------------------------------------------------
OPEN_IMAGES = [(5, 3), (8, 4), (16, 16)]
TRI_UVS = np.array([[-1.5, -1.5], [2.5, -0.5], [-0.75, 2.5], [2.5, 2.25], [-1.0, 2.5], [2.5, -1.5]], F)


def open_table(k):
    """the table of open_world(k) as the twin takes it: [(image, wrap, filter)] with entry 0 on the sphere, 1 on the parallelogram, 2 on the triangles"""
    return [(image(*OPEN_IMAGES[i], seed=7), *XT.MODES[(k + i) % 4]) for i in range(3)]


def open_world(p, k, as_list=False):
    """a white constant background and nothing but image-textured surfaces: a sphere (entry 0, the scene's own image under non-default modes), a parallelogram
    (entry 1) and one parallelogram cut into two triangles whose coordinates run from -1.5 to 2.5 (entry 2); surface kind i is under mode pair (k + i) % 4"""
    tab = open_table(k)
    s = p.Scene()
    s.set_background((1, 1, 1))
    s.set_image(tab[0][0])
    s.image_sampling(0, *MODE_NAMES[tab[0][1:]])
    i1 = s.add_image(tab[1][0], *MODE_NAMES[tab[1][1:]])
    i2 = s.add_image(tab[2][0], *MODE_NAMES[tab[2][1:]])
    assert (i1, i2) == (1, 2)
    s.MakeSphere((2.3, 6.6, 6.0), 1.6, s.ImageTexture(0))
    s.MakeQuad((5.0, 4.6, 6.0), (3.8, 0, 0.5), (0, 3.4, 0), s.ImageTexture(1))
    tri = s.ImageTexture(2)
    s.MakeTriangle((0.5, 0.3, 5), (9.5, 0.3, 5), (0.5, 3.9, 5), tri, uvs=TRI_UVS[0:3])
    s.MakeTriangle((9.5, 3.9, 5), (0.5, 3.9, 5), (9.5, 0.3, 5), tri, uvs=TRI_UVS[3:6])
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


# ---- all riders together ------------------------------------------------------------------------------------------------------------------------------------
def environment():
    yy, xx = np.mgrid[0:8, 0:16]
    return np.stack([0.05 * xx + 0.1, 0.1 * yy + 0.1, np.where((xx == 5) & (yy == 1), 30.0, 0.3)], axis=2).astype(F)


def riders_room(p, as_list=False, env=True, **room):
    """the room without its right wall under an environment map, lit by its quad light, a sphere light and a triangle light, holding a uv_sphere(8, 4) with its
    exact vertex normals and random texture coordinates on a 5 x 3 image under repeat / bilinear, a sphere on an 8 x 4 image under clamp / bilinear and the
    room's own image-textured triangle on entry 0 under repeat / nearest"""
    def add(s):
        m = TW.mesh_io()
        v, f, n, _ = m.uv_sphere(8, 4)
        a = s.add_image(image(5, 3, seed=3), "repeat", "bilinear")
        b = s.add_image(image(8, 4, seed=3), "clamp", "bilinear")
        s.image_sampling(0, "repeat", "nearest")
        s.MakeMesh(v, f, s.ImageTexture(a), MESH_AT["scale"], MESH_AT["rotate_y"], MESH_AT["translate"], normals=n, uvs=UW.random_uvs(len(v)))
        s.MakeSphere((2.2, 1.3, 3.5), 1.3, s.ImageTexture(b))
        if env:
            s.set_environment(environment(), rotate_y=30.0)
    return TW.tri_room(p, as_list=as_list, textured=True, open_right=True, lamp=True, tri_light=True, more=add, **room)
