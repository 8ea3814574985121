"""The maps, directions and worlds of the environment-map tests — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device; what is computed here is computed once per process and never modified.
"""
import functools

import numpy as np

import _env_twin as ET
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
SEED = 1984
W, H = 24, 16
SPP, DEPTH = 8, 6
SIZES = [(1, 1), (2, 1), (7, 3), (16, 8), (64, 32)]                         # (width, height)
ROTATIONS = [F(0.0), F(0.25), F(0.5), np.nextafter(F(1.0), F(0.0))]         # the last: just under 1
ROTATION_IDS = ["u0=0", "u0=0.25", "u0=0.5", "u0<1"]
C = (1.75, 0.5, 0.25)   # the colour of the constant maps: one component above 1


def random_map(width, height, seed=0, decades=(-2, 3)):
    """an HDR map (height, width, 3) float32: texels scaled by 10^x, x uniform over `decades` — by default most below 1 and some far above"""
    rng = np.random.default_rng(1000 * width + height + seed)
    env = (rng.random((height, width, 3)) * 10.0 ** rng.uniform(decades[0], decades[1], (height, width, 1))).astype(F)
    env.setflags(write=False)
    return env


def constant_map(width=4, height=2, color=C):
    env = np.broadcast_to(np.array(color, F), (height, width, 3)).copy()
    env.setflags(write=False)
    return env


def random_directions(n, seed):
    """n directions uniform over the sphere, of random length in [1e-3, 1e3]"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d = d / np.linalg.norm(d, axis=1)[:, None] * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return np.ascontiguousarray(d, F)


@functools.lru_cache(maxsize=None)
def crafted_directions():
    """(names, (k, 3) float32): the axes, the seam, the poles, and per rotation a fan of directions whose u lands within ulps of 1 on both sides"""
    out = [("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)),
           ("seam z=+0", (-1, 0.3, 0.0)), ("seam z=-0", (-1, 0.3, -0.0)), ("seam z=+1e-30", (-1, 0.3, 1e-30)), ("seam z=-1e-30", (-1, 0.3, -1e-30)),
           ("seam x=-1e-3 z=+1e-30", (-1e-3, 0, 1e-30)), ("seam x=-1e-3 z=-1e-30", (-1e-3, 0, -1e-30)),
           ("pole up, tiny x z", (1e-20, 1, 1e-20)), ("pole down, tiny x z", (1e-20, -1, -1e-20)), ("pole up, -x", (-1e-30, 1, 0.0)), ("pole down, -z", (0.0, -1, -1e-30)),
           ("pole up, long", (1e-12, 1e3, -1e-12)), ("pole down, short", (-1e-12, -1e-3, 1e-15))]
    for u0, tag in zip(ROTATIONS, ROTATION_IDS):   # u = phi / 2 pi + u0 reaches 1 where atan2(-z, x) = 2 pi (1 - u0) - pi; steps of 2^-24 of a turn around it
        for k in range(-6, 7):
            a = 2.0 * np.pi * ((1.0 - float(u0)) + k * 2.0 ** -24) - np.pi
            out.append((f"fan {tag} {k:+d}", (np.cos(a), 0.2, -np.sin(a))))
    names = [n for n, _ in out]
    dirs = np.array([d for _, d in out], np.float64).astype(F)
    dirs.setflags(write=False)
    return names, dirs


@functools.lru_cache(maxsize=None)
def directions():
    """test 1's directions: 10^5 random ones and the crafted ones"""
    d = np.concatenate([random_directions(100000, seed=1), crafted_directions()[1]])
    d.setflags(write=False)
    return d


def camera(p, w=W, h=H):
    return TW.camera(p, w, h)


# ---- open sky: every primary ray misses -----------------------------------------------------------------------------------------------------------------
def open_sky(p, env, rotate_y=0.0):
    """two small spheres far behind the camera, under the map"""
    s = p.Scene()
    s.MakeSphere((5, 5, -400), 0.5, s.Lambertian((0.5, 0.5, 0.5)))
    s.MakeSphere((7, 4, -420), 0.5, s.Metal((0.5, 0.5, 0.5), 0.0))
    s.set_environment(env, rotate_y=rotate_y)
    s.BuildBVH_TopDown()
    return s


def open_sky_frame(p, env, u0, w=W, h=H, spp=SPP):
    """the frame of an open sky by the twin alone: the in-order mean of the lookups of the twin's primary rays"""
    cam = as_oracle_camera(camera(p, w, h))
    gids = np.repeat(np.arange(w * h, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), w * h)
    _, _, d = ET.primary_rays(cam, w, h, SEED, gids, smp)
    samples = ET.lookup(env, u0, d)[0].reshape(h, w, spp, 3)
    return ET.resolve(ET.in_order_sums(samples), spp)


# ---- the room of the constant-map test: everything a scattered ray can do before it leaves ---------------------------------------------------------------
def env_room(p, background, tri, as_list=False, traversal=0, builder="BuildBVH_SAH", tables=False, image_material=False):
    """_tri_worlds' room without its right wall, holding glass, fuzzy metal, a moving sphere, a checker, a quad light and a sphere light; tri: the glass and the
    fuzzy metal are small meshes and the checker a triangle (a TRI world), otherwise spheres; tables: the meshes carry vertex normals and texture coordinates and an
    image-textured triangle hangs on the back wall; image_material: the world has an image material that no primitive uses, which makes it an EXT 2 world under
    any background.  background: None (mode 0), a colour (mode 1) or ("map", image, rotate_y) (mode 2)."""
    s = p.Scene()
    white, red = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05))
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), white)
    s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), white)
    s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), red)
    s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 10, 0), white)
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 10, 0), white)
    s.MakeQuad((3.5, 9.9, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    s.MakeSphere((2, 7.5, 7), 0.6, s.DiffuseLight((20, 14, 6)))
    glass, fuzzy, checker = s.Dielectric((1, 1, 1), 1.5), s.Metal((0.7, 0.6, 0.5), 0.4), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5)
    s.MakeMovingSphere((2, 2, 7.5), (2, 2.9, 7.5), 0.8, s.Lambertian((0.2, 0.4, 0.8)))
    if tri:
        m = TW.mesh_io()
        kw_ico, kw_tet = {}, {}
        if tables:
            v, f = m.icosphere(1)
            kw_ico = {"normals": v, "uvs": (np.random.default_rng(4).random((len(v), 2)) * 1.5 - 0.25).astype(F)}
        s.MakeMesh(*m.icosphere(1), glass, 1.3, 0.0, (5, 3.6, 7), **kw_ico)
        s.MakeMesh(*m.tetrahedron(), fuzzy, 1.3, 45.0, (8, 6, 7.5), **kw_tet)
        s.MakeTriangle((4, 0.05, 2.5), (6.5, 0.05, 2), (5, 2.5, 4), checker)
        if tables:
            from _nee_worlds import small_image
            s.set_image(small_image())
            s.MakeTriangle((0.8, 5.2, 9.9), (3.3, 5.2, 9.9), (0.8, 7.7, 9.9), s.ImageTexture(), uvs=[(0.1, 0.2), (0.9, 0.1), (0.3, 0.8)])
            s.MakeTriangle((0.2, 6, 3), (0.2, 8, 5), (0.2, 6, 7), s.DiffuseLight((5, 9, 5)))
    else:
        s.MakeSphere((5, 3.6, 7), 1.3, glass)
        s.MakeSphere((8, 6, 7.5), 1.0, fuzzy)
        s.MakeSphere((5, 1.2, 3.5), 1.2, checker)
    if image_material:
        from _nee_worlds import small_image
        s.set_image(small_image())
        s.ImageTexture()
    if isinstance(background, tuple) and background[0] == "map":
        s.set_environment(background[1], rotate_y=background[2])
    else:
        s.set_background(background)
    if as_list:
        s.MakeHittableList()
    else:
        s.set_traversal(traversal)
        getattr(s, builder)()
    return s


# the eight stack-walk and list families of render_kernel_stream at EXT 2, with the recipe (variant, environment) that reaches each: _tri_worlds' table
EXT2_FORMS = [f for f in TW.FORMS if f[2] == 2]
QUEUE_FORM = {"kernel": "stream", "exact": 1, "filter": 0, "world": 3, "ext": 2, "big": 1, "wide": 1, "tol": 0, "nee": 0}   # RT_WORLD_BVH_QUEUE: the ninth plain key


# ---- a real map against the whole-sample twin --------------------------------------------------------------------------------------------------------------
SKY_U0_DEGREES = 108.0   # u0 = 0.3


def sky_map():
    pkg()
    from ray_tracing_v06_amd import image_io
    env = image_io.sky_environment(32, 16)
    env.setflags(write=False)
    return env


def sky_room(p, hidden_triangle=False, as_list=False, traversal=0, builder="BuildBVH_SAH"):
    """Lambertian, checker and metal spheres on a parallelogram under sky_environment(32, 16) turned by u0 = 0.3: all the twin follows.
    hidden_triangle: plus a tiny triangle below the middle of the ground, where no ray of this world arrives (a segment from a point above the ground to it
    crosses the ground), which makes the world a TRI world and changes no sample."""
    s = p.Scene()
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    s.MakeSphere((5, 1.5, 7), 1.5, s.Metal((0.8, 0.8, 0.9), 0.05))
    s.MakeSphere((2.2, 1.0, 5.5), 1.0, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeSphere((8, 1.2, 6), 1.2, s.Metal((0.9, 0.7, 0.4), 0.3))
    s.MakeSphere((5, 0.6, 3.5), 0.6, s.Lambertian((0.3, 0.4, 0.8)))
    if hidden_triangle:
        s.MakeTriangle((5, -1, 5), (5.01, -1, 5), (5, -1, 5.01), s.Lambertian((0.5, 0.5, 0.5)))
    s.set_environment(sky_map(), rotate_y=SKY_U0_DEGREES)
    if as_list:
        s.MakeHittableList()
    else:
        s.set_traversal(traversal)
        getattr(s, builder)()
    return s


class SkyRoomRun:
    def __init__(self):
        p = pkg()
        self.scene = sky_room(p)
        env, u0 = self.scene.environment()
        assert u0 == F(0.3)
        self.stats = {}
        samples, followed = ET.frame_samples(as_oracle_world(self.scene.getWorldPtr()), as_oracle_camera(camera(p)), W, H, SPP, DEPTH, SEED,
                                             ET.sky_environment(env, u0), stats=self.stats)
        self.samples, self.followed = samples, followed
        self.frame = ET.resolve(ET.in_order_sums(np.where(followed[..., None], samples, 0)), SPP)
        for a in (self.samples, self.followed, self.frame):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def sky_room_run():
    return SkyRoomRun()
