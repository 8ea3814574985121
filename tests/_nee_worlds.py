"""The worlds of the light-sampling tests and the matrix of kernel forms they must reach — test infrastructure only.

FORMS is the suite's statement of which light-sampling instantiations of render_kernel_stream exist: one (world, exact, ext, big, wide) tuple per
form of the NEE family of csrc/rt_device.hip's kernel table, each with the recipe — world kind, kernel variant, environment — that makes a renderer resolve to it.
tests/test_light_sampling_cpu.py holds the set against the source and every world against the conditions it is there for (run(name).stats), without
a GPU; tests/test_gpu_light_sampling.py renders each form and compares it with the twin's run of its world (tests/_nee_twin.py).

Every world is built through the product's host vocabulary, which needs no device; run(name) is the twin's samples of it, computed once per process.
"""
import functools

import numpy as np

import _nee_twin as T
from _common import as_oracle_camera, as_oracle_world, pkg

SEED = 1984
BVH, LIST = "RT_WORLD_BVH", "RT_WORLD_LIST"
WORLD_ID = {BVH: 0, LIST: 1}   # RT_WORLD_BVH, RT_WORLD_LIST of include/rt06.h
LDS, NARROW, WIDE = {}, {"RT06_FORCE_BIG": "1"}, {"RT06_FORCE_BIG": "1", "RT06_FORCE_WIDE": "1"}

# (world, exact, ext, big, wide) -> (world name, kernel variant, environment)
FORMS = {
    (BVH, 0, 1, 0, 0): ("room", 3, LDS),     (BVH, 1, 1, 0, 0): ("room", 2, LDS),
    (BVH, 0, 1, 1, 0): ("room", 3, NARROW),  (BVH, 1, 1, 1, 0): ("room", 2, NARROW),
    (BVH, 0, 1, 1, 1): ("room", 3, WIDE),    (BVH, 1, 1, 1, 1): ("room", 2, WIDE),
    (BVH, 0, 2, 0, 0): ("textured_room", 3, LDS),     (BVH, 1, 2, 0, 0): ("textured_room", 2, LDS),
    (BVH, 0, 2, 1, 0): ("textured_room", 3, NARROW),  (BVH, 1, 2, 1, 0): ("textured_room", 2, NARROW),
    (BVH, 0, 2, 1, 1): ("textured_room", 3, WIDE),    (BVH, 1, 2, 1, 1): ("textured_room", 2, WIDE),
    (LIST, 1, 1, 0, 0): ("room_list", 0, LDS),           (LIST, 1, 1, 1, 1): ("room_list", 0, NARROW),
    (LIST, 1, 2, 0, 0): ("textured_room_list", 0, LDS),  (LIST, 1, 2, 1, 1): ("textured_room_list", 0, NARROW),
}


def form_id(form):
    world, exact, ext, big, wide = form
    return f"{world[9:].lower()}-{'exact' if exact else 'fast'}-ext{ext}-{('lds', 'narrow', 'wide')[big + wide]}"


def kernel_form_of(form, nee=1):
    """what Renderer.kernel_form() reports for a FORMS key"""
    world, exact, ext, big, wide = form
    return {"kernel": "stream", "exact": exact, "filter": 0, "world": WORLD_ID[world], "ext": ext, "big": big, "wide": wide, "tol": 0, "nee": nee}


def small_image(h=12, w=24):
    """a small picture with a gradient in two channels and a chequerboard in the third (tests/test_gpu_cornell.py's, smaller)"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3), np.uint8)
    img[..., 0] = (xx * 255 // (w - 1)).astype(np.uint8)
    img[..., 1] = (yy * 255 // (h - 1)).astype(np.uint8)
    img[..., 2] = (((xx // 4) + (yy // 4)) % 2 * 200 + 30).astype(np.uint8)
    return img


def _shell(s, floor, walls, left=None, right=None):
    """a closed 10 x 10 x 10 room seen from inside"""
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), floor)
    s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), walls)                          # ceiling
    s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), walls if left is None else left)
    s.MakeQuad((10, 0, 0), (0, 10, 0), (0, 0, 10), walls if right is None else right)
    s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 10, 0), walls)                          # back
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 10, 0), walls)                           # front, behind the camera


def two_light_room(p, textured=False, as_list=False, irregular=False):
    """a closed 6-quad room seen from inside, two quad lights of different size (one skew), a metal, a checker and a dielectric sphere;
    textured: plus a noise-textured sphere and an image-textured quad with their tables (the EXT = 2 kernels); as_list: left a HittableList;
    irregular: plus a sphere whose box has a coordinate outside the fast-division class (1e-15), which variant 0 answers with the verbatim kernel"""
    s = p.Scene()
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    light_a, light_b = s.DiffuseLight((8, 8, 8)), s.DiffuseLight((20, 14, 6))
    _shell(s, white, white, red, green)
    s.MakeQuad((2, 9.9, 3), (2, 0, 0), (0, 0, 2), light_a)
    s.MakeQuad((6.5, 9.5, 6), (1, 0.2, 0), (0, 0.1, 0.7), light_b)
    s.MakeSphere((3, 1.5, 6), 1.5, s.Metal((0.8, 0.8, 0.9), 0.1))
    s.MakeSphere((7, 1.2, 5), 1.2, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    s.MakeSphere((5, 1, 3), 1.0, s.Dielectric((1, 1, 1), 1.5))
    if textured:
        s.set_perlin(1984).set_image(small_image())
        s.MakeSphere((8.8, 0.6, 8.5), 0.6, s.NoiseTexture(4.0))
        s.MakeQuad((0.8, 0.2, 9.9), (1.2, 0, 0), (0, 0.9, 0), s.ImageTexture())
    if irregular:
        s.MakeSphere((2e-15, 0.4, 1.0), 1e-15, white)   # box min.x = 1e-15: not 0 and below 2^-40
    if as_list:
        s.MakeHittableList()
    else:
        s.BuildBVH_SAH()
    return s


def sixteen_light_room(p):
    """the light table at its limit: 16 small quad lights of different sizes, every third one skew, on the ceiling, the left and the back wall of a
    closed room with a checker floor, a Lambertian and a checker sphere"""
    s = p.Scene()
    white, blue = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.2, 0.3, 0.7))
    checker = s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.8)
    _shell(s, checker, white, blue)
    for i in range(16):
        emit = s.DiffuseLight((6 + i, 14 - 0.5 * i, 4 + 0.7 * (i % 5)))
        a, b = 0.4 + 0.07 * i, 0.9 - 0.04 * i                     # side lengths: every light has its own area
        k = 0.15 * a if i % 3 == 2 else 0.0                       # skew: out of the wall's plane and off the axes
        if i < 8:      # ceiling, two rows
            s.MakeQuad((0.8 + 1.1 * i, 9.8, 3 + 3 * (i % 2)), (a, k, 0), (k, 0, b), emit)
        elif i < 12:   # left wall
            s.MakeQuad((0.2, 3 + 1.5 * (i - 8), 2 + 1.8 * (i - 8)), (k, a, 0), (0, k, b), emit)
        else:          # back wall
            s.MakeQuad((1 + 2.2 * (i - 12), 2 + 1.6 * (i - 12), 9.8), (a, k, 0), (0, b, -k), emit)
    s.MakeSphere((6.5, 1.3, 6), 1.3, white)
    s.MakeSphere((3, 1, 4), 1.0, s.LambertianTexture((0.8, 0.2, 0.2), (0.9, 0.9, 0.6), 0.4))
    s.BuildBVH_SAH()
    return s


def stacked_lights_room(p):
    """two parallel quad lights over the middle of the floor, the upper one larger: a direction from the floor through the lower one meets both,
    so the density of a cosine-half direction has two light terms"""
    s = p.Scene()
    white = s.Lambertian((0.73, 0.73, 0.73))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 1.0), white)
    s.MakeQuad((3.5, 6, 4), (3, 0, 0), (0, 0, 3), s.DiffuseLight((6, 6, 6)))
    s.MakeQuad((2, 8.5, 2.5), (6, 0, 0), (0, 0, 6), s.DiffuseLight((3, 5, 9)))
    s.MakeSphere((2, 1, 7), 1.0, white)
    s.BuildBVH_TopDown()
    return s


def lights_behind_surfaces(p):
    """under the sky: a light lower than a Lambertian table top (from the top every sampled light point is below the surface: pdf_cos == 0) and a
    light in the plane of the floor quad beside it (from the floor the direction to it lies in its plane: quad::hit's |denom| < 1e-8 rejects it, or
    an ulp off the plane grazes it)"""
    s = p.Scene()
    grey, sand = s.Lambertian((0.6, 0.6, 0.6)), s.Lambertian((0.7, 0.6, 0.4))
    s.MakeQuad((0, 0, 0), (6, 0, 0), (0, 0, 10), sand)                               # floor
    s.MakeQuad((6.5, 0, 3), (2.5, 0, 0), (0, 0, 3), s.DiffuseLight((9, 9, 9)))       # in the floor's plane
    s.MakeQuad((1, 2, 4), (4, 0, 0), (0, 0, 3), grey)                                # table top
    s.MakeQuad((6.5, 1, 7), (2, 0, 0), (0, 0, 2), s.DiffuseLight((12, 8, 4)))        # lower than the table top
    s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 6, 0), grey)                              # a wall behind
    s.BuildBVH_TopDown()
    return s


def moving_world(p):
    """moving spheres under a quad light, for a motion-blur camera: outside the twin's scope (pinhole only), compared across forms and variants"""
    s = p.Scene()
    s.MakeSphere((0, -100.5, -1), 100.0, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.6))
    s.MakeMovingSphere((-1.2, 0.0, -1.5), (-1.2, 0.4, -1.5), 0.5, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeMovingSphere((0.0, 0.0, -1.0), (0.3, 0.0, -1.2), 0.5, s.Metal((0.8, 0.8, 0.8), 0.2))
    s.MakeSphere((1.2, 0.0, -1.2), 0.5, s.Dielectric((1, 1, 1), 1.5))
    s.MakeQuad((-1, 2.5, -2), (2, 0, 0), (0, 0.3, 1.5), s.DiffuseLight((10, 10, 8)))
    s.set_background((0.05, 0.05, 0.08))
    s.BuildBVH_SAH()
    return s


# name -> (builder, camera arguments (lookfrom, lookat, vfov), W, H, max depth, quad lights); every run is 4 samples per pixel, pinhole
SPP = 4
ROOM_VIEW = ((5, 5, 0.5), (5, 4, 10), 80.0)
WORLDS = {
    "room": (two_light_room, ROOM_VIEW, 32, 32, 8, 2),
    "textured_room": (functools.partial(two_light_room, textured=True), ROOM_VIEW, 32, 32, 8, 2),
    "room_list": (functools.partial(two_light_room, as_list=True), ROOM_VIEW, 32, 32, 8, 2),
    "textured_room_list": (functools.partial(two_light_room, textured=True, as_list=True), ROOM_VIEW, 32, 32, 8, 2),
    "irregular_room": (functools.partial(two_light_room, irregular=True), ROOM_VIEW, 32, 32, 8, 2),
    "sixteen_lights": (sixteen_light_room, ROOM_VIEW, 32, 32, 8, 16),
    "stacked_lights": (stacked_lights_room, ((5, 3, 0.5), (5, 3, 10), 90.0), 32, 24, 8, 2),
    "lights_behind": (lights_behind_surfaces, ((4.5, 5, -3), (4.5, 0.5, 5), 70.0), 32, 24, 8, 2),
}
WORLDS["clamped_index"] = (sixteen_light_room, ROOM_VIEW, 16, 16, 8, 16)
# the uniforms are k 2^-24, k in [1, 2^24]: a light-index draw of exactly 1, where uint(u * n_l) = n_l and only the clamp keeps the index in the table, is one
# draw in 2^24.  Under this seed sample 2 of pixel 227 of a 16 x 16 frame has it as its fourth uniform — behind an accepted jitter pair and a mixture draw
# below 0.5 — (found by a search over seeds with orc_rng_uniforms; tests/test_light_sampling_cpu.py holds the twin's count to it)
SEEDS = {"clamped_index": 3497}
MATRIX_WORLDS = ("room", "textured_room", "room_list", "textured_room_list")
EDGE_WORLDS = ("sixteen_lights", "stacked_lights", "lights_behind", "clamped_index")


class Run:
    """a world, its camera and the twin's samples of it with light sampling on; nothing here is modified after it is made"""

    def __init__(self, name):
        build, (lookfrom, lookat, vfov), self.W, self.H, self.depth, self.lights = WORLDS[name]
        p = pkg()
        self.name, self.spp, self.seed = name, SPP, SEEDS.get(name, SEED)
        self.scene = build(p)
        self.cam = p.PinholeCamera(lookfrom, lookat, (0, 1, 0), vfov, self.W / self.H)
        self.stats = T.new_stats()
        self.samples, followed = T.frame_samples(as_oracle_world(self.scene.getWorldPtr()), as_oracle_camera(self.cam), self.W, self.H, SPP, self.depth, self.seed,
                                                 light_sampling=True, stats=self.stats)
        self.followed = followed.all(axis=2)   # pixels whose every sample the twin followed to its end
        self.sums = T.in_order_sums(np.where(followed[..., None], self.samples, 0))   # exact where `followed`; elsewhere not the frame's
        for a in (self.samples, self.followed, self.sums):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(name):
    return Run(name)
