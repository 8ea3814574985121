"""The worlds of the sphere-light tests (mode 2) — test infrastructure only, beside tests/_nee_worlds.py, which stays §16's.

Every world is built through the product's host vocabulary, which needs no device; run(name) is the mode-2 twin's samples of it (tests/_nee2_twin.py),
computed once per process and never modified.  tests/test_light_sampling_spheres_cpu.py holds every world to what it is there for, by the twin's own
counts, without a GPU; tests/test_gpu_light_sampling_spheres.py renders them and compares every pixel.
"""
import functools

import numpy as np

import _nee2_twin as T2
from _common import as_oracle_camera, as_oracle_world, pkg
from _nee_worlds import ROOM_VIEW, SEEDS, _shell, small_image

SEED = 1984
SPP = 4


def lamp_room(p, as_list=False):
    """a closed 6-quad room seen from inside with ONE light, a sphere: no quad light, so mode 1 refuses it; a metal, a checker and a Lambertian sphere"""
    s = p.Scene()
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5), white, red, green)
    s.MakeSphere((5, 7.5, 5.5), 0.8, s.DiffuseLight((20, 18, 14)))
    s.MakeSphere((3, 1.5, 6), 1.5, s.Metal((0.8, 0.8, 0.9), 0.1))
    s.MakeSphere((7, 1.2, 5), 1.2, white)
    if as_list:
        s.MakeHittableList()
    else:
        s.BuildBVH_SAH()
    return s


def mixed_room(p, as_list=False, textured=False):
    """the same room lit by a sphere AND a skew quad light (and a moving sphere with a light material, which emits and is in no table):
    mode 1 samples the quad alone, mode 2 both; textured: plus a noise-textured sphere and an image-textured quad (the EXT = 2 kernels), which
    the twin does not follow"""
    s = p.Scene()
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5), white, red, green)
    s.MakeSphere((7, 1.2, 5), 1.2, white)
    s.MakeSphere((3.5, 7, 6), 0.7, s.DiffuseLight((24, 20, 12)))
    s.MakeQuad((6.5, 9.5, 4), (1.5, 0.2, 0), (0, 0.1, 1.2), s.DiffuseLight((8, 10, 14)))
    s.MakeMovingSphere((8.5, 8, 8), (8.5, 8.4, 8), 0.4, s.DiffuseLight((5, 12, 5)))
    s.MakeSphere((3, 1.5, 6), 1.5, s.Metal((0.8, 0.8, 0.9), 0.1))
    if textured:
        s.set_perlin(1984).set_image(small_image())
        s.MakeSphere((8.8, 0.6, 8.5), 0.6, s.NoiseTexture(4.0))
        s.MakeQuad((0.8, 0.2, 9.9), (1.2, 0, 0), (0, 0.9, 0), s.ImageTexture())
    if as_list:
        s.MakeHittableList()
    else:
        s.BuildBVH_SAH()
    return s


def sphere_world(p):
    """no quad at all (n_quads = 0: the light table lies directly at `quads`): a ground sphere, three spheres on it and two sphere lights under a dim constant sky"""
    s = p.Scene()
    s.MakeSphere((0, -100.5, -1), 100.0, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.6))
    s.MakeSphere((-1.1, 0.0, -1.4), 0.5, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeSphere((1.5, 1.6, -1.0), 0.3, s.DiffuseLight((30, 26, 20)))
    s.MakeSphere((0.0, 0.0, -1.0), 0.5, s.Lambertian((0.6, 0.6, 0.7)))
    s.MakeSphere((1.1, 0.0, -1.3), 0.5, s.Metal((0.8, 0.8, 0.8), 0.2))
    s.MakeSphere((-1.6, 0.9, -2.2), 0.2, s.DiffuseLight((10, 25, 40)))
    s.set_background((0.02, 0.02, 0.03))
    s.BuildBVH_SAH()
    return s


def inside_a_light(p):
    """a floor, a table top and two spheres INSIDE one large sphere light (a luminous dome of radius 30) and a small one: from every hit point the
    dome has one crossing in front and one behind (t1 < 0 < t2)"""
    s = p.Scene()
    s.MakeQuad((-8, 0, -8), (16, 0, 0), (0, 0, 16), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 1.0))
    s.MakeQuad((-1, 1.5, 1), (3, 0, 0), (0, 0, 2), s.Lambertian((0.6, 0.6, 0.6)))
    s.MakeSphere((-2.5, 1, 2), 1.0, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeSphere((0.5, 0.4, -1), 0.4, s.Lambertian((0.3, 0.4, 0.7)))
    s.MakeSphere((0, 2, 0), 30.0, s.DiffuseLight((0.6, 0.7, 0.9)))
    s.MakeSphere((3, 3, 2), 0.5, s.DiffuseLight((12, 10, 8)))
    s.set_background((0, 0, 0))
    s.BuildBVH_TopDown()
    return s


def tangent_light(p):
    """a sphere light that touches the ceiling and one that touches the right wall of the closed room: seen along the ceiling, so that hit points
    beside the points of tangency are in view: there the light fills nearly half the sky and cc = dot(oc, oc) - r * r is what cancellation leaves"""
    s = p.Scene()
    white, blue = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.2, 0.3, 0.7))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.8), white, blue)
    s.MakeSphere((5, 9, 6), 1.0, s.DiffuseLight((10, 10, 9)))
    s.MakeSphere((9.25, 4, 7), 0.75, s.DiffuseLight((6, 9, 12)))
    s.MakeSphere((4, 1, 5), 1.0, white)
    s.BuildBVH_TopDown()
    return s


def stacked_sphere_and_quad(p):
    """a sphere light under a larger quad light: a direction from the floor through the sphere meets both, so pl has a sphere and a quad term"""
    s = p.Scene()
    white = s.Lambertian((0.73, 0.73, 0.73))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 1.0), white)
    s.MakeSphere((5, 6, 5.5), 1.0, s.DiffuseLight((9, 7, 5)))
    s.MakeQuad((2, 8.5, 2.5), (6, 0, 0), (0, 0, 6), s.DiffuseLight((3, 5, 9)))
    s.MakeSphere((2, 1, 7), 1.0, white)
    s.BuildBVH_TopDown()
    return s


def far_small_lamp(p):
    """a hall of the Cornell box's size (coordinates in the hundreds) lit by one sphere of radius 2 under its ceiling: D / r is in the hundreds, so some
    sampled points on the sphere's silhouette come out with disc <= 0 even in the cancellation-free form, and their paths end as failed scatters"""
    s = p.Scene()
    white = s.Lambertian((0.73, 0.73, 0.73))
    s.MakeQuad((0, 0, 0), (555, 0, 0), (0, 0, 555), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 40.0))
    s.MakeQuad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)
    s.MakeQuad((0, 0, 0), (0, 555, 0), (0, 0, 555), s.Lambertian((0.65, 0.05, 0.05)))
    s.MakeSphere((278, 520, 278), 2.0, s.DiffuseLight((9000, 8000, 6000)))
    s.MakeSphere((380, 60, 300), 60.0, white)
    s.set_background((0, 0, 0))
    s.BuildBVH_TopDown()
    return s


def sixteen_sphere_lights(p):
    """the table at its limit with spheres alone: 16 sphere lights of different radii along the ceiling, the left and the back wall of a closed room with a
    checker floor (n_quads = 6, no quad light)"""
    s = p.Scene()
    white, blue = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.2, 0.3, 0.7))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.8), white, blue)
    for i in range(16):
        emit = s.DiffuseLight((6 + i, 14 - 0.5 * i, 4 + 0.7 * (i % 5)))
        rad = 0.15 + 0.03 * i
        if i < 8:
            s.MakeSphere((0.9 + 1.15 * i, 9.2, 3 + 3 * (i % 2)), rad, emit)
        elif i < 12:
            s.MakeSphere((0.9, 3 + 1.5 * (i - 8), 2 + 1.8 * (i - 8)), rad, emit)
        else:
            s.MakeSphere((1.5 + 2.2 * (i - 12), 2 + 1.6 * (i - 12), 9.1), rad, emit)
    s.MakeSphere((6.5, 1.3, 6), 1.3, white)
    s.MakeSphere((3, 1, 4), 1.0, s.LambertianTexture((0.8, 0.2, 0.2), (0.9, 0.9, 0.6), 0.4))
    s.BuildBVH_SAH()
    return s


# name -> (builder, camera arguments (lookfrom, lookat, vfov), W, H, max depth, lights of mode 2); every run is 4 samples per pixel, pinhole
WORLDS = {
    "lamp_room": (lamp_room, ROOM_VIEW, 32, 32, 8, 1),
    "lamp_room_list": (functools.partial(lamp_room, as_list=True), ROOM_VIEW, 32, 32, 8, 1),
    "mixed_room": (mixed_room, ROOM_VIEW, 32, 32, 8, 2),
    "mixed_room_list": (functools.partial(mixed_room, as_list=True), ROOM_VIEW, 32, 32, 8, 2),
    "textured_mixed_room": (functools.partial(mixed_room, textured=True), ROOM_VIEW, 32, 32, 8, 2),
    "textured_mixed_room_list": (functools.partial(mixed_room, textured=True, as_list=True), ROOM_VIEW, 32, 32, 8, 2),
    "far_small_lamp": (far_small_lamp, ((278, 278, -500), (278, 200, 278), 50.0), 32, 24, 8, 1),
    "sphere_world": (sphere_world, ((0, 1.2, 2.5), (0, 0.2, -1.2), 60.0), 32, 24, 8, 2),
    "inside_a_light": (inside_a_light, ((0, 4, -9), (0, 1, 1), 60.0), 32, 24, 8, 2),
    "tangent_light": (tangent_light, ((3.5, 9.6, 0.5), (6, 9.0, 8), 70.0), 32, 32, 8, 2),
    "stacked_sphere_and_quad": (stacked_sphere_and_quad, ((5, 3, 0.5), (5, 3, 10), 90.0), 32, 24, 8, 2),
    "sixteen_sphere_lights": (sixteen_sphere_lights, ROOM_VIEW, 32, 32, 8, 16),
    # _nee_worlds.SEEDS["clamped_index"]: under that seed sample 2 of pixel 227 of a 16 x 16 frame has the uniform 1 as its fourth draw, behind an accepted
    # jitter pair and a mixture draw below 0.5 — a property of the stream alone, so it serves any 16-light world whose pixel 227 first meets a Lambertian
    "clamped_sphere_index": (sixteen_sphere_lights, ROOM_VIEW, 16, 16, 8, 16),
}
SEEDS2 = {"clamped_sphere_index": SEEDS["clamped_index"]}
ROOM_WORLDS = ("lamp_room", "mixed_room", "sphere_world")                 # compared in every memory form, variant and cut
LIST_WORLDS = ("lamp_room_list", "mixed_room_list")
TEXTURED_WORLDS = ("textured_mixed_room", "textured_mixed_room_list")      # the EXT = 2 forms; compared where the twin follows, and across forms elsewhere
EDGE_WORLDS = ("far_small_lamp", "inside_a_light", "tangent_light", "stacked_sphere_and_quad", "sixteen_sphere_lights", "clamped_sphere_index")


class Run:
    """a world, its camera and the twin's samples of it in mode 2; nothing here is modified after it is made"""

    def __init__(self, name):
        build, (lookfrom, lookat, vfov), self.W, self.H, self.depth, self.lights = WORLDS[name]
        p = pkg()
        self.name, self.spp, self.seed = name, SPP, SEEDS2.get(name, SEED)
        self.scene = build(p)
        self.cam = p.PinholeCamera(lookfrom, lookat, (0, 1, 0), vfov, self.W / self.H)
        self.stats = T2.new_stats()
        self.samples, followed = T2.frame_samples(as_oracle_world(self.scene.getWorldPtr()), as_oracle_camera(self.cam), self.W, self.H, SPP, self.depth, self.seed,
                                                  mode=2, stats=self.stats)
        self.followed = followed.all(axis=2)
        self.sums = T2.in_order_sums(np.where(followed[..., None], self.samples, 0))
        for a in (self.samples, self.followed, self.sums):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(name):
    return Run(name)
