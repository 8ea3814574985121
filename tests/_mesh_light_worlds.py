"""The worlds of the triangle- and mesh-light tests (mode 4) — test infrastructure only, beside tests/_tri_worlds.py, which stays §18's.

Every world is built through the product's host vocabulary, which needs no device, and holds only what tests/_mesh_light_twin.py follows; run(name, mode) is the
twin's samples of it, computed once per process and never modified.  tests/test_mesh_lights_cpu.py holds every world to what it is there for, by the twin's own
counts, without a GPU; tests/test_gpu_mesh_lights.py renders them and compares every pixel.
"""
import functools

import numpy as np

import _mesh_light_twin as MT
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg
from _nee_worlds import SEEDS, _shell

SEED, SPP, DEPTH = TW.SEED, TW.SPP, TW.DEPTH


def lit_room(p, lights, as_list=False):
    """tri_room's closed 10 x 10 x 10 shell with a checker floor, a red tetrahedron, a metal icosphere(1) and a Lambertian sphere, and NO light but what
    lights(s) adds"""
    s = p.Scene()
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    _shell(s, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5), white, red, green)
    m = TW.mesh_io()
    s.MakeMesh(*m.tetrahedron(), red, 1.6, 20.0, (3, 1.4, 6))
    s.MakeMesh(*m.icosphere(1), s.Metal((0.8, 0.8, 0.9), 0.1), 1.5, 0.0, (7, 1.6, 5.5))
    s.MakeSphere((5, 1.0, 3.5), 1.0, white)
    lights(s)
    if as_list:
        s.MakeHittableList()
    else:
        s.BuildBVH_SAH()
    return s


def _one_triangle(s):
    s.MakeTriangle((3.5, 9.5, 4), (6.5, 9.7, 4.5), (5, 9.2, 7), s.DiffuseLight((14, 12, 9)))


def _mesh_lamp(s):
    s.MakeMesh(*TW.mesh_io().icosphere(0), s.DiffuseLight((18, 15, 10)), 0.8, 15.0, (5, 7.5, 5.5))


def _tetrahedron_lamp(s, scale=1.2, emit=(12, 10, 8)):
    s.MakeMesh(*TW.mesh_io().tetrahedron(), s.DiffuseLight(emit), scale, 35.0, (5, 7.2, 5.5))


def _free_triangles(n):
    """n triangle lights of different areas: rows under the ceiling, then along the back and the left wall"""
    def lights(s):
        for i in range(n):
            emit = s.DiffuseLight((4 + 0.1 * i, 9 - 0.08 * i, 3 + 0.5 * (i % 7)))
            e = 0.25 + 0.012 * i   # the edge grows with the index: no two areas are equal
            if i < 40:
                x, z = 0.8 + 1.1 * (i % 8), 1.5 + 1.6 * (i // 8)
                s.MakeTriangle((x, 9.6, z), (x + e, 9.6, z + 0.1), (x + 0.1, 9.6 - 0.2, z + e), emit)
            elif i < 56:
                x, y = 0.7 + 1.1 * ((i - 40) % 8), 5.5 + 1.7 * ((i - 40) // 8)
                s.MakeTriangle((x, y, 9.7), (x + e, y + 0.1, 9.7), (x + 0.1, y + e, 9.6), emit)
            else:
                y, z = 4 + 0.6 * (i - 56), 2 + 0.8 * (i - 56)
                s.MakeTriangle((0.3, y, z), (0.3, y + e, z + 0.1), (0.4, y + 0.1, z + e), emit)
    return lights


def three_kinds(p, as_list=False, textured=False):
    """a quad light, a sphere lamp and a triangle light in one table (tri_room's own: n_l = 3 in mode 4, 2 in mode 2, 1 in mode 1)"""
    return TW.tri_room(p, as_list=as_list, lamp=True, tri_light=True, textured=textured)


# name -> (builder, W, H, lights of mode 4)
WORLDS = {
    "triangle_lit": (functools.partial(lit_room, lights=_one_triangle), 32, 32, 1),        # one light: no index draw; modes 1 and 2 refuse it
    "triangle_lit_list": (functools.partial(lit_room, lights=_one_triangle, as_list=True), 32, 32, 1),
    "three_kinds": (three_kinds, 32, 32, 3),
    "three_kinds_list": (functools.partial(three_kinds, as_list=True), 32, 32, 3),
    "three_kinds_textured": (functools.partial(three_kinds, textured=True), 32, 32, 3),
    "three_kinds_textured_list": (functools.partial(three_kinds, textured=True, as_list=True), 32, 32, 3),
    "mesh_lamp": (functools.partial(lit_room, lights=_mesh_lamp), 32, 32, 20),             # a closed emissive icosphere(0)
    "tetrahedron_lamp": (functools.partial(lit_room, lights=_tetrahedron_lamp), 32, 32, 4),
    "sixty_four": (functools.partial(lit_room, lights=_free_triangles(64)), 32, 32, 64),
    "sixty_five": (functools.partial(lit_room, lights=_free_triangles(65)), 32, 32, 65),   # refused: it has no run
    # _nee_worlds.SEEDS["clamped_index"]: under that seed sample 2 of pixel 227 of a 16 x 16 frame has the uniform 1 as its fourth draw, behind an accepted jitter
    # pair and a mixture draw below 0.5 — a property of the stream alone, so it serves any world of more than one light whose pixel 227 first meets a Lambertian
    "clamped_triangle_index": (functools.partial(lit_room, lights=_free_triangles(64)), 16, 16, 64),
    "plain_lamp": (functools.partial(TW.tri_room, lamp=True), 32, 32, 2),                  # triangles, but no triangle light: mode 4's table is mode 2's
}
SEEDS4 = {"clamped_triangle_index": SEEDS["clamped_index"]}
EDGE_WORLDS = ("three_kinds", "mesh_lamp", "tetrahedron_lamp", "sixty_four", "triangle_lit", "clamped_triangle_index")


def scene(name):
    return WORLDS[name][0](pkg())


class Run:
    """a world, its camera and the twin's samples of it in `mode`; nothing here is modified after it is made"""

    def __init__(self, name, mode):
        build, self.W, self.H, self.lights = WORLDS[name]
        p = pkg()
        self.name, self.mode, self.spp, self.depth, self.seed = name, mode, SPP, DEPTH, SEEDS4.get(name, SEED)
        self.scene = build(p)
        self.cam = TW.camera(p, self.W, self.H)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        self.stats = MT.new_stats()
        self.samples, followed = MT.frame_samples(self.world, as_oracle_camera(self.cam), self.W, self.H, SPP, DEPTH, self.seed, mode=mode, stats=self.stats)
        self.pixel_followed = followed.all(axis=2)
        self.followed = bool(followed.all())
        self.sums = MT.in_order_sums(np.where(followed[..., None], self.samples, 0))
        self.frame = MT.resolve(self.sums, SPP)
        for a in (self.samples, self.sums, self.frame, self.pixel_followed):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(name, mode=4):
    return Run(name, mode)
