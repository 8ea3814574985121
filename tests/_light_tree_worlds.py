"""The worlds of the light-tree tests (mode 16) — test infrastructure only, beside tests/_mesh_light_worlds.py, which stays §19's.

Every world is built through the product's host vocabulary, which needs no device, and holds only what tests/_light_tree_twin.py follows; run(name, mode) is the
twin's samples of it, computed once per process and never modified.  tests/test_light_tree_cpu.py holds every world to what it is there for without a GPU;
tests/test_gpu_light_tree.py renders them and compares every pixel.
"""
import functools

import numpy as np

import _light_tree_twin as LT
import _mesh_light_worlds as MW
import _nee2_worlds as NW2
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg
from _nee_worlds import SEEDS

SEED, SPP, DEPTH = TW.SEED, TW.SPP, TW.DEPTH


def _two_triangles(s):
    s.MakeTriangle((3.5, 9.5, 4), (6.5, 9.7, 4.5), (5, 9.2, 7), s.DiffuseLight((14, 12, 9)))
    s.MakeTriangle((0.3, 5, 3), (0.3, 7, 4), (0.4, 5.5, 6), s.DiffuseLight((4, 8, 12)))


def _coincident(s):
    """two triangles with the same vertices (equal centroids on every axis: the sort keeps mode 4's order) and a third elsewhere"""
    emit = s.DiffuseLight((7, 6, 5))
    s.MakeTriangle((3.5, 9.5, 4), (6.5, 9.5, 4.5), (5, 9.5, 7), emit)
    s.MakeTriangle((3.5, 9.5, 4), (6.5, 9.5, 4.5), (5, 9.5, 7), emit)
    s.MakeTriangle((0.3, 5, 3), (0.3, 7, 4), (0.4, 5.5, 6), s.DiffuseLight((4, 8, 12)))


def _areas_1_to_10000(s):
    """two similar triangles under the ceiling, edges 0.03 and 3: areas 1 : 10^4"""
    s.MakeTriangle((2, 9.5, 3), (5, 9.5, 3), (2, 9.5, 6), s.DiffuseLight((3, 3, 3)))
    s.MakeTriangle((7, 9.5, 7), (7.03, 9.5, 7), (7, 9.5, 7.03), s.DiffuseLight((900, 600, 300)))


def _icosphere_lamp(level, scale=0.8, emit=(18, 15, 10)):
    def lights(s):
        s.MakeMesh(*TW.mesh_io().icosphere(level), s.DiffuseLight(emit), scale, 15.0, (5, 7.5, 5.5))
    return lights


def panel(n):
    """E10's panel: an n-triangle strip under the ceiling (n even: n / 2 cells of two triangles), 4 x 2 in all"""
    def lights(s):
        emit = s.DiffuseLight((10, 10, 10))
        cells = max(n // 2, 1)
        w = 4.0 / cells
        for c in range(cells):
            x = 3 + c * w
            s.MakeTriangle((x, 9.8, 4), (x + w, 9.8, 4), (x, 9.8, 6), emit)
            if 2 * c + 1 < n:
                s.MakeTriangle((x + w, 9.8, 6), (x, 9.8, 6), (x + w, 9.8, 4), emit)
    return lights


def _mixed(s):
    """a quad light, a sphere lamp and a closed icosphere(1): the pin's mixed table (82 lights)"""
    s.MakeQuad((3.5, 9.9, 1), (3, 0, 0), (0, 0, 1.5), s.DiffuseLight((8, 8, 8)))
    s.MakeSphere((2, 7.5, 7), 0.6, s.DiffuseLight((20, 14, 6)))
    _icosphere_lamp(1, 0.7)(s)


def no_triangles(p):
    """tri_room without any triangle, with its quad light and the sphere lamp: n_plain_quads == n_quads"""
    return TW.tri_room(p, plain=True, lamp=True)


def far_small_lamp(p):
    """_nee2_worlds' hall lit by one small far sphere: drawn points lost on the silhouette; no triangle either"""
    return NW2.far_small_lamp(p)


lit = lambda lights, **kw: functools.partial(MW.lit_room, lights=lights, **kw)   # noqa: E731
ROOM = (TW.VIEW, 32, 32)
# name -> (builder, (view, W, H), lights of mode 16)
WORLDS = {
    "one": (lit(MW._one_triangle), ROOM, 1),                       # the root is a leaf; no draw
    "two": (lit(_two_triangles), ROOM, 2),
    "three_kinds": (MW.three_kinds, ROOM, 3),                      # unbalanced: a leaf and a pair
    "three_kinds_list": (functools.partial(MW.three_kinds, as_list=True), ROOM, 3),
    "three_kinds_textured": (functools.partial(MW.three_kinds, textured=True), ROOM, 3),
    "three_kinds_textured_list": (functools.partial(MW.three_kinds, textured=True, as_list=True), ROOM, 3),
    "mesh_lamp": (lit(MW._mesh_lamp), ROOM, 20),                   # a closed icosphere(0): both crossings
    "sixty_four": (lit(MW._free_triangles(64)), ROOM, 64),
    "sixty_five": (lit(MW._free_triangles(65)), ROOM, 65),         # what mode 4 refuses
    "icosphere2": (lit(_icosphere_lamp(2)), ROOM, 320),
    "tie": (lit(_coincident), ROOM, 3),
    "silhouette": (far_small_lamp, (((278, 278, -500), (278, 200, 278), 50.0), 32, 24), 1),
    "clamped_last_index": (lit(MW._free_triangles(64)), (TW.VIEW, 16, 16), 64),   # _nee_worlds.SEEDS["clamped_index"]: the index draw is the uniform 1, x = A
    "areas": (lit(_areas_1_to_10000), ROOM, 2),
    "no_triangles": (no_triangles, ROOM, 2),
    "icosphere1": (lit(_icosphere_lamp(1, 1.0, (12, 10, 8))), ROOM, 80),   # the expectation's room
    "panel64": (lit(panel(64)), ROOM, 64),
    "mixed": (lit(_mixed), ROOM, 82),
}
SEEDS16 = {"clamped_last_index": SEEDS["clamped_index"]}
SHAPE_WORLDS = ("one", "two", "three_kinds", "mesh_lamp", "sixty_four", "sixty_five", "icosphere2", "tie", "silhouette", "clamped_last_index", "areas")
HOST_WORLDS = ("one", "two", "three_kinds", "mesh_lamp", "sixty_five", "icosphere2", "tie", "mixed", "areas", "no_triangles", "silhouette")
PIN_WORLDS = ("icosphere2", "panel64", "mixed")


@functools.lru_cache(maxsize=None)
def scene(name):
    return WORLDS[name][0](pkg())


def camera(name):
    (lookfrom, lookat, vfov), W, H = WORLDS[name][1]
    return pkg().PinholeCamera(lookfrom, lookat, (0, 1, 0), vfov, W / H)


class Run:
    """a world, its camera and the twin's samples of it in `mode`; nothing here is modified after it is made"""

    def __init__(self, name, mode):
        _, (_, self.W, self.H), self.lights = WORLDS[name]
        self.name, self.mode, self.spp, self.depth, self.seed = name, mode, SPP, DEPTH, SEEDS16.get(name, SEED)
        self.scene = scene(name)
        self.cam = camera(name)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        self.stats = {}
        self.samples, followed = LT.frame_samples(self.world, as_oracle_camera(self.cam), self.W, self.H, SPP, DEPTH, self.seed, mode=mode, stats=self.stats)
        self.pixel_followed = followed.all(axis=2)
        self.followed = bool(followed.all())
        self.sums = LT.in_order_sums(np.where(followed[..., None], self.samples, 0))
        self.frame = LT.resolve(self.sums, SPP)
        for a in (self.samples, self.sums, self.frame, self.pixel_followed):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(name, mode=16):
    return Run(name, mode)
