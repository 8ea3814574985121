"""The worlds of the smooth-shading tests and the twin's runs of them — test infrastructure only.

smooth_room() is _tri_worlds' EXT 1 room — the closed room of quads with its quad light, its flat tetrahedron, flat metal icosphere and flat checker triangle —
with a triangle light and, on top: a smooth Lambertian icosphere(1), a smooth fuzzy-metal tetrahedron whose normals come from mesh_io.vertex_normals (a
deliberately bad case: a vertex normal stands 70 degrees off its faces, so grazing hits take the second fallback), and one free flat triangle.  It holds
only what tests/_smooth_twin.py follows, so a test asserts `followed.all()`; run(...) is computed once per process and never modified.
"""
import functools

import numpy as np

import _smooth_twin as ST
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

SEED = 1984
W, H = 48, 32
SPP, DEPTH = 8, 6


def add_smooth(s):
    m = TW.mesh_io()
    v, f = m.icosphere(1)
    s.MakeMesh(v, f, s.Lambertian((0.3, 0.5, 0.8)), 1.3, 15.0, (5, 5.2, 6.5), normals=m.icosphere_normals(1))
    tv, tf = m.tetrahedron()
    s.MakeMesh(tv, tf, s.Metal((0.85, 0.75, 0.6), 0.3), 1.9, 35.0, (2.2, 4.6, 4.2), normals=m.vertex_normals(tv, tf))
    s.MakeTriangle((7.2, 4.0, 7.5), (9.4, 4.4, 6.2), (8.3, 6.6, 7.8), s.Lambertian((0.7, 0.6, 0.2)))   # free, flat


def smooth_room(p, more=None, **room):
    def both(s):
        add_smooth(s)
        if more is not None:
            more(s)
    return TW.tri_room(p, tri_light=True, more=both, **room)


def camera(p):
    return TW.camera(p, W, H)


class Run:
    """a room, its table of vertex normals, the camera and the twin's samples of it"""

    def __init__(self, as_list, mode, lamp, textured, flat):
        p = pkg()
        self.scene = smooth_room(p, as_list=as_list, lamp=lamp, textured=textured)
        self.cam = camera(p)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        self.vn = self.scene.vertex_normals()
        vn = np.zeros_like(self.vn) if flat else self.vn
        self.info = {}
        self.samples, followed = ST.frame_samples(self.world, vn, as_oracle_camera(self.cam), W, H, SPP, DEPTH, SEED, mode=mode, info=self.info)
        self.pixel_followed = followed.all(axis=2)
        self.followed = bool(followed.all())
        self.sums = ST.in_order_sums(np.where(followed[..., None], self.samples, 0))
        self.frame = ST.resolve(self.sums, SPP)
        for a in (self.samples, self.sums, self.frame, self.pixel_followed):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(as_list=False, mode=0, lamp=False, textured=False, flat=False):
    return Run(as_list, mode, lamp, textured, flat)


# ---- crafted hits: one triangle per case, its record, a ray and what the rule must do with it ---------------------------------------------------------
def unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x)).astype(np.float32)


TRI = ((0, 0, 0), (2, 0, 0), (0, 2, 0))                     # a, b, c: its plane is z = 0, its normal +z
TILTED = (unit((0.3, 0.1, 1)), unit((-0.2, 0.3, 1)), unit((0.1, -0.3, 1)))
AWAY = (unit((1, 0, 0.15)), unit((1, 0.1, 0.15)), unit((1, -0.1, 0.15)))   # normals that lean far towards +x


def crafted_cases():
    """[(name, vertex normals (3, 3) or None for an all-zero record, point of the plane z = 0 aimed at, ray origin, expected: 'interpolated' / 'flat')]"""
    down = lambda x, y: ((x, y, 0.0), (x, y, 3.0))
    cases = []
    for name, (x, y) in (("vertex a", (0, 0)), ("vertex b", (2, 0)), ("vertex c", (0, 2)), ("midpoint ab", (1, 0)), ("midpoint ac", (0, 1)), ("midpoint bc", (1, 1)),
                         ("alpha + beta == 1", (0.5, 1.5)), ("inside", (0.5, 0.25))):
        cases.append((name, TILTED, *down(x, y), "interpolated"))
    cases.append(("n0 == -n1 at the midpoint of ab: l2 == 0", (unit((0, 0, 1)), unit((0, 0, -1)), unit((0, 0, 1))), *down(1, 0), "flat"))
    cases.append(("an all-zero record", None, *down(0.5, 0.25), "flat"))
    cases.append(("a NaN component", (np.float32([np.nan, 0, 1]), TILTED[1], TILTED[2]), *down(0.5, 0.25), "flat"))
    cases.append(("grazing, normals tilting away", AWAY, (0.5, 0.5, 0.0), (-9.5, 0.5, 1.0), "flat"))      # from -x, 5.7 degrees above the plane: dot(d, s) > 0
    cases.append(("back face", TILTED, (0.5, 0.25, 0.0), (0.5, 0.25, -3.0), "interpolated"))           # from below: s is negated to the side the ray sees
    return cases


def crafted_arrays(p):
    """the cases as rt_shading_normal_batch takes them: (names, tris (capi.QUAD_DT), vn (n, 3, 3), rays (n, 6), t (n,), expected interpolated (n,) bool)"""
    cases = crafted_cases()
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    s.MakeTriangle(*TRI, m)
    s.MakeHittableList()
    tri = s.quads()[0]
    n = len(cases)
    tris = np.repeat(tri[None], n)
    vn, rays, t = np.zeros((n, 3, 3), np.float32), np.zeros((n, 6), np.float32), np.zeros(n, np.float32)
    for i, (_, normals, target, origin, _) in enumerate(cases):
        if normals is not None:
            vn[i] = np.asarray(normals, np.float32)
        o, d = np.float32(origin), np.float32(target) - np.float32(origin)
        rays[i, 0:3], rays[i, 3:6] = o, d
        t[i] = np.float32(1)   # the direction is not normalised: the target is at t = 1 (exactly: origin z and d z are -each other)
    return [c[0] for c in cases], tris, vn, rays, t, np.array([c[4] == "interpolated" for c in cases])


def crafted_world(p, as_list):
    """the crafted triangle alone with a sphere far behind it (as _tri_worlds.unit_world has one, so that a list's bounds do not end in the triangle's plane),
    for rt_probe_shading_normal, which takes a case's record as its one-record table"""
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    s.MakeTriangle(*TRI, m)
    s.MakeSphere((0.5, 0.5, -30), 3.0, m)
    s.MakeHittableList() if as_list else s.BuildBVH_TopDown()
    return s
