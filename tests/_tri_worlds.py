"""The worlds of the triangle tests and the twin's runs of them — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device.  tri_room() and the unit worlds hold only what tests/_tri_twin.py follows
(pinhole camera; Lambertian, checker, metal and diffuse-light materials), so a test asserts `followed.all()` and leaves no pixel out; run(...) is computed once
per process and never modified.  The worlds below `wide_room` go beyond the twin's scope (dielectrics, moving spheres, media, noise and image textures, the
defocus and motion-blur cameras, the lane walks) and are judged by the oracle, which knows the triangle kind and is pinned to the twin on it
(tests/test_triangles_cpu.py); tests/test_gpu_triangles_oracle.py renders them.
"""
import functools

import numpy as np

import _tri_twin as TT
from _common import as_oracle_camera, as_oracle_world, pkg
from _nee_worlds import _shell

SEED = 1984
W = H = 32
SPP, DEPTH = 4, 8
VIEW = ((5, 5, 0.5), (5, 4, 10), 80.0)


def mesh_io():
    pkg()
    from ray_tracing_v06_amd import mesh_io as m
    return m


BVH, LIST = "RT_WORLD_BVH", "RT_WORLD_LIST"
WORLD_ID = {BVH: 0, LIST: 1}   # RT_WORLD_BVH, RT_WORLD_LIST of include/rt06.h
LDS, NARROW, WIDE = {}, {"RT06_FORCE_BIG": "1"}, {"RT06_FORCE_BIG": "1", "RT06_FORCE_WIDE": "1"}

# The suite's statement of which TRI instantiations of render_kernel_stream exist: one (world, exact, ext, big, wide) key per form of the TRI family of
# csrc/rt_device.hip — and, the same sixteen keys once more, per form of its TRI_NEE family —, each with the recipe (kernel variant, environment) that makes a
# renderer of a triangle room resolve to it; ext 2 takes the textured room, a list the room left a HittableList.  tests/test_triangles_cpu.py holds the table against
# the source, tests/test_gpu_triangles.py renders every key plain and with light sampling and compares it with the twin.
FORMS = {
    (BVH, 0, 1, 0, 0): (3, LDS),     (BVH, 1, 1, 0, 0): (2, LDS),     (BVH, 0, 2, 0, 0): (3, LDS),     (BVH, 1, 2, 0, 0): (2, LDS),
    (BVH, 0, 1, 1, 0): (3, NARROW),  (BVH, 1, 1, 1, 0): (2, NARROW),  (BVH, 0, 2, 1, 0): (3, NARROW),  (BVH, 1, 2, 1, 0): (2, NARROW),
    (BVH, 0, 1, 1, 1): (3, WIDE),    (BVH, 1, 1, 1, 1): (2, WIDE),    (BVH, 0, 2, 1, 1): (3, WIDE),    (BVH, 1, 2, 1, 1): (2, WIDE),
    (LIST, 1, 1, 0, 0): (0, LDS),    (LIST, 1, 1, 1, 1): (0, NARROW), (LIST, 1, 2, 0, 0): (0, LDS),    (LIST, 1, 2, 1, 1): (0, NARROW),
}


def form_id(form):
    world, exact, ext, big, wide = form
    return f"{world[9:].lower()}-{'exact' if exact else 'fast'}-ext{ext}-{('lds', 'narrow', 'wide')[big + wide]}"


def kernel_form_of(form, nee=0):
    """what Renderer.kernel_form() reports for a FORMS key"""
    world, exact, ext, big, wide = form
    return {"kernel": "stream", "exact": exact, "filter": 0, "world": WORLD_ID[world], "ext": ext, "big": big, "wide": wide, "tol": 0, "nee": nee}


def tri_room(p, as_list=False, traversal=0, lamp=False, tri_light=False, wall_as_triangles=False, plain=False, textured=False, open_right=False, more=None,
             builder="BuildBVH_SAH"):
    """a closed 10 x 10 x 10 room of quads with one quad light, holding a tetrahedron, an icosphere(1) (80 triangles) of metal and a checker triangle;
    lamp: plus a sphere light; tri_light: plus a triangle with a light material (it emits, no table lists it); wall_as_triangles: the back wall as
    its two triangles; plain: the room without any triangle (the pins' world); textured: plus an image-textured triangle on the back wall and its image
    (an EXT = 2 world; the twin does not follow the samples that meet it); open_right: the room without its right wall; more(s): called before the world is
    built, to add to it; builder: the BVH builder of a world that is not left a list"""
    s = p.Scene()
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    if wall_as_triangles:
        s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), white)
        s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), white)
        s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), red)
        s.MakeQuad((10, 0, 0), (0, 10, 0), (0, 0, 10), green)
        s.MakeTriangle((0, 0, 10), (10, 0, 10), (0, 10, 10), white)      # the back wall (0,0,10) + (10,0,0) a + (0,10,0) b, cut along its diagonal
        s.MakeTriangle((10, 10, 10), (0, 10, 10), (10, 0, 10), white)
        s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 10, 0), white)
    elif open_right:   # _shell without its fourth quad
        s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), white)
        s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), white)
        s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), red)
        s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 10, 0), white)
        s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 10, 0), white)
    else:
        _shell(s, white, white, red, green)
    s.MakeQuad((3.5, 9.9, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    if lamp:
        s.MakeSphere((2, 7.5, 7), 0.6, s.DiffuseLight((20, 14, 6)))
    if not plain and not wall_as_triangles:
        m = mesh_io()
        s.MakeMesh(*m.tetrahedron(), red, 1.6, 20.0, (3, 1.4, 6))
        s.MakeMesh(*m.icosphere(1), s.Metal((0.8, 0.8, 0.9), 0.1), 1.5, 0.0, (7, 1.6, 5.5))
        s.MakeTriangle((4, 0.05, 2.5), (6.5, 0.05, 2), (5, 2.5, 4), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    else:
        s.MakeSphere((3, 1.5, 6), 1.5, s.Metal((0.8, 0.8, 0.9), 0.1))
        s.MakeSphere((7, 1.2, 5), 1.2, s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    if tri_light:
        s.MakeTriangle((0.2, 6, 3), (0.2, 8, 5), (0.2, 6, 7), s.DiffuseLight((5, 9, 5)))
    if textured:
        from _nee_worlds import small_image
        s.set_image(small_image())
        s.MakeTriangle((0.8, 5.2, 9.9), (3.3, 5.2, 9.9), (0.8, 7.7, 9.9), s.ImageTexture())
    if more is not None:
        more(s)
    if as_list:
        s.MakeHittableList()
    else:
        s.set_traversal(traversal)
        getattr(s, builder)()
    return s


CAMERAS = ("pinhole", "defocus", "motion")


def camera(p, w=W, h=H, kind="pinhole"):
    if kind == "defocus":
        return p.DefocusBlurCamera(VIEW[0], VIEW[1], (0, 1, 0), VIEW[2], w / h, 0.3, 6.0)
    if kind == "motion":
        return p.MotionBlurCamera(VIEW[0], VIEW[1], (0, 1, 0), VIEW[2], w / h, 0.0, 1.0)
    assert kind == "pinhole"
    return p.PinholeCamera(VIEW[0], VIEW[1], (0, 1, 0), VIEW[2], w / h)


class Run:
    """a room, the camera and the twin's samples of it (mode 0 / 1 / 2 of light sampling)"""

    def __init__(self, as_list, mode, lamp, tri_light, textured):
        p = pkg()
        self.scene = tri_room(p, as_list=as_list, lamp=lamp, tri_light=tri_light, textured=textured)
        self.cam = camera(p)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        self.samples, followed = TT.frame_samples(self.world, as_oracle_camera(self.cam), W, H, SPP, DEPTH, SEED, mode=mode)
        self.pixel_followed = followed.all(axis=2)    # pixels whose every sample the twin followed to its end: all of them, but in a textured room
        self.followed = bool(followed.all())
        self.sums = TT.in_order_sums(np.where(followed[..., None], self.samples, 0))   # exact where pixel_followed; elsewhere not the frame's
        self.frame = TT.resolve(self.sums, SPP)
        for a in (self.samples, self.sums, self.frame, self.pixel_followed):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(as_list=False, mode=0, lamp=False, tri_light=False, textured=False):
    return Run(as_list, mode, lamp, tri_light, textured)


# ---- crafted rays and unit worlds: rt_probe_trace, the twin and the oracle are held to one another on them ------------------------------------------
def unit_world(p, triangle, as_list, second=False):
    """the unit triangle (0,0,0), (1,0,0), (0,1,0) or the quad of the same Q, u, v; second: plus the coplanar triangle across the diagonal"""
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    if triangle:
        s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
        if second:
            s.MakeTriangle((1, 1, 0), (0, 1, 0), (1, 0, 0), m)
    else:
        s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    s.MakeSphere((0.5, 0.5, -10), 3.0, m)   # behind the plane; widens a list's bounds, so that the rays at the vertices and on the edges get past them to the interior test
    s.MakeHittableList() if as_list else s.BuildBVH_TopDown()
    return s


def equal_distance_world(p, as_list):
    """a quad and two triangles in one plane, the second triangle a copy of the first: down z every one of them gives t = 1 exactly"""
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    s.MakeSphere((0.5, 0.5, -10), 3.0, m)
    s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    s.MakeHittableList() if as_list else s.BuildBVH_TopDown()
    return s


def down_z(points):
    rays = np.zeros((len(points), 7), np.float32)
    rays[:, 0:2] = np.array(points, np.float32)
    rays[:, 2], rays[:, 5] = 1, -1
    return rays


EPS = np.float32(2.0 ** -23)
CRAFTED = [(0.25, 0.25), (0.5, 0.5), (0.5, np.float32(0.5) + EPS), (0.75, 0.75), (0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (-0.25, 0.5), (0.5, -0.25), (1.25, 0.1)]
DIAGONAL = [(0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.25, 0.25), (0.75, 0.75)]
EQUAL_DISTANCE = [(0.25, 0.25), (0.125, 0.5), (0.75, 0.75)]


def crafted_rays():
    rays = down_z(CRAFTED)
    in_plane = np.array([[-1, 0.25, 0, 1, 0, 0, 0], [-1, 0.25, 0, 1, 0, 1e-9, 0]], np.float32)   # |denom| < 1e-8: rejected whatever it would meet
    return np.concatenate([rays, in_plane])


def room_rays(n, seed=11, timed=False):
    """n rays from inside the room, one half in every direction, the other towards where the meshes stand; timed: each with a time in [0, 1) for a moving sphere"""
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 7), np.float32)
    rays[:, 0:3] = rng.random((n, 3), dtype=np.float32) * 8 + 1
    rays[:, 3:6] = rng.standard_normal((n, 3)).astype(np.float32)
    aimed = (rng.random((n - n // 2, 3), dtype=np.float32) * np.float32([6.5, 3.5, 5.5]) + np.float32([2, 0, 2])).astype(np.float32)
    rays[n // 2:, 3:6] = aimed - rays[n // 2:, 0:3]
    if timed:
        rays[:, 6] = rng.random(n, dtype=np.float32)
    return rays


# ---- worlds beyond the twin's scope: the oracle judges them -----------------------------------------------------------------------------------------
SKY = (0.3, 0.5, 0.9)
MAT = {"lambertian": 0, "metal": 1, "dielectric": 2, "checker": 3, "light": 4, "isotropic": 5, "noise": 6, "image": 7}   # RT_MAT_* of include/rt06.h


def wide_room(p, ext=1, medium=True, mesh_level=1, **room):
    """tri_room without its right wall, a constant background behind the opening, plus a glass icosphere(mesh_level), a fuzzy-metal tetrahedron and a moving
    sphere; ext = 2: plus an image-textured and a Perlin-noise triangle with their tables and, with `medium`, a sphere of Isotropic medium"""
    def more(s):
        m = mesh_io()
        s.MakeMesh(*m.icosphere(mesh_level), s.Dielectric((1, 1, 1), 1.5), 1.3, 0.0, (5, 3.6, 7))
        s.MakeMesh(*m.tetrahedron(), s.Metal((0.7, 0.6, 0.5), 0.4), 1.3, 45.0, (8, 6, 7.5))
        s.MakeMovingSphere((2, 2, 7.5), (2, 2.9, 7.5), 0.8, s.Lambertian((0.2, 0.4, 0.8)))
        s.set_background(SKY)
        if ext == 2:
            s.set_perlin(SEED)
            s.MakeTriangle((0.05, 0.5, 4), (0.05, 0.5, 8), (0.05, 4.5, 6), s.NoiseTexture(2.0, (0.6, 0.6, 0.6)))
            if medium:
                s.MakeSphere((6.5, 6.5, 6), 1.6, s.Isotropic((0.9, 0.9, 0.9), 0.4))
    assert ext in (1, 2)
    return tri_room(p, open_right=True, textured=ext == 2, more=more, **room)


def boundary_world(p, which, builder="BuildBVH_TopDown", traversal=0):
    """the worlds around `quad index >= n_plain_quads`: "triangles_only" (no sphere, no parallelogram), "one_quad" (one parallelogram, many triangles),
    "one_triangle" (many parallelograms, one triangle), "siblings" (the last parallelogram and the first triangle are the two leaves of one inner node: a flat
    leaf holds one primitive, so this is as close as two primitives come in a tree)"""
    s = p.Scene()
    m = mesh_io()
    grey, red, mirror = s.Lambertian((0.6, 0.6, 0.6)), s.Lambertian((0.7, 0.2, 0.2)), s.Metal((0.8, 0.8, 0.8), 0.05)
    s.set_background((0.6, 0.7, 0.9))
    if which == "triangles_only":
        s.MakeTriangle((-6, 0, -6), (6, 0, -6), (-6, 0, 6), grey)
        s.MakeTriangle((6, 0, 6), (-6, 0, 6), (6, 0, -6), grey)
        s.MakeMesh(*m.icosphere(1), mirror, 1.2, 0.0, (-1.5, 1.3, 0))
        s.MakeMesh(*m.tetrahedron(), red, 1.3, 10.0, (1.8, 1.0, 0.5))
    elif which == "one_quad":
        s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), grey)
        s.MakeMesh(*m.icosphere(1), mirror, 1.2, 0.0, (-1.5, 1.3, 0))
        s.MakeMesh(*m.tetrahedron(), s.Dielectric((1, 1, 1), 1.5), 1.3, 10.0, (1.8, 1.0, 0.5))
        s.MakeSphere((0.3, 0.6, 2.0), 0.6, red)
    elif which == "one_triangle":
        s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), grey)
        s.MakeBox((-2.5, 0, -1), (-0.8, 2.2, 0.6), red, 20.0, (0, 0, 0))
        s.MakeBox((0.8, 0, -0.5), (2.4, 1.4, 1.0), mirror, -15.0, (0, 0, 0))
        s.MakeQuad((-1, 3.5, -1), (2, 0, 0), (0, 0, 2), s.DiffuseLight((6, 6, 6)))
        s.MakeTriangle((-0.6, 0.02, 1.2), (0.9, 0.02, 1.5), (0.1, 1.6, 1.0), s.Dielectric((1, 1, 1), 1.5))
        s.MakeSphere((3.0, 0.5, 2.0), 0.5, mirror)
    else:
        assert which == "siblings"
        for i in range(6):   # quads to the left, one quad and one triangle close together and away from the rest, triangles to the right
            s.MakeQuad((-6 + 0.9 * i, 0.2 * i, -1), (0.7, 0, 0.1), (0, 1.5, 0.2), (grey, red, mirror)[i % 3])
        s.MakeQuad((0.5, 0, 0), (1, 0, 0), (0, 1.2, 0.1), red)
        s.MakeTriangle((1.6, 0, 0), (2.6, 0, 0.1), (2.0, 1.4, 0), mirror)
        for i in range(6):
            s.MakeTriangle((4 + 0.9 * i, 0, -1 + 0.1 * i), (4.7 + 0.9 * i, 0, -1), (4.3 + 0.9 * i, 1.5 - 0.1 * i, -0.8), (grey, red, mirror)[i % 3])
    if builder == "MakeHittableList":
        s.MakeHittableList()
    else:
        s.set_traversal(traversal)
        getattr(s, builder)()
    return s


def boundary_camera(p, w=W, h=H):
    return p.PinholeCamera((0.5, 2.2, 7.5), (0.3, 0.8, 0), (0, 1, 0), 60.0, w / h)


def sibling_leaves(scene):
    """(primitive of the left leaf, primitive of the right leaf) of every inner node of the flat tree whose two children are leaves"""
    nodes, _, _ = scene.arrays()
    out = []
    for n in nodes[nodes["left"] >= 0]:
        a, b = nodes[n["left"]], nodes[n["right"]]
        if a["left"] == -1 and b["left"] == -1:
            out.append((int(a["right"]), int(b["right"])))
    return out


def mesh_room(p, level, **room):
    """tri_room plus an icosphere(level) of glass: level 4 (5120 triangles) does not fit the LDS by itself, level 2 (320) does"""
    def more(s):
        s.MakeMesh(*mesh_io().icosphere(level), s.Dielectric((1, 1, 1), 1.5), 1.4, 0.0, (5, 4.5, 7))
    return tri_room(p, more=more, **room)


def closed_mesh_world(p, as_list=False, level=2):
    """a closed icosphere(level) of radius 1.5 about the origin and nothing else, and rays from outside at every vertex, every edge midpoint and every face
    centroid (computed in float64 from the unit mesh, rounded once): from the point radially outside each target and from one fixed point"""
    v, f = mesh_io().icosphere(level)
    s = p.Scene()
    s.MakeMesh(v, f, s.Lambertian((0.5, 0.5, 0.5)), 1.5, 0.0, (0, 0, 0))
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    v64 = v.astype(np.float64) * 1.5
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), axis=1), axis=0)
    targets = np.concatenate([v64, (v64[edges[:, 0]] + v64[edges[:, 1]]) * 0.5, v64[f.astype(np.int64)].mean(axis=1)])
    radial = targets / np.linalg.norm(targets, axis=1)[:, None] * 4.0
    fixed = np.broadcast_to(np.array([3.0, 2.5, 4.0]), targets.shape)
    rays = np.zeros((2 * len(targets), 7), np.float32)
    rays[:, 0:3] = np.concatenate([radial, fixed]).astype(np.float32)
    rays[:, 3:6] = (np.concatenate([targets, targets]) - rays[:, 0:3].astype(np.float64)).astype(np.float32)
    return s, rays, (len(v), len(edges), len(f))


BUILDERS = ("BuildBVH_TopDown", "BuildBVH_SAH", "BuildBVH_BottomUp", "MakeHittableList")
EYE_SPECIALS = (0.0, 1e-30, -1e-25)   # eye coordinates outside the fast-division class, as tools/fuzz_campaign.py draws them


def random_triangles(s, rng, mats, spread=6.0, n_free=None, meshes=None):
    """free triangles — now and then axis-aligned (padded bounds), a sliver (one edge 1e-3 of the others) or large — and meshes (tetrahedron, icosphere(0..2))
    with random scale, rotation and translation, added to scene s with materials drawn from mats; returns what was added, for a recipe"""
    m = mesh_io()
    n_free = int(rng.integers(5, 31)) if n_free is None else n_free
    shapes = {"plain": 0, "axis": 0, "sliver": 0, "large": 0}
    for _ in range(n_free):
        a = ((rng.random(3) * 2 - 1) * np.array([spread, 2.5, spread])).astype(np.float32)
        shape = ("plain", "axis", "sliver", "large")[int(rng.choice(4, p=[0.55, 0.2, 0.15, 0.1]))]
        if shape == "axis":
            e1, e2 = np.float32([rng.random() * 3 + 0.3, 0, 0]), np.float32([rng.random() * 2, 0, rng.random() * 3 + 0.3])
        elif shape == "sliver":
            e1 = (rng.standard_normal(3) * 1.5).astype(np.float32)
            e2 = (e1 + np.cross(e1, rng.standard_normal(3)) / max(np.linalg.norm(e1), 1e-3) * 1e-3).astype(np.float32)   # the edge between b and c: 1e-3 of the others
        elif shape == "large":
            e1, e2 = (rng.standard_normal(3) * 12).astype(np.float32), (rng.standard_normal(3) * 12).astype(np.float32)
        else:
            e1, e2 = (rng.standard_normal(3) * 1.5).astype(np.float32), (rng.standard_normal(3) * 1.5).astype(np.float32)
        try:
            s.MakeTriangle(a, a + e1, a + e2, mats[int(rng.integers(0, len(mats)))])
            shapes[shape] += 1
        except Exception as e:   # a degenerate draw is refused by the host (RtError), and is not a triangle of this world
            if "degenerate triangle" not in str(e):
                raise
    added = []
    for _ in range(int(rng.integers(1, 4)) if meshes is None else meshes):
        level = int(rng.integers(-1, 3))
        v, f = m.tetrahedron() if level < 0 else m.icosphere(level)
        c = ((rng.random(3) * 2 - 1) * np.array([spread * 0.7, 1.5, spread * 0.7])).astype(np.float32)
        _, n = s.MakeMesh(v, f, mats[int(rng.integers(0, len(mats)))], float(rng.uniform(0.3, 1.8)), float(rng.uniform(-180, 180)), c)
        added.append(("tetrahedron" if level < 0 else f"icosphere({level})", n))
    return {"free": shapes, "meshes": added}


def random_tri_world(p, seed):
    """One world of the randomised test: spheres (moving ones too), parallelograms, meshes and free triangles, materials of every kind, a random background,
    builder and camera.  Returns (scene, camera, W, H, spp, depth, recipe)."""
    rng = np.random.default_rng(31000 + seed)
    s = p.Scene()
    ext2 = bool(rng.random() < 0.5)
    mats = [s.Lambertian(rng.random(3)), s.Metal(rng.random(3), float(rng.choice([0.0, 0.1, 0.7]))), s.Dielectric((1, 1, 1), float(rng.choice([1.5, 1.33, 1 / 1.5]))),
            s.LambertianTexture(rng.random(3), rng.random(3), float(rng.choice([0.2, 0.5, 1.3]))), s.DiffuseLight(rng.random(3) * float(rng.choice([2.0, 8.0])))]
    if ext2:
        s.set_perlin(int(rng.integers(0, 1 << 30)))
        s.set_image(rng.integers(0, 256, (int(rng.integers(1, 20)), int(rng.integers(1, 30)), 3)).astype(np.uint8))
        mats += [s.NoiseTexture(float(rng.choice([0.5, 2.0])), rng.random(3)), s.ImageTexture()]
    medium = s.Isotropic(rng.random(3), float(rng.choice([0.05, 0.5])))   # on spheres only: a quad never bounds a medium
    n_spheres = int(rng.integers(0, 25))
    for _ in range(n_spheres):
        c = ((rng.random(3) * 2 - 1) * np.array([6, 2, 6])).astype(np.float32)
        r = float(rng.choice([0.05, 0.3, 0.8, 2.0]))
        m = medium if rng.random() < 0.1 else mats[int(rng.integers(0, len(mats)))]
        if rng.random() < 0.3:
            s.MakeMovingSphere(c, c + (rng.random(3).astype(np.float32) - 0.5), r, m)
        else:
            s.MakeSphere(c, r, m)
    n_quads = int(rng.integers(0, 12))
    for _ in range(n_quads):
        Q = ((rng.random(3) * 2 - 1) * np.array([6, 3, 6])).astype(np.float32)
        if rng.random() < 0.4:
            u, v = np.float32([rng.random() * 4 + 0.3, 0, 0]), np.float32([0, 0, rng.random() * 4 + 0.3])
        else:
            u, v = (rng.standard_normal(3) * 2).astype(np.float32), (rng.standard_normal(3) * 2).astype(np.float32)
        s.MakeQuad(Q, u, v, mats[int(rng.integers(0, len(mats)))])
    added = random_triangles(s, rng, mats)
    background = None
    if rng.random() < 0.7:
        background = tuple(float(x) for x in rng.random(3) * 0.6)
        s.set_background(background)
    builder = int(rng.integers(0, 4))
    getattr(s, BUILDERS[builder])()
    W, H = int(rng.integers(17, 49)), int(rng.integers(9, 33))
    spp, depth = int(rng.integers(1, 9)), int(rng.choice([1, 2, 5, 50]))
    eye = ((rng.random(3) * 2 - 1) * np.array([9, 4, 9])).astype(np.float32)
    if seed % 4 == 1:   # now and then
        eye[int(rng.integers(0, 3))] = float(rng.choice(EYE_SPECIALS))
    ck = int(rng.integers(0, 3))
    fov = float(rng.uniform(20, 100))
    if ck == 0:
        cam = p.PinholeCamera(eye, (0, 0, 0), (0, 1, 0), fov, W / H)
    elif ck == 1:
        cam = p.DefocusBlurCamera(eye, (0, 0, 0), (0, 1, 0), fov, W / H, float(rng.uniform(0, 0.5)), float(rng.uniform(2, 12)))
    else:
        cam = p.MotionBlurCamera(eye, (0, 0, 0), (0, 1, 0), fov, W / H, 0.0, 1.0)
    recipe = {"seed": seed, "ext": 2 if ext2 else 1, "spheres": n_spheres, "quads": n_quads, "triangles": added, "background": background, "builder": BUILDERS[builder],
              "camera": CAMERAS[ck], "eye": eye.tolist(), "fov": fov, "frame": (W, H, spp, depth)}
    return s, cam, W, H, spp, depth, recipe


def flat_bytes(scene):
    """every byte a flat world hands a renderer: header fields, nodes, spheres, materials, quads, noise tables and image"""
    w = scene.getWorldPtr()
    nodes, prims, mats = scene.arrays()
    head = np.array([w.kind, w.root, w.n_nodes, w.n_prims, w.n_materials, w.n_quads, w.background, w.image_width, w.image_height, w.traversal], np.int64).tobytes()
    head += np.array(list(w.bounds_min) + list(w.bounds_max) + list(w.background_color), np.float32).tobytes()
    return head + nodes.tobytes() + prims.tobytes() + mats.tobytes() + scene.quads().tobytes() + scene.perlin_bytes() + scene.image().tobytes()
