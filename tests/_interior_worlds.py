"""The cases and worlds of the solid-glass tests — test infrastructure only.

random_cases() / aimed_cases(): inputs of rt_interior_batch, shared by the CPU test (host batch against the numpy twin) and the GPU test (device probe against the
host batch).  room(): a floor, a light and glass of every kind the rule meets, seen from outside and from inside the glass box.  Every world is built through
the product's host vocabulary, which needs no device.
"""
import functools

import numpy as np

import _env_tree_twin as VT
import _env_twin as ET
import _env_worlds as EW
import _interior_twin as IT
import _mfac_worlds as MW
import _rglass_twin as GT
import _smooth_twin as ST
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
_unit = MW._unit


def random_cases(n=4096, seed=32):
    """n cases: unit normals, directions of any length on either side, distances and coefficients over many decades (so that sigma dist runs from 0 past 87),
    indices of water, glass, diamond and 1, a third of them on spheres"""
    rng = np.random.default_rng(seed)
    Ng, nn = _unit(rng.standard_normal((n, 3))), _unit(rng.standard_normal((n, 3)))
    ray_d = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(F)
    t = (10.0 ** rng.uniform(-3, 2, n)).astype(F)
    ior = rng.choice(np.array([1.0, 1.33, 1.5, 2.4], F), n).astype(F)
    sigma = (10.0 ** rng.uniform(-3, 2, (n, 3))).astype(F)
    sigma[rng.random((n, 3)) < 0.15] = F(0)
    sphere = (rng.random(n) < 1 / 3).astype(np.uint32)
    return dict(Ng=Ng, n=nn, ray_d=ray_d, t=t, ior=ior, sigma=sigma, sphere=sphere)


AIMED = ["triangle, front", "triangle, back", "parallelogram, front", "parallelogram, back", "sphere, front", "sphere, back", "sphere of negative radius, entered",
         "sphere of negative radius, left", "sigma 0, back", "sigma dist past 87", "sigma dist at 87", "total reflection from inside", "edge on", "a long direction"]


def aimed_cases():
    """one case per name of AIMED, in that order, and the facing each must take"""
    z, up, down = (0.0, 0.0, 1.0), (0.3, 0.2, 1.0), (0.3, 0.2, -1.0)
    tint = (0.5, 0.25, 2.0)
    rows = [
        # Ng, n, d, t, ior, sigma, sphere, back
        (z, z, down, 2.0, 1.5, tint, 0, 0),
        (z, (0.0, 0.0, -1.0), up, 2.0, 1.5, tint, 0, 1),          # the shading normal faces the ray; the stored one decides
        (z, z, down, 0.5, 1.33, tint, 0, 0),
        (z, (0.0, 0.0, -1.0), up, 0.5, 1.33, tint, 0, 1),
        ((1.0, 0.0, 0.0), z, down, 1.0, 1.5, tint, 1, 0),          # on a sphere Ng is not read
        ((1.0, 0.0, 0.0), z, up, 1.0, 1.5, tint, 1, 1),
        (z, (0.0, 0.0, -1.0), down, 1.0, 1.5, tint, 1, 1),         # (hit - centre) / r with r < 0 points inwards: the hollow shell's inner sphere, entered = back
        (z, (0.0, 0.0, -1.0), up, 1.0, 1.5, tint, 1, 0),
        (z, (0.0, 0.0, -1.0), up, 3.0, 1.5, (0.0, 0.0, 0.0), 0, 1),
        (z, (0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 30.0, 1.5, (3.0, 2.9, 100.0), 0, 1),
        (z, (0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 29.0, 1.5, (3.0, 2.9999, 3.0001), 0, 1),
        (z, (0.0, 0.0, -1.0), (0.9, 0.0, 0.45), 1.0, 1.5, tint, 0, 1),   # 63 degrees off the normal, beyond the critical angle of 1.5: charged all the same
        (z, z, (1.0, 0.0, 0.0), 1.0, 1.5, tint, 0, 0),
        (z, (0.0, 0.0, -1.0), (30.0, 20.0, 100.0), 0.02, 1.5, tint, 0, 1),
    ]
    assert len(rows) == len(AIMED)
    cols = list(zip(*rows))
    cases = dict(Ng=np.array(cols[0], F), n=np.array(cols[1], F), ray_d=np.array(cols[2], F), t=np.array(cols[3], F), ior=np.array(cols[4], F),
                 sigma=np.array(cols[5], F), sphere=np.array(cols[6], np.uint32))
    return cases, np.array(cols[7], np.uint32)


def run_cases(fn, cases):
    """fn = api.interior_batch, api.probe_interior or the twin's case()"""
    c = cases
    return fn(c["Ng"], c["n"], c["ray_d"], c["t"], c["ior"], c["sigma"], c["sphere"])


def expf_samples(n=1 << 22, seed=32):
    """n fp32 x spread over [-87, 0] by bit pattern and by value, every reduction boundary with its 16 neighbours on either side, and the ends"""
    rng = np.random.default_rng(seed)
    lo, hi = 0x80000000, int(np.array(-87.0, F).view(np.uint32))
    by_bits = rng.integers(lo, hi + 1, n // 2, dtype=np.uint64).astype(np.uint32).view(F)
    by_value = (-87.0 * rng.random(n - n // 2)).astype(F)
    b = IT.BOUNDARIES.view(np.uint32).astype(np.int64)
    near = (b[:, None] + np.arange(-16, 17)[None, :]).reshape(-1).astype(np.uint32).view(F)
    ends = np.array([0.0, -0.0, -87.0, np.nextafter(F(-87.0), F(0))], F)
    return np.concatenate([by_bits, by_value, near, ends]).astype(F)


# ---- the test room -----------------------------------------------------------------------------------------------------------------------------------------------
SEED = EW.SEED
W, H, SPP, DEPTH = 24, 16, 8, 8   # a path needs to enter, leave and land
ENV_TREE = 48
BACKGROUND = MW.BACKGROUND
FORMS = dict(MW.FORMS)   # one key per form of the INTERIOR family of csrc/rt_device.hip's kernel table and, once more, of its INTERIOR_ENV_TREE family: §29's shapes
OUTSIDE, INSIDE = "outside", "inside"
BOX = ((6.4, 0.2, 4.4), (8.2, 2.2, 6.2))
TINT = dict(smooth=((0.9, 0.6, 0.3), 1.0), box=((0.3, 0.8, 0.5), 1.0), ball=((0.8, 0.4, 0.9), 0.8), frosted=((0.95, 0.7, 0.7), 1.0))
RECORDS = 5


def room(p, env=False, as_list=False, records=True):
    """A Lambertian floor, a quad light, a metal ball, and glass: a flat icosphere(1) with a record and no tint, a smooth-normal icosphere(1) with a tint, a tinted
    box of six parallelograms, a tinted sphere, a frosted tinted tetrahedron, and an icosphere(0) WITHOUT a record — under a constant background or, env, the sky
    map.  records False: the same room without an interior record (the frosted tetrahedron keeps its rough-glass record)."""
    io = TW.mesh_io()
    s = p.Scene()
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s.Lambertian((0.6, 0.55, 0.5)))
    s.MakeQuad((3.5, 7, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((6, 6, 6)))
    s.MakeSphere((9.2, 0.9, 7.8), 0.9, s.Metal((0.8, 0.8, 0.9), 0.05))
    flat, smooth, box, ball, frosted, bare = (s.Dielectric(c, ior) for c, ior in (((1, 1, 1), 1.5), ((1, 1, 1), 1.5), ((1, 1, 1), 1.5), ((1, 1, 1), 1.5),
                                                                                      ((0.98, 0.98, 1.0), 1.5), ((1, 1, 1), 1.33)))
    v, f = io.icosphere(1)
    s.MakeMesh(v, f, flat, 1.1, 0.0, (2.6, 1.3, 6.0))
    s.MakeMesh(v, f, smooth, 1.2, 25.0, (5.0, 1.4, 7.6), normals=io.icosphere_normals(1))
    s.MakeBox(BOX[0], BOX[1], box)
    s.MakeSphere((4.2, 0.8, 4.0), 0.8, ball)
    tv, tf = io.tetrahedron()
    s.MakeMesh(tv, tf, frosted, 1.5, 10.0, (7.6, 1.6, 8.8))
    v0, f0 = io.icosphere(0)
    s.MakeMesh(v0, f0, bare, 0.9, 0.0, (1.4, 1.0, 8.6))
    s.set_rough_glass(frosted, 0.3)
    if records:
        s.set_interior(flat)
        for name, mat in (("smooth", smooth), ("box", box), ("ball", ball), ("frosted", frosted)):
            s.set_interior(mat, color=TINT[name][0], at=TINT[name][1])
    if env:
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(BACKGROUND)
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


def camera(p, view=OUTSIDE, w=W, h=H):
    if view == INSIDE:   # in the middle of the glass box, looking across the room through its wall
        return p.PinholeCamera((7.3, 1.2, 5.3), (4.0, 1.2, 7.0), (0, 1, 0), 80.0, w / h)
    return EW.camera(p, w, h)


def no_tint(interiors):
    """the table with every sigma 0: the facing alone"""
    out = interiors.copy()
    out["sigma"] = 0.0
    return out


def all_off(interiors):
    """a table of records that are all off"""
    return np.zeros(len(interiors), IT.INTERIOR_DT)


class Run:
    """the room, seen from `view`, and the twins' samples of it, plain or in mode 48: under the whole rule (samples), with every sigma 0 through the loop of its
    own (untinted) and through _path_twin's (facing), and with every record off (off: _rglass_twin's frame of the room)"""

    def __init__(self, env, as_list=False, view=OUTSIDE, spp=SPP, first_sample=0):
        p = pkg()
        self.scene = room(p, env=env, as_list=as_list)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        vn, self.mfacs, self.interiors = self.scene.vertex_normals(), self.scene.microfacets().copy(), self.scene.interiors().copy()
        cam = as_oracle_camera(camera(p, view))
        sky, light, tree = GT_lights(p, self.scene, self.world, env)
        trace = ST.smooth_walk(vn)
        smooth_tris = (ST.table(vn) != 0).any(axis=(1, 2))
        args = (self.world, cam, W, H, DEPTH, SEED)
        self.stats, self.info = IT.new_stats(), {}

        def frame(fn):
            import _path_twin as PT
            return PT.frame_samples(fn, W, H, spp, first_sample)
        self.samples, self.followed = frame(lambda g, s: IT.radiance(*args, g, s, sky, self.interiors, light, tree, self.mfacs, self.stats, trace, smooth_tris))
        self.untinted, _ = frame(lambda g, s: IT.radiance(*args, g, s, sky, no_tint(self.interiors), light, tree, self.mfacs, None, trace))
        self.facing, self.facing_followed = frame(lambda g, s: IT.facing_radiance(*args, g, s, sky, self.interiors, light, tree, None, self.mfacs, None, None, trace,
                                                                                   self.info))
        self.off, self.off_followed = GT.frame_samples(self.world, cam, W, H, spp, DEPTH, SEED, sky, vn, None, None, self.mfacs, None, light=light, tree=tree,
                                                       first_sample=first_sample)
        self.sums, self.facing_sums, self.off_sums = (IT.in_order_sums(a) for a in (self.samples, self.facing, self.off))
        self.frame = IT.resolve(self.sums, spp)
        for a in (self.samples, self.followed, self.untinted, self.facing, self.off, self.sums, self.facing_sums, self.off_sums, self.frame, self.mfacs, self.interiors):
            a.setflags(write=False)


def GT_lights(p, scene, world, env):
    """(sky, light, tree) as the twins take them: a constant background, or mode 48's map and table"""
    if env:
        image, u0 = scene.environment()
        return ET.sky_environment(image, u0), (p.api.environment_distribution(image), u0), VT.table_of(world)
    colour = np.array(BACKGROUND, F)
    return (lambda d: np.broadcast_to(colour, (len(d), 3))), None, None


@functools.lru_cache(maxsize=None)
def run(env, as_list=False, view=OUTSIDE):
    return Run(env, as_list, view)
