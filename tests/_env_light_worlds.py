"""The maps, uniforms, worlds and kernel forms of the environment-light-sampling tests — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device; what is computed here is computed once per process and never modified.
"""
import functools

import numpy as np

import _env_light_twin as LT
import _env_twin as ET
import _env_worlds as EW
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
SEED = EW.SEED
W, H, SPP, DEPTH = EW.W, EW.H, EW.SPP, EW.DEPTH   # 24 x 16 at 8 spp and depth 6
ENV = 32                                          # RT_LIGHT_SAMPLING_ENV
TINY = F(2.0 ** -24)                              # the smallest uniform the generator gives

# The suite's statement of which ENVL instantiations of render_kernel_stream exist: one (world, exact, ext, big, wide) key per form of the ENV_LIGHT family of
# csrc/rt_device.hip, each with _tri_worlds' recipe (kernel variant, environment) that makes a renderer of a background-2 world resolve to it.
# tests/test_env_light_cpu.py holds the list against the source; tests/test_gpu_env_light.py renders every key and compares it with the twin.
FORMS = {f: TW.FORMS[f] for f in [(TW.BVH, 0, 2, 0, 0), (TW.BVH, 1, 2, 0, 0), (TW.BVH, 0, 2, 1, 0), (TW.BVH, 1, 2, 1, 0), (TW.BVH, 0, 2, 1, 1), (TW.BVH, 1, 2, 1, 1),
                                  (TW.LIST, 1, 2, 0, 0), (TW.LIST, 1, 2, 1, 1)]}


def black_rows_map():
    """16 x 8, the bottom three rows black"""
    env = EW.random_map(16, 8).copy()
    env[5:] = 0
    env.setflags(write=False)
    return env


def sun_map(width=32, height=16, at=(3, 20), value=1e4):
    """a dim grey sky with one texel at `value`"""
    env = np.full((height, width, 3), 0.05, F)
    env[at] = value
    env.setflags(write=False)
    return env


def half_black_map(width=32, height=16):
    """the procedural sky with its lower half black"""
    env = EW.sky_map().copy()
    assert env.shape == (height, width, 3)
    env[height // 2:] = 0
    env.setflags(write=False)
    return env


def random_uniforms(n, seed):
    """n quadruples uniform in (0, 1], on the generator's grid of 2^-24"""
    rng = np.random.default_rng(seed)
    u = ((rng.integers(0, 1 << 24, (n, 4)) + 1).astype(np.float64) * 2.0 ** -24).astype(F)
    u.setflags(write=False)
    return u


def crafted_uniforms(tables):
    """quadruples with exactly 1 and 2^-24 in each place and in all at once, and x1, x2 such that x1 * A rounds up to A and x2 * R_j to R_j: the largest floats below 1"""
    out = []
    for k in range(4):
        for v in (F(1), TINY):
            q = np.full(4, 0.37, F)
            q[k] = v
            out.append(q)
    out.append(np.full(4, 1, F))
    out.append(np.full(4, TINY, F))
    near_one = [np.nextafter(F(1), F(0)), F(1) - F(2.0 ** -23), F(1) - F(2.0 ** -22)]
    rowc = np.asarray(tables["rowc"], F)
    A = rowc[-1]
    for x1 in near_one + [F(1)]:
        for x2 in near_one + [F(1)]:
            out.append(np.array([x1, x2, 0.5, 0.5], F))
    # x1 that lands exactly on a stored row sum (x = rowc[j] picks row j + 1 or later) and just below it, where the division gives such a float
    for c in rowc[:-1][:4]:
        x1 = F(c / A)
        if F(0) < x1 <= F(1):
            out.append(np.array([x1, 0.5, 0.25, 0.75], F))
            out.append(np.array([np.nextafter(x1, F(0)) if x1 > TINY else x1, 0.5, 0.25, 0.75], F))
    u = np.maximum(np.stack(out).astype(F), TINY)
    u.setflags(write=False)
    return u


# ---- the world of the forms: all the twin follows, under the sky ----------------------------------------------------------------------------------------
def sky_mesh_room(p, as_list=False, builder="BuildBVH_SAH", env=None, rotate_y=EW.SKY_U0_DEGREES, tables=False):
    """a checker floor, a Lambertian and a metal sphere and a small Lambertian mesh (a tetrahedron: a TRI world) under sky_environment(32, 16) at u0 = 0.3;
    tables: the mesh is an icosphere(1) with vertex normals and texture coordinates (beyond the twin: the forms are compared with one another)"""
    s = p.Scene()
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    s.MakeSphere((2.2, 1.0, 5.5), 1.0, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeSphere((8, 1.2, 6), 1.2, s.Metal((0.9, 0.7, 0.4), 0.3))
    m = TW.mesh_io()
    if tables:
        from _nee_worlds import small_image
        v, f = m.icosphere(1)
        s.set_image(small_image())
        s.MakeMesh(v, f, s.ImageTexture(), 1.3, 0.0, (5, 1.5, 6.5), normals=v, uvs=(np.random.default_rng(4).random((len(v), 2)) * 1.5 - 0.25).astype(F))
    else:
        s.MakeMesh(*m.tetrahedron(), s.Lambertian((0.3, 0.4, 0.8)), 1.6, 20.0, (5, 1.4, 6.5))
    s.set_environment(EW.sky_map() if env is None else env, rotate_y=rotate_y)
    if as_list:
        s.MakeHittableList()
    else:
        getattr(s, builder)()
    return s


def quad_light_sky_room(p):
    """sky_mesh_room plus a quad light above it: modes 1 and 16 have a table to sample, mode 32 leaves it to be hit"""
    s = p.Scene()
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s.Lambertian((0.6, 0.6, 0.6)))
    s.MakeSphere((2.2, 1.0, 5.5), 1.0, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeSphere((8, 1.2, 6), 1.2, s.Metal((0.9, 0.7, 0.4), 0.3))
    s.MakeQuad((3.5, 6, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    s.BuildBVH_SAH()
    return s


class Run:
    """a world under a map, and the whole-sample twin's samples of it with the mode on"""

    def __init__(self, scene, w=W, h=H, spp=SPP, depth=DEPTH, first_sample=0):
        p = pkg()
        self.scene = scene
        env, u0 = scene.environment()
        self.env, self.u0 = env, u0
        self.tables = p.api.environment_distribution(env)
        self.stats = {}
        samples, followed = LT.frame_samples(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(EW.camera(p, w, h)), w, h, spp, depth, SEED,
                                             ET.sky_environment(env, u0), light=(self.tables, u0), first_sample=first_sample, stats=self.stats)
        self.samples, self.followed = samples, followed
        self.pixel_followed = followed.all(axis=2)
        self.sums = LT.in_order_sums(np.where(followed[..., None], samples, 0))
        self.frame = LT.resolve(self.sums, spp)
        for a in (self.samples, self.followed, self.pixel_followed, self.sums, self.frame):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(name, as_list=False):
    p = pkg()
    if name == "forms":
        return Run(sky_mesh_room(p, as_list=as_list))
    if name == "sun":
        return Run(sky_mesh_room(p, env=sun_map(), rotate_y=0.0))
    if name == "half_black":
        return Run(sky_mesh_room(p, env=half_black_map()))
    if name == "replaced":   # the forms' world after its map was replaced by the sun
        return Run(sky_mesh_room(p, env=sun_map(), rotate_y=EW.SKY_U0_DEGREES))
    raise KeyError(name)
