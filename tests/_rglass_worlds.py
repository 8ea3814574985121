"""The cases and worlds of the rough-glass tests — test infrastructure only.

random_cases() / aimed_cases(): inputs of rt_rough_glass_batch, shared by the CPU test (host batch against the numpy twin) and the GPU test (device probe against
the host batch).  room(): §29's room with a frosted ball, which rays enter and leave, and a frosted pane under the room's roughness map.
"""
import functools

import numpy as np

import _env_tree_twin as VT
import _env_twin as ET
import _env_worlds as EW
import _mfac_worlds as MW
import _rglass_twin as GT
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
HALF = MW.HALF
_unit, _signed = MW._unit, MW._signed


def random_cases(n=4096, seed=30):
    """n cases: unit normals, directions of any length on either side, roughness over [0, 1] with both ends, indices of water, glass, diamond and — no interface at
    all — 1, tapes of 0 to 16 words (a short one ends inside the rule, where the tape serves its accepting word)"""
    rng = np.random.default_rng(seed)
    normal = _unit(rng.standard_normal((n, 3)))
    ray_d = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(F)
    roughness = rng.choice(np.array([0.0, 0.01, 0.2, 0.5, 1.0], F), n).astype(F)
    some = rng.random(n) < 0.5
    roughness[some] = rng.random(int(some.sum())).astype(F)
    ior = rng.choice(np.array([1.0, 1.33, 1.5, 2.4], F), n).astype(F)
    tapes = [rng.integers(1, 2 ** 24 + 1, int(k)).astype(np.uint32) for k in rng.integers(0, 17, n)]
    return dict(normal=normal, ray_d=ray_d, roughness=roughness, ior=ior, tapes=tapes)


AIMED = ["reflected at normal incidence", "transmitted at normal incidence", "toss at F exactly goes through", "edge on", "co of one ulp", "back face, transmitted",
         "back face, reflected", "total reflection", "total reflection, rough", "roughness 0", "N = -z", "an empty tape", "index 1", "absorbed mirror, front",
         "absorbed mirror, back", "absorbed refraction, back"]
# name: (back face, mirrored).  A ray refracted into the denser side cannot come out absorbed: with eta <= 1, sqrt(k) >= eta ch, so w = (-v) eta - M (sqrt(k) - eta ch)
# has dot(n, w) <= 0 for every M of the upper hemisphere; from inside, eta > 1, it can
SEARCHED = {"absorbed mirror, front": (False, True), "absorbed mirror, back": (True, True), "absorbed refraction, back": (True, False)}


def aimed_cases():
    """one case per name of AIMED, in that order, the way out each must take (0: whatever the twin says) and the names of those that must be total reflections"""
    z, down, up = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)
    slant = (0.3, 0.2, -1.0)
    centre = [HALF, HALF]                                   # the disk's centre: t1 = t2 = 0, M = n
    steep = (0.9, 0.0, 0.45)                                # from inside, 63 degrees off the normal: beyond the critical angle of 1.5
    f0 = float(F(F(F(1) - F(1) / F(1.5)) / F(F(1) + F(1) / F(1.5))) ** 2)   # ~0.04: the toss words below and above it
    at_f = int(np.ceil(f0 * 2.0 ** 24))
    rows = [
        # normal, ray_d, roughness, ior, tape, way
        (z, down, 0.3, 1.5, centre + [1], GT.SPECULAR),
        (z, down, 0.3, 1.5, centre + [2 ** 24], GT.TRANSMITTED),
        (z, down, 0.3, 1.5, centre + [at_f], 0),
        (z, (1.0, 0.0, 0.0), 0.5, 1.5, centre, GT.BASE),
        (z, (1.0, 0.0, -1.4e-45), 0.5, 1.5, centre, 0),
        (z, up, 0.3, 1.5, centre + [2 ** 24], GT.TRANSMITTED),
        (z, up, 0.3, 1.5, centre + [1], GT.SPECULAR),
        (z, steep, 0.0, 1.5, centre + [2 ** 24], GT.SPECULAR),
        (z, steep, 0.15, 1.5, [_signed(0.25), _signed(-0.25), 2 ** 24], 0),
        (z, slant, 0.0, 1.5, [_signed(-0.5), _signed(0.75), HALF], GT.TRANSMITTED),
        (down, (0.3, 0.2, 1.0), 0.5, 1.5, [_signed(0.25), _signed(-0.5), HALF], GT.TRANSMITTED),
        (z, slant, 0.6, 1.5, [], 0),
        (z, slant, 0.5, 1.0, [_signed(0.25), _signed(-0.5), 1], GT.TRANSMITTED),
    ] + [None] * len(SEARCHED)
    assert len(rows) == len(AIMED)
    # the absorbed cases, found once each by a fixed search: the first of 4096 seeded triples of words that sends a grazing view's mirrored or refracted ray to the
    # wrong side of a surface of roughness 1
    rng = np.random.default_rng(3030)
    words = rng.integers(1, 2 ** 24 + 1, (4096, 3)).astype(np.uint32)
    k = len(words)
    for name, (back, mirrored) in SEARCHED.items():
        d = (1.0, 0.0, 0.05) if back else (1.0, 0.0, -0.05)
        detail = {}
        _, _, way = GT.scatter(np.tile(z, (k, 1)), np.tile(d, (k, 1)), np.full(k, 1.0, F), np.full(k, 1.5, F), GT.CaseTape(list(words)), detail=detail)
        found = np.nonzero((way == GT.ABSORBED) & (detail["mirror"] == mirrored))[0]
        assert len(found), name
        rows[AIMED.index(name)] = (z, d, 1.0, 1.5, list(words[int(found[0])]), GT.ABSORBED)
    cols = list(zip(*rows))
    cases = dict(normal=np.array(cols[0], F), ray_d=np.array(cols[1], F), roughness=np.array(cols[2], F), ior=np.array(cols[3], F),
                 tapes=[np.array(t, np.uint32) for t in cols[4]])
    return cases, np.array(cols[5], np.uint32), ("total reflection",)


def run_cases(fn, cases):
    """fn = api.rough_glass_batch, api.probe_rough_glass or the twin's case()"""
    c = cases
    return fn(c["normal"], c["ray_d"], c["roughness"], c["ior"], c["tapes"])


# ---- the test room -----------------------------------------------------------------------------------------------------------------------------------------------
SEED = MW.SEED
W, H, SPP, DEPTH = MW.W, MW.H, MW.SPP, MW.DEPTH   # 24 x 16 at 8 spp and depth 6
ENV_TREE = 48
BACKGROUND = MW.BACKGROUND
FORMS = dict(MW.FORMS)
room_table = MW.room_table


def room(p, env=False, as_list=False, glass_records=True, records=True, normal_map=True):
    """_mfac_worlds.room object for object, and then a frosted ball (rays enter it, cross it and leave it: the back face, and total reflection inside) and a
    frosted pane, a quad under the room's roughness map (entry 2), before the camera.  glass_records False: both are clear glass, and the room is §29's with two
    more glass things in it."""
    tab = room_table()
    s = p.Scene()
    floor = s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5)
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), floor)
    gold, steel, fuzzy = s.Metal((0.9, 0.7, 0.4), 0.3), s.Metal((0.6, 0.7, 0.8), 0.0), s.Metal((0.8, 0.8, 0.9), 0.05)
    s.MakeSphere((8, 1.2, 6), 1.2, gold)
    s.MakeTriangle((0.5, 0.0, 9.5), (8.5, 0.0, 10.0), (1.5, 4.5, 9.5), steel)
    s.MakeSphere((2.0, 0.8, 6.0), 0.8, fuzzy)
    s.MakeSphere((3.4, 0.7, 3.8), 0.7, s.Dielectric((1, 1, 1), 1.5))
    shell = s.Lambertian((0.8, 0.8, 0.8))
    s.MakeSphere((5, 0, 5), 30.0, shell)
    s.set_image(tab[0][0])
    assert s.add_image(tab[1][0], "repeat", "bilinear") == 1 and s.add_image(tab[2][0], "repeat", "bilinear") == 2
    mesh = s.ImageTexture(0)
    v, f, n, uv = TW.mesh_io().uv_sphere(8, 4)
    s.MakeMesh(v, f, mesh, 1.5, 20.0, (5, 1.6, 6.5), normals=n, uvs=uv * F(2.0) - F(0.25))
    s.MakeQuad((3.5, 6, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    frosted, pane = s.Dielectric((0.95, 0.98, 1.0), 1.5), s.Dielectric((1.0, 0.95, 0.9), 1.33)
    s.MakeSphere((6.3, 1.0, 3.4), 1.0, frosted)
    s.MakeQuad((3.9, 1.9, 2.6), (1.7, 0, 0.2), (0, 1.5, 0.5), pane)
    if normal_map:
        s.set_normal_map(mesh, 1, 1.5)
    if records:
        s.set_microfacet(floor, 0.25, 0.3)
        s.set_microfacet(gold, 0.35)
        s.set_microfacet(steel, 0.6)
        s.set_microfacet(shell, 0.5, 0.04)
        s.set_microfacet(mesh, 0.9, 0.2)
        s.set_roughness_map(mesh, 2)
    if glass_records:
        s.set_rough_glass(frosted, 0.45)
        s.set_rough_glass(pane, 0.8)
        s.set_roughness_map(pane, 2)
    if env:
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(BACKGROUND)
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


def camera(p, w=W, h=H):
    return EW.camera(p, w, h)


def lights_of(p, scene, world, env):
    """(sky, light, tree) as the twins take them: a constant background, or mode 48's map and table"""
    if env:
        image, u0 = scene.environment()
        return ET.sky_environment(image, u0), (p.api.environment_distribution(image), u0), VT.table_of(world)
    colour = np.array(BACKGROUND, F)
    return (lambda d: np.broadcast_to(colour, (len(d), 3))), None, None


class Run:
    """the room and the whole-sample twin's samples of it, plain or in mode 48: with every record (samples), with the glass records off (clear: the table's other
    records stay)"""

    def __init__(self, env, as_list=False, spp=SPP, first_sample=0, w=W, h=H):
        p = pkg()
        self.scene = room(p, env=env, as_list=as_list)
        self.table = room_table()
        self.world = as_oracle_world(self.scene.getWorldPtr())
        vn, uv, nmaps, mfacs = self.scene.vertex_normals(), self.scene.texture_coords(), self.scene.normal_maps(), self.scene.microfacets()
        cam = as_oracle_camera(camera(p, w, h))
        sky, light, tree = lights_of(p, self.scene, self.world, env)
        self.stats = {}
        self.args = (self.world, cam, w, h, spp, DEPTH, SEED, sky, vn, uv, nmaps)
        self.lights = dict(light=light, tree=tree)
        self.mfacs = mfacs.copy()
        self.mfacs_clear = clear_glass(mfacs)
        self.samples, self.followed = GT.frame_samples(*self.args, mfacs, self.table, light=light, tree=tree, first_sample=first_sample, stats=self.stats)
        self.clear, _ = GT.frame_samples(*self.args, self.mfacs_clear, self.table, light=light, tree=tree, first_sample=first_sample)
        self.sums, self.clear_sums = GT.in_order_sums(self.samples), GT.in_order_sums(self.clear)
        self.frame, self.clear_frame = GT.resolve(self.sums, spp), GT.resolve(self.clear_sums, spp)
        for a in (self.samples, self.followed, self.clear, self.sums, self.frame, self.clear_sums, self.clear_frame, self.mfacs, self.mfacs_clear):
            a.setflags(write=False)


def clear_glass(mfacs):
    """the table with its rough-glass records off"""
    out = mfacs.copy()
    out[np.isin(out["on"], (GT.GLASS, GT.GLASS_MAPPED))] = (0, 0, 0.0, 0.0)
    return out


@functools.lru_cache(maxsize=None)
def run(env, as_list=False):
    return Run(env, as_list)
