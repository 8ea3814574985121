"""The cases and worlds of the microfacet tests — test infrastructure only.

random_cases() / aimed_cases(): inputs of rt_microfacet_batch, shared by the CPU test (host batch against the numpy twin) and the GPU test (device probe against
the host batch).  room(): §28's room refurnished — every world is built through the product's host vocabulary, which needs no device.
"""
import functools

import numpy as np

import _env_tree_twin as VT
import _env_twin as ET
import _env_worlds as EW
import _mfac_twin as MT
import _nmap_worlds as NW
import _tex_worlds as XW
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
HALF = 1 << 23   # the word of u = 0.5, and of a signed draw of 0


def _unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F)


def random_cases(n=4096, seed=29):
    """n cases: unit normals (as float32 rounds them), directions of any length on either side, roughness over [0, 1] with both ends, conductors and coats, tapes
    of 0 to 16 words (a short one ends inside the rule, where the tape serves its accepting word)"""
    rng = np.random.default_rng(seed)
    normal = _unit(rng.standard_normal((n, 3)))
    ray_d = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(F)
    roughness = rng.choice(np.array([0.0, 0.01, 0.2, 0.5, 1.0], F), n).astype(F)
    some = rng.random(n) < 0.5
    roughness[some] = rng.random(int(some.sum())).astype(F)
    f0 = rng.random((n, 3)).astype(F)
    f0[rng.random(n) < 0.1] = F(1.0)
    coat = (rng.random(n) < 0.5).astype(np.uint32)
    tapes = [rng.integers(1, 2 ** 24 + 1, int(k)).astype(np.uint32) for k in rng.integers(0, 17, n)]
    return dict(normal=normal, ray_d=ray_d, roughness=roughness, f0=f0, coat=coat, tapes=tapes)


AIMED = ["backside", "edge on", "co of one ulp", "N = +z", "N = -z", "N.z = -0", "N.z = -0, tilted", "normal incidence, l2 == 0", "roughness below the clamp", "roughness 0",
         "disk point on the rim", "coat toss below F", "coat toss above F", "coat toss at 0.5", "coat with F0 = 1", "absorbed bounce", "an empty tape"]


def _signed(x):
    """the word whose signed draw is x (a multiple of 2^-23)"""
    return int(round(x * 2.0 ** 23)) + HALF


def aimed_cases():
    """one case per name of AIMED, in that order, and the way out each must take (0: whatever the twin says)"""
    z, down = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    slant = (0.3, 0.2, -1.0)
    centre = [HALF, HALF]                                   # the disk's centre: t1 = t2 = 0
    grazing = (1.0, 0.0, -0.05)
    rows = [
        # normal, ray_d, roughness, f0, coat, tape, way
        (z, (0.1, 0.2, 1.0), 0.5, (0.9, 0.8, 0.7), 0, centre, MT.BACKSIDE),
        (z, (1.0, 0.0, 0.0), 0.5, (0.9, 0.8, 0.7), 0, centre, MT.BACKSIDE),
        (z, (1.0, 0.0, -1.4e-45), 0.5, (0.9, 0.8, 0.7), 0, centre, 0),
        (z, slant, 0.5, (0.9, 0.8, 0.7), 0, [_signed(0.25), _signed(-0.5)], MT.SPECULAR),
        ((0.0, 0.0, -1.0), (0.3, 0.2, 1.0), 0.5, (0.9, 0.8, 0.7), 0, [_signed(0.25), _signed(-0.5)], MT.SPECULAR),
        ((1.0, 0.0, -0.0), (-1.0, 0.2, 0.1), 0.5, (0.9, 0.8, 0.7), 0, [_signed(0.25), _signed(-0.5)], MT.SPECULAR),
        ((0.6, 0.8, -0.0), (-1.0, -1.0, 0.1), 0.4, (0.9, 0.8, 0.7), 1, [_signed(-0.25), _signed(0.5), 1], MT.SPECULAR),
        (z, down, 0.5, (0.9, 0.8, 0.7), 0, [_signed(0.5), _signed(0.25)], MT.SPECULAR),
        (z, slant, 0.01, (0.9, 0.8, 0.7), 0, [_signed(0.5), _signed(0.25)], MT.SPECULAR),
        (z, slant, 0.0, (0.9, 0.8, 0.7), 0, [_signed(-0.5), _signed(0.75)], MT.SPECULAR),
        (z, slant, 0.7, (0.9, 0.8, 0.7), 0, [2 ** 24 - 1, HALF], 0),
        (z, down, 0.3, (0.5, 0.0, 0.0), 1, centre + [HALF // 2], MT.SPECULAR),
        (z, down, 0.3, (0.5, 0.0, 0.0), 1, centre + [HALF + HALF // 2], MT.BASE),
        (z, down, 0.3, (0.5, 0.0, 0.0), 1, centre + [HALF], 0),
        (z, slant, 0.3, (1.0, 0.0, 0.0), 1, centre + [2 ** 24], 0),
        (z, grazing, 1.0, (0.9, 0.8, 0.7), 0, None, MT.ABSORBED),
        (z, slant, 0.6, (0.9, 0.8, 0.7), 1, [], 0),
    ]
    assert len(rows) == len(AIMED)
    # the absorbed bounce, found once by a fixed search: the first of 512 seeded pairs of words that sends a grazing view's reflection below a rough surface
    rng = np.random.default_rng(2929)
    words = rng.integers(1, 2 ** 24 + 1, (512, 2)).astype(np.uint32)
    k = len(words)
    _, _, way = MT.scatter(np.tile(z, (k, 1)), np.tile(grazing, (k, 1)), np.full(k, 1.0, F), np.tile((0.9, 0.8, 0.7), (k, 1)), np.zeros(k), MT.CaseTape(list(words)))
    at = AIMED.index("absorbed bounce")
    rows[at] = rows[at][:5] + (list(words[int(np.nonzero(way == MT.ABSORBED)[0][0])]), MT.ABSORBED)
    cols = list(zip(*rows))
    cases = dict(normal=np.array(cols[0], F), ray_d=np.array(cols[1], F), roughness=np.array(cols[2], F), f0=np.array(cols[3], F), coat=np.array(cols[4], np.uint32),
                 tapes=[np.array(t, np.uint32) for t in cols[5]])
    return cases, np.array(cols[6], np.uint32)


def run_cases(fn, cases):
    """fn = api.microfacet_batch, api.probe_microfacet or the twin's case()"""
    c = cases
    return fn(c["normal"], c["ray_d"], c["roughness"], c["f0"], c["coat"], c["tapes"])


# ---- the test room and the kernel forms ------------------------------------------------------------------------------------------------------------------------
SEED = NW.SEED
W, H, SPP, DEPTH = NW.W, NW.H, NW.SPP, NW.DEPTH   # §28's: 24 x 16 at 8 spp and depth 6
ENV_TREE = 48
BACKGROUND = NW.BACKGROUND

# The suite's statement of which MFAC instantiations of render_kernel_stream exist: one (world, exact, ext, big, wide) key per form of the MICROFACET family of
# csrc/rt_device.hip and, the same eight once more, of the MICROFACET_ENV_TREE family: the shapes of §28's family, each with _tri_worlds' recipe.
# tests/test_microfacets_cpu.py holds the list against the source; tests/test_gpu_microfacets.py renders every key, plain and in mode 48, against the twin.
FORMS = dict(NW.FORMS)


def roughness_map():
    """6 x 4 random bytes, for repeat / bilinear: the green channel scales a roughness"""
    return XW.image(6, 4, seed=29)


def room_table():
    """the room's texture table as the twin takes it: entry 0 the mesh's colours, 1 its normal map, 2 its roughness map"""
    return [(XW.image(8, 4, seed=28), 0, 0), (NW.bumps(), 1, 1), (roughness_map(), 1, 1)]


def room(p, env=False, as_list=False, records=True, normal_map=True):
    """A coated checker floor, a rough-conductor sphere and a rough-conductor triangle, a coated image-textured uv_sphere(8, 4) mesh with vertex normals,
    coordinates, a normal map and a roughness map, a fuzzy metal without a record, a glass ball, a quad light — inside a large coated Lambertian sphere, which
    every ray that leaves the room meets from inside: the backside way out, after which it leaves diffusely through the shell — under a constant background
    or, env, the sky map.  records False: the same room without a microfacet record."""
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
    if normal_map:
        s.set_normal_map(mesh, 1, 1.5)
    if records:
        s.set_microfacet(floor, 0.25, 0.3)
        s.set_microfacet(gold, 0.35)
        s.set_microfacet(steel, 0.6)
        s.set_microfacet(shell, 0.5, 0.04)
        s.set_microfacet(mesh, 0.9, 0.2)
        s.set_roughness_map(mesh, 2)
    if env:
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(BACKGROUND)
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


def camera(p, w=W, h=H):
    return EW.camera(p, w, h)


class Run:
    """the room and the whole-sample twin's samples of it, plain (a constant background) or in mode 48 (the sky map and the light tree): with the records
    (samples), without (unrecorded)"""

    def __init__(self, env, as_list=False, spp=SPP, first_sample=0, w=W, h=H):
        p = pkg()
        self.scene = room(p, env=env, as_list=as_list)
        self.table = room_table()
        self.world = as_oracle_world(self.scene.getWorldPtr())
        vn, uv, nmaps, mfacs = self.scene.vertex_normals(), self.scene.texture_coords(), self.scene.normal_maps(), self.scene.microfacets()
        cam = as_oracle_camera(camera(p, w, h))
        if env:
            image, u0 = self.scene.environment()
            sky, light, tree = ET.sky_environment(image, u0), (p.api.environment_distribution(image), u0), VT.table_of(self.world)
        else:
            colour = np.array(BACKGROUND, F)
            sky, light, tree = (lambda d: np.broadcast_to(colour, (len(d), 3))), None, None
        self.stats = {}
        args = (self.world, cam, w, h, spp, DEPTH, SEED, sky, vn, uv, nmaps)
        self.samples, self.followed = MT.frame_samples(*args, mfacs, self.table, light=light, tree=tree, first_sample=first_sample, stats=self.stats)
        self.unrecorded, _ = MT.frame_samples(*args, None, self.table, light=light, tree=tree, first_sample=first_sample)
        self.sums = MT.in_order_sums(self.samples)
        self.frame = MT.resolve(self.sums, spp)
        for a in (self.samples, self.followed, self.unrecorded, self.sums, self.frame):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(env, as_list=False):
    return Run(env, as_list)
