"""The cases and worlds of the cutout tests — test infrastructure only.

batches(): inputs of rt_cutout_batch over the three sources of coordinates, shared by the CPU test (host batch against the numpy twin) and the GPU test (device
probe against the host batch).  room(): a checker wall behind a lattice-masked parallelogram, a masked mesh with texture coordinates and a masked plain triangle in
front of a glass and a metal sphere, under a pinhole camera.  Every world is built through the product's host vocabulary, which needs no device.
"""
import functools

import numpy as np

import _cutout_twin as CT
import _env_tree_twin as VT
import _env_worlds as EW
import _interior_worlds as IW
import _path_twin as PT
import _tex_twin as XT
import _uv_twin as UT
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
SEED = EW.SEED
W, H, SPP, DEPTH = 24, 16, 8, 8
ENV_TREE = 48
BACKGROUND = IW.BACKGROUND
FORMS = dict(IW.FORMS)   # one key per form of the CUTOUT family of csrc/rt_device.hip's kernel table and, once more, of its CUTOUT_ENV_TREE family: §32's shapes
EYE = (0.0, 2.0, 8.0)
RECORDS = 3


def image_io():
    pkg()
    from ray_tracing_v06_amd import image_io as m
    return m


def grey(values):
    """a mask image [H][W][3] uint8 from its opacities [H][W]"""
    a = np.asarray(values, np.uint8)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, axis=2))


# ---- the rule's cases --------------------------------------------------------------------------------------------------------------------------------------------
def case_table():
    """the masks of the batches: a lattice under nearest / clamp, random opacities under bilinear / repeat, a 1 x 1 mask, a 3 x 2 mask, and one more lattice
    under bilinear / clamp; entry 0 is the empty entry that stands for a world's image"""
    rng = np.random.default_rng(34)
    return [(None, XT.CLAMP, XT.NEAREST), (image_io().lattice_mask(16, 8, 3, 2, 0.4), XT.CLAMP, XT.NEAREST), (grey(rng.integers(0, 256, (5, 7))), XT.REPEAT, XT.BILINEAR),
            (grey([[128]]), XT.REPEAT, XT.NEAREST), (grey([[0, 255, 90], [200, 128, 30]]), XT.CLAMP, XT.NEAREST), (image_io().lattice_mask(9, 9, 2, 2, 0.5), XT.CLAMP, XT.BILINEAR)]


def case_records():
    """one record per 'material' of the batches: off, then every mask at cutoffs 0, 1, 1/2 and the value of its 1 x 1 texel"""
    texel = F(128) * XT.SCALE
    rows = [(0, 0, 0.0, 0)] + [(1, image, cutoff, 0) for image in range(1, 6) for cutoff in (0.0, 1.0, 0.5, float(texel), 0.25)]
    return np.array(rows, CT.CUTOUT_DT)


def surfaces(p, n, seed, triangle):
    """n random records of capi.QUAD_DT as the scene packs them (one world of n surfaces), and rays that meet their planes near them: (quads, rays (n, 6), t)"""
    rng = np.random.default_rng(seed)
    s = p.Scene()
    mat = s.Lambertian((0.5, 0.5, 0.5))
    for _ in range(n):
        Q = rng.uniform(-3, 3, 3)
        u, v = rng.standard_normal(3) * rng.uniform(0.2, 3), rng.standard_normal(3) * rng.uniform(0.2, 3)
        if triangle:
            s.MakeTriangle(Q, Q + u, Q + v, mat)
        else:
            s.MakeQuad(Q, u, v, mat)
    s.MakeHittableList()
    quads = s.quads().copy()
    a, b = rng.uniform(-0.3, 1.3, n), rng.uniform(-0.3, 1.3, n)   # some of them outside the surface: the rule is asked what it is asked
    target = quads["Q"].astype(np.float64) + quads["u"] * a[:, None] + quads["v"] * b[:, None]
    o = target + quads["normal"] * rng.uniform(0.5, 4, n)[:, None] * rng.choice([-1.0, 1.0], n)[:, None] + rng.standard_normal((n, 3)) * 0.7
    t = rng.uniform(0.3, 3, n)
    d = (target - o) / t[:, None]
    return quads, np.ascontiguousarray(np.concatenate([o, d], axis=1), F), t.astype(F)


@functools.lru_cache(maxsize=None)
def batches(n=1536):
    """[(name, quads, uv or None, rays, t, material)]: a parallelogram, a triangle under a record of coordinates, a triangle under the identity record"""
    p = pkg()
    rng = np.random.default_rng(35)
    n_records = len(case_records())
    out = []
    for name, triangle, seed in (("parallelogram", False, 1), ("triangle, coordinates", True, 2), ("triangle, identity", True, 3)):
        quads, rays, t = surfaces(p, n, seed, triangle)
        uv = None
        if name.endswith("coordinates"):
            uv = rng.uniform(-1.5, 2.5, (n, 3, 2)).astype(F)
        elif name.endswith("identity"):
            uv = np.broadcast_to(UT.IDENTITY, (n, 3, 2)).astype(F)
        out.append((name, quads, uv, rays, t, rng.integers(0, n_records, n).astype(np.uint32)))
    return out


# ---- the test room -----------------------------------------------------------------------------------------------------------------------------------------------
def masks():
    """the room's masks, as (image, wrap, filter) by name"""
    io = image_io()
    return {"fence": (io.lattice_mask(32, 16, 6, 3, 0.3), "clamp", "nearest"), "card": (io.lattice_mask(8, 8, 2, 2, 0.35), "repeat", "bilinear"),
            "wedge": (grey([[0, 255, 0], [255, 0, 255]]), "clamp", "nearest"), "white": (grey([[255]]), "clamp", "nearest"), "black": (grey([[0]]), "clamp", "nearest")}


def room(p, env=False, as_list=False, fence=True, uvs=True, records=True, live=False):
    """A floor, a checker wall and a quad light; a lattice-masked parallelogram in front of the wall; a glass and a metal sphere behind a masked plain triangle and
    a masked card of two triangles with texture coordinates (uvs False: without them — the world then has no table of coordinates), the card's triangles being
    the world's last; under a constant background or, env, the sky map.  fence False: the room without the parallelogram (its material stays); records False:
    no cutout record.  live: every other kind of record beside the masks — a tinted solid-glass box with an interior record in front of the fence, a rough
    conductor's microfacet record on the metal sphere and a glossy coat on the card's own material, which is masked too — so that a CUT form reads a
    sub-header whose three lanes are all live."""
    s = p.Scene()
    images = {name: s.add_image(img, wrap=wrap, filter=filt) for name, (img, wrap, filt) in masks().items()}
    floor, wall, light = s.Lambertian((0.6, 0.55, 0.5)), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 1.3), s.DiffuseLight((5, 5, 5))
    fence_mat, card_mat, wedge_mat = s.Lambertian((0.7, 0.5, 0.3)), s.Lambertian((0.3, 0.7, 0.3)), s.Metal((0.8, 0.6, 0.5), 0.1)
    glass, metal = s.Dielectric((1, 1, 1), 1.5), s.Metal((0.8, 0.8, 0.9), 0.05)
    s.MakeQuad((-10, 0, -6), (20, 0, 0), (0, 0, 16), floor)
    s.MakeQuad((-7, 0, -4), (9, 0, 0), (0, 6, 0), wall)
    s.MakeQuad((-2, 7, -2), (4, 0, 0), (0, 0, 4), light)
    if fence:
        s.MakeQuad((-6, 0, 0), (7, 0, 0), (0, 4.5, 0), fence_mat)
    s.MakeSphere((2.6, 1.0, 0.0), 1.0, glass)
    s.MakeSphere((4.6, 1.0, -1.0), 1.0, metal)
    s.MakeTriangle((1.6, 0.2, 3.0), (5.6, 0.2, 3.0), (3.6, 3.9, 3.0), wedge_mat)
    v = np.array([(1.2, 0.3, 1.5), (3.8, 0.3, 1.5), (3.8, 3.4, 1.5), (1.2, 3.4, 1.5)], F)
    f = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
    s.MakeMesh(v, f, card_mat, uvs=np.array([(0, 0), (2, 0), (2, 2), (0, 2)], F) if uvs else None)
    box = None
    if live:
        box = s.Dielectric((1, 1, 1), 1.5)
        s.MakeBox((-4.6, 0.05, 1.4), (-3.0, 1.7, 3.0), box, rotate_y=20.0)
        s.set_interior(box, color=(0.4, 0.8, 0.6), at=1.0)
        s.set_microfacet(metal, 0.3)
        s.set_microfacet(card_mat, 0.25, 0.04)
    if records:
        s.set_cutout(fence_mat, images["fence"]).set_cutout(card_mat, images["card"], 0.5).set_cutout(wedge_mat, images["wedge"], 0.25)
    if env:
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(BACKGROUND)
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    s.names = dict(images=images, fence=fence_mat, card=card_mat, wedge=wedge_mat, light=light, glass=glass, box=box)
    return s


def camera(p, w=W, h=H):
    return p.PinholeCamera(EYE, (0.0, 2.0, -4.0), (0, 1, 0), 50.0, w / h)


def twin_table(scene):
    """the scene's texture table as the twins take one: [(image [H][W][3] or None, wrap, filter), ...]"""
    records, texels = scene.textures()
    return [(texels[r["first"]:r["first"] + r["width"] * r["height"]].reshape(r["height"], r["width"], 3) if r["width"] else None, int(r["wrap"]), int(r["filter"]))
            for r in records]


def all_of(p, scene, image):
    """a table with mask `image` on every material that takes a record"""
    types = scene.arrays()[2]["type"]
    t = np.zeros(len(types), p.capi.CUTOUT_DT)
    for i, kind in enumerate(types):
        if kind not in (4, 5):
            t[i] = (1, image, 0.5, 0)
    return t


def twin_frame(scene, cutouts, env, spp=SPP, stats=None, first_sample=0, interiors=None):
    """the twin's samples of `scene` under the table `cutouts` (None: the plain walk of _tri_twin): (samples, followed).  The scene's interior and microfacet
    records, where it has any, go to the one loop of _path_twin as its `interiors` (or the table given here) and `mfacs` arguments, with the cutout walk as the
    unwrapped `trace`."""
    p = pkg()
    world = as_oracle_world(scene.getWorldPtr())
    cam = as_oracle_camera(camera(p))
    sky, light, tree = IW.GT_lights(p, scene, world, env)
    uv = scene.texture_coords()
    uv = uv if uv is not None and len(uv) else None
    table = twin_table(scene)
    if cutouts is None:
        import _tri_twin as TT
        trace = TT.closest_intersection
    else:
        trace = CT.walk_of(uv, np.asarray(cutouts), table, stats, EYE)
    rule = VT.MapRule(world, light, tree) if light is not None else None
    interiors, mfacs = scene.interiors() if interiors is None else interiors, scene.microfacets()

    def radiance(g, s):
        return PT.radiance(world, cam, W, H, DEPTH, SEED, g, s, trace, sky=sky, rule=rule, tex=(uv, table), mfacs=mfacs, glass=True, interiors=interiors)
    return PT.frame_samples(radiance, W, H, spp, first_sample)


def facing_frame(scene, cutouts, env, spp=SPP):
    """the twin's samples of `scene` by the other road: the cutout walk wrapped by _interior_twin.solid_walk, which folds the facing of the interior records into
    the normal, through _rglass_twin.radiance without an `interiors` argument — the facing alone, no absorption: (samples, followed)"""
    import _interior_twin as IT
    import _rglass_twin as RG
    p = pkg()
    world = as_oracle_world(scene.getWorldPtr())
    cam = as_oracle_camera(camera(p))
    sky, light, tree = IW.GT_lights(p, scene, world, env)
    uv = scene.texture_coords()
    uv = uv if uv is not None and len(uv) else None
    table = twin_table(scene)
    trace = IT.solid_walk(CT.walk_of(uv, np.asarray(cutouts), table), scene.interiors())
    return PT.frame_samples(lambda g, s: RG.radiance(world, cam, W, H, DEPTH, SEED, g, s, sky, light, tree, (uv, table), scene.microfacets(), None, None, trace), W, H, spp)


class Run:
    """the room and the twin's samples of it, plain or in mode 48: under its records (samples, sums, frame) and without the table (off_sums); live: the room with
    an interior and two microfacet records beside the masks, and facing_sums, its frame with every sigma zero by the road of the wrapped walk"""

    def __init__(self, env, as_list=False, uvs=True, live=False):
        p = pkg()
        self.scene = room(p, env=env, as_list=as_list, uvs=uvs, live=live)
        self.cutouts = self.scene.cutouts().copy()
        self.stats = CT.new_stats()
        self.samples, self.followed = twin_frame(self.scene, self.cutouts, env, stats=self.stats)
        off, self.off_followed = twin_frame(self.scene, None, env)
        self.sums, self.off_sums = VT.in_order_sums(self.samples), VT.in_order_sums(off)
        self.frame = VT.resolve(self.sums, SPP)
        if live:   # with every sigma zero, by the walk that _interior_twin.solid_walk wraps: the facing alone
            facing, self.facing_followed = facing_frame(self.scene, self.cutouts, env)
            self.facing_sums = VT.in_order_sums(facing)
            self.facing_sums.setflags(write=False)
        for a in (self.samples, self.followed, self.sums, self.off_sums, self.frame, self.cutouts):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(env, as_list=False, uvs=True, live=False):
    return Run(env, as_list, uvs, live)
