"""The inert tables and the sphere worlds of the surface tests — test infrastructure only.

inert_tables(): a normal-map table of flat maps and a microfacet table whose records on the materials in use are all off, put on a world that is already built.
They run the NMAP and MFAC forms of render_kernel_stream on worlds whose expected frame the CPU oracle gives (media, noise, glass on triangles, moving spheres,
three cameras): §28 promises that a flat map changes no bit of any frame, §29 that a record that is off does.  sphere_room() and random_surface_world(): spheres
under normal maps, image textures and roughness maps — where the kernels take (u, v) from the normal BEFORE the map replaces it and share that (u, v) with the
image lookup and the roughness map — for the whole-sample twin (tests/_rglass_twin.py, which follows every sample of them).  Every world is built through the
product's host vocabulary, which needs no device; run(...) and random_run(...) are computed once per process and never modified.
"""
import functools

import numpy as np

import _env_tree_twin as VT
import _env_twin as ET
import _env_worlds as EW
import _mfac_worlds as MW
import _nmap_worlds as NW
import _rglass_twin as GT
import _tex_worlds as XW
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
SEED = MW.SEED
W, H, SPP, DEPTH = MW.W, MW.H, MW.SPP, MW.DEPTH   # the rooms': 24 x 16 at 8 spp and depth 6
ENV_TREE = 48
BACKGROUND = MW.BACKGROUND
FORMS = dict(NW.FORMS)   # the eight shapes of both families, plain and in mode 48
MAPPABLE = (TW.MAT["lambertian"], TW.MAT["metal"], TW.MAT["checker"], TW.MAT["noise"], TW.MAT["image"])   # what rt_scene_set_normal_map and rt_scene_set_microfacet take
LIVE_RECORDS = 5   # the records of an inert microfacet table: a coat, a conductor, a mapped coat, frosted glass and mapped frosted glass, on materials no primitive uses


# ---- the inert tables ----------------------------------------------------------------------------------------------------------------------------------------
def materials_in_use(scene):
    """the indices of the materials some primitive of the built scene carries"""
    _, prims, _ = scene.arrays()
    quads = scene.quads()
    return np.unique(np.concatenate([(prims["mat"] & np.uint32(0x7fffffff)).astype(np.int64), quads["mat"].astype(np.int64)]))


def takes_a_record(scene):
    """how many materials in use take a normal map (and a microfacet record): Lambertian, checker, noise, image and metal ones"""
    mats = scene.arrays()[2]
    return int(np.isin(mats["type"][materials_in_use(scene)], MAPPABLE).sum())


def inert_tables(scene, normal_maps=True, microfacets=True, bend=False, live=False):
    """Puts the inert tables on a built scene, in place, and returns {'mapped', 'records'} as the renderer's *_info() will count them.

    normal_maps: every material that takes a map gets one, in turn a flat 8 x 8 map (128, 128, 255) under repeat / bilinear at strength 1, a flat 5 x 3 map
    (128, 128, 90) under clamp / nearest at strength 0.7 — _nmap_worlds.room_table(flat=True)'s two — and _nmap_worlds.bumps(), a map that bends, at strength 0.
    The rule runs on every hit up to where it leaves the normal alone: (u, v), tangents, texel fetch, decode.  bend: the first flat map is the bending one at
    strength 1 — the proof that the records are in view.
    microfacets: five more materials that no primitive uses carry live records — a coat, a conductor, a mapped coat, frosted glass, mapped frosted glass —, so
    the table, its count and the header bits are a real table's, and every material in use has none.  live: the materials in use that take one get a record too."""
    mats = scene.arrays()[2]
    types = mats["type"].copy()
    out = {"mapped": 0, "records": 0}
    if normal_maps:
        flat_a = scene.add_image(NW.bumps() if bend else XW.constant(8, 8, (128, 128, 255)), "repeat", "bilinear")
        flat_b = scene.add_image(XW.constant(5, 3, (128, 128, 90)), "clamp", "nearest")
        bent = scene.add_image(NW.bumps(), "repeat", "bilinear")
        turn = [(flat_a, 1.0), (flat_b, 0.7), (bent, 0.0)]
        for m in np.nonzero(np.isin(types, MAPPABLE))[0]:
            image, strength = turn[out["mapped"] % 3]
            scene.set_normal_map(int(m), image, strength)
            out["mapped"] += 1
    if microfacets:
        rough = scene.add_image(MW.roughness_map(), "repeat", "bilinear")
        coat, conductor, mapped = scene.Lambertian((0.5, 0.5, 0.5)), scene.Metal((0.9, 0.7, 0.4), 0.2), scene.Lambertian((0.3, 0.6, 0.4))
        frosted, frosted_mapped = scene.Dielectric((1, 1, 1), 1.5), scene.Dielectric((1, 1, 1), 1.33)
        scene.set_microfacet(coat, 0.3, 0.04).set_microfacet(conductor, 0.4).set_microfacet(mapped, 0.8, 0.2).set_roughness_map(mapped, rough)
        scene.set_rough_glass(frosted, 0.45).set_rough_glass(frosted_mapped, 0.8).set_roughness_map(frosted_mapped, rough)
        out["records"] = LIVE_RECORDS
        if live:
            for m in materials_in_use(scene):
                if types[m] in MAPPABLE:
                    scene.set_microfacet(int(m), 0.3, 0.5)
                    out["records"] += 1
    return out


# ---- sphere_room: spheres under maps ---------------------------------------------------------------------------------------------------------------------------
room_table = MW.room_table   # entry 0 the globes' colours, 1 the normal map (bumps), 2 the roughness map
POLE_CENTRE, POLE_RADIUS = (5.0, 0.6, 5.5), 0.55


def sphere_room(p, env=False, as_list=False, flat=False):
    """Inside §29's large coated shell (every ray that leaves the room meets it from inside: the backside way out) and on its coated checker floor:
    a globe — an image-textured sphere with a normal map and a mapped coat —, a metal sphere with a normal map and a mapped conductor record, a Lambertian
    sphere with a mapped coat and no normal map, a frosted glass ball under the roughness map that rays enter, cross and leave, a small Lambertian sphere with
    a normal map below the camera, which primary rays meet on its upper cap around the pole, a second, smaller globe with a normal map and no microfacet
    record, and a quad light — under a constant background or, env, the sky map.  flat: entry 1 is a flat map of the same size and modes."""
    tab = room_table()
    s = p.Scene()
    floor = s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5)
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), floor)
    shell = s.Lambertian((0.8, 0.8, 0.8))
    s.MakeSphere((5, 0, 5), 30.0, shell)
    s.set_image(tab[0][0])
    one = XW.constant(8, 8, (128, 128, 255)) if flat else tab[1][0]
    assert s.add_image(one, "repeat", "bilinear") == 1 and s.add_image(tab[2][0], "repeat", "bilinear") == 2
    globe, gold, lam = s.ImageTexture(0), s.Metal((0.9, 0.7, 0.4), 0.3), s.Lambertian((0.7, 0.3, 0.3))
    frosted, pole, plain_globe = s.Dielectric((0.95, 0.98, 1.0), 1.5), s.Lambertian((0.4, 0.5, 0.7)), s.ImageTexture(0)
    s.MakeSphere((5, 1.6, 7.5), 1.5, globe)
    s.MakeSphere((8, 1.2, 6), 1.2, gold)
    s.MakeSphere((2.0, 0.9, 6.0), 0.9, lam)
    s.MakeSphere((6.3, 1.0, 3.4), 1.0, frosted)
    s.MakeSphere(POLE_CENTRE, POLE_RADIUS, pole)
    s.MakeSphere((1.0, 0.8, 8.5), 0.8, plain_globe)
    s.MakeQuad((3.5, 6, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    s.set_normal_map(globe, 1, 1.5).set_normal_map(gold, 1, 1.0).set_normal_map(pole, 1, 2.0).set_normal_map(plain_globe, 1, 0.7)
    s.set_microfacet(floor, 0.25, 0.3)
    s.set_microfacet(shell, 0.5, 0.04)
    s.set_microfacet(globe, 0.9, 0.2).set_roughness_map(globe, 2)
    s.set_microfacet(gold, 0.7).set_roughness_map(gold, 2)
    s.set_microfacet(lam, 0.6, 0.3).set_roughness_map(lam, 2)
    s.set_rough_glass(frosted, 0.45).set_roughness_map(frosted, 2)
    if env:
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(BACKGROUND)
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


SPHERE_ROOM_RECORDS = 6   # the floor, the shell, the globe, the gold, the Lambertian ball, the frosted ball


def camera(p, w=W, h=H):
    return EW.camera(p, w, h)


class Run:
    """a world, its tables and the whole-sample twin's samples of it, plain or in mode 48: with every record (samples, stats, info), without the microfacet table
    (unrecorded: the frame of the NMAP family)"""

    def __init__(self, scene, table, cam, w, h, spp, depth, mode48, after_map=False, unrecorded=True):
        p = pkg()
        self.scene, self.table, self.cam, self.args = scene, table, cam, (w, h, spp, depth)
        self.world = as_oracle_world(scene.getWorldPtr())
        vn, uv, nmaps, mfacs = scene.vertex_normals(), scene.texture_coords(), scene.normal_maps(), scene.microfacets()
        sky, light, tree = lights_of(p, scene, self.world, mode48)
        self.stats, self.info = {}, ({"after_map": True} if after_map else {})
        self.twin_args = (self.world, as_oracle_camera(cam), w, h, spp, depth, SEED, sky, vn, uv, nmaps)
        self.lights = dict(light=light, tree=tree)
        self.mfacs = mfacs
        self.samples, self.followed = GT.frame_samples(*self.twin_args, mfacs, table, stats=self.stats, info=self.info, **self.lights)
        self.sums = GT.in_order_sums(self.samples)
        self.frame = GT.resolve(self.sums, spp)
        frozen = [self.samples, self.followed, self.sums, self.frame]
        if unrecorded:
            self.unrecorded, self.unrecorded_followed = GT.frame_samples(*self.twin_args, None, table, **self.lights)
            self.unrecorded_sums = GT.in_order_sums(self.unrecorded)
            frozen += [self.unrecorded, self.unrecorded_followed, self.unrecorded_sums]
        for a in frozen:
            a.setflags(write=False)


def lights_of(p, scene, world, mode48):
    """(sky, light, tree) as the twins take them: the world's constant background or its map as what a miss sees and, mode48, the map and the table as lights"""
    if world.background == 2:
        image, u0 = scene.environment()
        sky = ET.sky_environment(image, u0)
        return (sky, (p.api.environment_distribution(image), u0), VT.table_of(world)) if mode48 else (sky, None, None)
    assert not mode48 and world.background == 1
    colour = np.array(list(world.background_color), F)
    return (lambda d: np.broadcast_to(colour, (len(d), 3))), None, None


@functools.lru_cache(maxsize=None)
def run(env, as_list=False, flat=False, after_map=False):
    p = pkg()
    tab = room_table()
    if flat:
        tab = [tab[0], (XW.constant(8, 8, (128, 128, 255)), 1, 1), tab[2]]
    return Run(sphere_room(p, env=env, as_list=as_list, flat=flat), tab, camera(p), W, H, SPP, DEPTH, env, after_map=after_map, unrecorded=not after_map)


def pole_rays(n=16):
    """n rays straight down the axis of sphere_room's small sphere from above it and n from inside it, whose hits are its two poles EXACTLY: x and z of origin
    and hit are the centre's, so the normal is (0, +-1, 0) and the sphere's tangent (n.z, 0, -n.x) has no length.  No sample of a frame gets there: dot(T, T) > 0
    fails only where n.x^2 + n.z^2 rounds to 0, below 2^-149, so the float32 hit point must have the pole's x and z to the last bit — about one ray in 10^12 of
    those that meet the sphere."""
    rays = np.zeros((2 * n, 7), F)
    rays[:, 0], rays[:, 2] = POLE_CENTRE[0], POLE_CENTRE[2]
    rays[:n, 1], rays[:n, 4] = POLE_CENTRE[1] + np.linspace(1.0, 3.0, n, dtype=F), -1.0      # from above, onto the north pole
    rays[n:, 1], rays[n:, 4] = POLE_CENTRE[1] + np.linspace(-0.2, 0.2, n, dtype=F), -1.0     # from inside, onto the south pole
    return rays


# ---- random worlds of spheres, parallelograms and triangles under random tables --------------------------------------------------------------------------------
SEEDS = tuple(range(8))
SEED_BASE = 31024   # chosen so that every seed has a recorded hit and the union of the seeds takes every way out (tests/test_surfaces_cpu.py checks it)
RW, RH, RSPP, RDEPTH = 16, 12, 4, 6
BUILDERS = ("BuildBVH_SAH", "BuildBVH_TopDown", "MakeHittableList")
STRENGTHS, ROUGHNESSES, SPECULARS = (0.0, 0.5, 1.0, 2.0), (0.0, 0.01, None, 1.0), (0.0, 0.04, 1.0)   # None: a random roughness


def random_surface_world(p, seed, live=False, before_build=None):
    """One world of the randomised surface test: at most 24 primitives — spheres, parallelograms, free triangles with or without vertex normals and
    coordinates (mirrored ones included) — plus at most one uv_sphere(8, 4) mesh, materials of the kinds the twin follows (Lambertian, checker, image, metal,
    glass, light), a texture table of 2 to 5 random images under random modes, random records of all three kinds, a random builder, a constant background or
    the sky map.  live: the same world — the seed's generator is left as it is — plus, from a generator of its own, a noise material under random
    records on a sphere and a parallelogram, moving spheres of the recorded materials, spheres of constant medium (one about the glass ball), a solid glass box
    with an interior record, and a camera of a random kind: the twin with `media` follows it.  Returns (scene, table, camera, recipe); frames are RW x RH at
    RSPP spp and depth RDEPTH.  before_build(s, materials, table), with live: called before the world is built with the scene, a dict of its materials by role
    and the texture table, to which it may append what it adds to the scene (tests/_live_worlds.random_masks: cutout records); it draws from no
    generator of this function."""
    rng = np.random.default_rng(SEED_BASE + seed)
    s = p.Scene()
    table = []
    for k in range(int(rng.integers(2, 6))):
        img = rng.integers(0, 256, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 3)).astype(np.uint8)
        if k % 2:
            img[:, :, 2] = 128 + img[:, :, 2] // 2   # every other image leans outwards as a normal map does; the others bend a normal any way, below the surface too
        wrap, filt = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        if k == 0:
            s.set_image(img)
            s.image_sampling(0, *XW.MODE_NAMES[(wrap, filt)])
        else:
            assert s.add_image(img, *XW.MODE_NAMES[(wrap, filt)]) == k
        table.append((img, wrap, filt))
    n_img = len(table)
    pick = lambda: int(rng.integers(0, n_img))   # noqa: E731
    image_of = {}   # which image each image material names

    def image_material():
        k = pick()
        m = s.ImageTexture(k)
        image_of[m] = k
        return m
    surface = [s.Lambertian(rng.random(3)), s.Lambertian(rng.random(3)), s.LambertianTexture(rng.random(3), rng.random(3), float(rng.choice([0.5, 1.3]))),
               image_material(), image_material(), s.Metal(rng.random(3), float(rng.choice([0.0, 0.3]))), s.Metal(rng.random(3), 0.1)]
    glass = [s.Dielectric((1, 1, 1), 1.5), s.Dielectric(0.8 + 0.2 * rng.random(3), 1.33)]
    records = {"normal_maps": 0, "microfacets": 0, "roughness_maps": 0, "rough_glass": 0}
    for m in surface:
        if rng.random() < 0.6:
            s.set_normal_map(m, pick(), float(rng.choice(STRENGTHS)))
            records["normal_maps"] += 1
        if rng.random() < 0.6:
            r = ROUGHNESSES[int(rng.integers(0, 4))]
            s.set_microfacet(m, float(rng.random()) if r is None else r, float(rng.choice(SPECULARS)))
            records["microfacets"] += 1
            if rng.random() < 0.5:
                s.set_roughness_map(m, pick())
                records["roughness_maps"] += 1
    for m in glass:
        if rng.random() < 0.7:
            r = ROUGHNESSES[int(rng.integers(0, 4))]
            s.set_rough_glass(m, float(rng.random()) if r is None else r)
            records["rough_glass"] += 1
            if rng.random() < 0.5:
                s.set_roughness_map(m, pick())
                records["roughness_maps"] += 1
    mats = surface + glass
    any_mat = lambda: mats[int(rng.integers(0, len(mats)))]   # noqa: E731
    n_spheres, n_quads, n_tris = int(rng.integers(4, 11)), int(rng.integers(2, 6)), int(rng.integers(2, 9))
    for k in range(n_spheres):   # the first a ball of glass, large enough that rays cross it
        c = ((rng.random(3) * 2 - 1) * np.array([4, 1.5, 4])).astype(F)
        ball = c if k == 0 else ball
        s.MakeSphere(c, float(rng.choice([0.3, 0.8, 1.4][int(k == 0):])), glass[int(rng.integers(0, 2))] if k == 0 else any_mat())
    s.MakeQuad((-8, -2.2, -8), (16, 0, 0), (0, 0, 16), surface[int(rng.integers(0, len(surface)))])   # a floor, so that paths go on
    s.MakeQuad((-1.5, 5.0, -1.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    for _ in range(n_quads - 2):
        Q = ((rng.random(3) * 2 - 1) * np.array([5, 2, 5])).astype(F)
        s.MakeQuad(Q, (rng.standard_normal(3) * 1.5).astype(F), (rng.standard_normal(3) * 1.5).astype(F), any_mat())
    shapes = {"flat": 0, "smooth": 0, "uv": 0, "mirrored": 0}
    for _ in range(n_tris):
        a = ((rng.random(3) * 2 - 1) * np.array([5, 2, 5])).astype(F)
        e1, e2 = (rng.standard_normal(3) * 1.8).astype(F), (rng.standard_normal(3) * 1.8).astype(F)
        normals = uvs = None
        if rng.random() < 0.5:
            flat_n = np.cross(e1.astype(np.float64), e2.astype(np.float64))
            flat_n /= max(np.linalg.norm(flat_n), 1e-12)
            normals = (flat_n[None, :] + 0.4 * rng.standard_normal((3, 3))).astype(F)
            shapes["smooth"] += 1
        if rng.random() < 0.6:
            uvs = (rng.random((3, 2)) * 2 - 0.5).astype(F)
            if rng.random() < 0.5:
                uvs = uvs[[0, 2, 1]]
            d1, d2 = uvs[1] - uvs[0], uvs[2] - uvs[0]
            shapes["uv"] += 1
            shapes["mirrored"] += int(d1[0] * d2[1] - d2[0] * d1[1] < 0)
        shapes["flat"] += int(normals is None and uvs is None)
        s.MakeTriangle(a, a + e1, a + e2, any_mat(), normals=normals, uvs=uvs)
    mesh = bool(rng.random() < 0.5)
    if mesh:
        v, f, n, uv = TW.mesh_io().uv_sphere(8, 4)
        c = ((rng.random(3) * 2 - 1) * np.array([3, 1, 3])).astype(F)
        s.MakeMesh(v, f, surface[int(rng.integers(0, len(surface)))], float(rng.uniform(0.8, 1.6)), float(rng.uniform(-180, 180)), c, normals=n,
                   uvs=uv * F(rng.uniform(0.5, 2.0)) - F(rng.uniform(0.0, 0.5)))
    extra = None
    if live:
        lr = np.random.default_rng(SEED_BASE + seed + (33 << 20))
        s.set_perlin(int(lr.integers(0, 1 << 30)))
        noise = s.NoiseTexture(float(lr.choice([0.5, 2.0, 4.0])), lr.random(3))
        if lr.random() < 0.7:
            s.set_normal_map(noise, int(lr.integers(0, n_img)), float(lr.choice(STRENGTHS)))
        if lr.random() < 0.7:
            s.set_microfacet(noise, float(lr.random()), float(lr.choice(SPECULARS)))
            if lr.random() < 0.5:
                s.set_roughness_map(noise, int(lr.integers(0, n_img)))
        place = lambda: ((lr.random(3) * 2 - 1) * np.array([4, 1.5, 4])).astype(F)   # noqa: E731
        s.MakeSphere(place(), float(lr.choice([0.5, 1.0])), noise)
        s.MakeQuad(place(), (lr.standard_normal(3) * 1.5).astype(F), (lr.standard_normal(3) * 1.5).astype(F), noise)
        n_moving = int(lr.integers(1, 4))
        for _ in range(n_moving):
            c = place()
            s.MakeMovingSphere(c, c + (lr.random(3).astype(F) - F(0.5)), float(lr.choice([0.4, 0.9])), surface[int(lr.integers(0, len(surface)))])
        n_media = int(lr.integers(1, 4))
        for k in range(n_media):   # the first about the glass ball of the world, the others anywhere: thin haze or a dense ball
            c = ball if k == 0 else place()
            s.MakeSphere(c, float(lr.choice([0.6, 1.2, 3.0])), s.Isotropic(lr.random(3), float(lr.choice([0.05, 0.5, 2.0]))))
        lo = place()
        s.MakeBox(lo, lo + lr.uniform(0.5, 2.0, 3), glass[0], rotate_y=float(lr.uniform(0, 90)))
        s.set_interior(glass[0], sigma=lr.choice([0.0, 0.1, 1.0], 3) * lr.random(3))
        extra = {"moving": n_moving, "media": n_media, "camera": TW.CAMERAS[int(lr.integers(0, 3))]}
        if before_build is not None:
            extra["masks"] = before_build(s, dict(surface=surface, image_of=image_of, noise=noise, clear=glass[1]), table)
    env = bool(rng.random() < 0.5)
    if env:
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    else:
        s.set_background(tuple(float(x) for x in 0.2 + 0.6 * rng.random(3)))
    builder = BUILDERS[int(rng.integers(0, 3))]
    getattr(s, builder)()
    angle = rng.uniform(0, 2 * np.pi)
    eye = np.array([9 * np.cos(angle), rng.uniform(0.5, 4.0), 9 * np.sin(angle)], F)
    fov = float(rng.uniform(45, 75))
    cam = p.PinholeCamera(eye, (0, 0, 0), (0, 1, 0), fov, RW / RH)
    if extra is not None and extra["camera"] == "defocus":
        cam = p.DefocusBlurCamera(eye, (0, 0, 0), (0, 1, 0), fov, RW / RH, float(lr.uniform(0.05, 0.5)), float(lr.uniform(4, 12)))
    elif extra is not None and extra["camera"] == "motion":
        cam = p.MotionBlurCamera(eye, (0, 0, 0), (0, 1, 0), fov, RW / RH, 0.0, 1.0)
    recipe = {"seed": seed, "images": [(t[0].shape[1], t[0].shape[0], t[1], t[2]) for t in table], "records": records, "spheres": n_spheres, "quads": n_quads,
              "triangles": shapes, "mesh": mesh, "env": env, "builder": builder, "eye": eye.tolist(), "fov": fov, "frame": (RW, RH, RSPP, RDEPTH)}
    if extra is not None:
        recipe["live"] = extra
    return s, table, cam, recipe


class RandomRun:
    def __init__(self, seed):
        p = pkg()
        scene, table, cam, self.recipe = random_surface_world(p, seed)
        self.env = self.recipe["env"]
        self.as_list = self.recipe["builder"] == "MakeHittableList"
        self.plain = Run(scene, table, cam, RW, RH, RSPP, RDEPTH, False, unrecorded=False)
        self.mode48 = Run(scene, table, cam, RW, RH, RSPP, RDEPTH, True, unrecorded=False) if self.env else None


@functools.lru_cache(maxsize=None)
def random_run(seed):
    return RandomRun(seed)
