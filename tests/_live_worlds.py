"""The room of the live-surface tests and the extended twin's frames of it — test infrastructure only.

room(): _tri_worlds.wide_room's contents — the open room, its quad light, the meshes, the glass icosphere, the noise and image triangles, the sphere of medium —
plus live records on primitives that rays reach, beside everything the surface families had only met under inert tables: a noise parallelogram under a coat, a
noise sphere under a normal map, a moving sphere under a normal map and a mapped coat, a moving rough conductor, a frosted glass ball with a medium inside it, a
solid tinted glass box that a sphere of medium pokes through — under the three cameras of _tri_worlds.CAMERAS.  The whole-sample twin (tests/_path_twin.py with
`media`), pinned to the CPU oracle by tests/test_path_twin_oracle_cpu.py, follows EVERY sample of it.

Mode 48 refuses a world with a constant medium (include/rt06.h: RT_LIGHT_SAMPLING_ENV_TREE), so the room under the sky map is built without its three media; every
other live record, the moving spheres and the cameras stay.  run(...) is computed once per process and never modified.
"""
import functools

import numpy as np

import _aov_tex_twin as AT
import _cutout_twin as CT
import _interior_twin as IT
import _mfac_worlds as MW
import _nmap_twin as NT
import _nmap_worlds as NW
import _path_twin as PT
import _env_tree_twin as VT
import _env_worlds as EW
import _surface_worlds as SW
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
SEED = TW.SEED
W, H, SPP, DEPTH = 24, 16, 8, 8   # the interior room's size
ENV_TREE = 48
FORMS = dict(MW.FORMS)            # the eight shapes of the NMAP, MFAC and INTR families, plain and once more under mode 48
CAMERAS = TW.CAMERAS
ALL, NO_INTERIORS, NO_MICROFACETS = "all", "no interiors", "no microfacets"   # which tables a frame has: every one, the interior table taken away, the microfacet table too
TABLES = (ALL, NO_INTERIORS, NO_MICROFACETS)
BOX = ((7.3, 0.1, 2.3), (9.3, 2.0, 4.1))
COUNTERS = ("recorded_noise", "mapped_moving", "rule_after_medium", "medium_after_rough_transmission", "charged", "inside_ended_on_medium")
COUNTERS_48 = ("recorded_noise", "mapped_moving", "charged", "table_draws", "map_draws")   # under mode 48 there is no medium to draw for


CUT_COUNTERS = ("rejected_quad", "rejected_tri_uv", "rejected_tri_plain", "rejected_deep", "hole_then_moving", "hole_then_medium_draw", "hole_then_solid",
                "kept_image_masked", "kept_mapped_masked", "kept_smooth_masked", "mask_uv_is_shade_uv", "light_picks_at_masked_image")
AT_LEAST = 20   # every counter that can occur in a frame reaches this in it


def can_occur(name, mode48, kind, medium=None, as_list=False):
    """whether counter `name` of CUT_COUNTERS can occur in the masked room's frame of (mode48, camera kind): a medium draws in the plain room alone — and after a
    rejection only under a BVH: a list tests every sphere, the media among them, before its first parallelogram —, a sphere has moved under the motion camera
    alone, and the light half is picked under mode 48 alone"""
    medium = not mode48 if medium is None else medium
    return {"hole_then_medium_draw": medium and not as_list, "hole_then_moving": kind == "motion", "light_picks_at_masked_image": mode48}.get(name, True)


def leaf_picture():
    """the leaf's RGBA picture, in memory: (rgb [16][16][3], alpha [16][16]) — veins of opacity that fall off smoothly, so that the bilinear mask crosses its
    cutoff between texels, and a colour that varies with them.  The mask is made of the alpha as image_io.read_png_alpha's is: every channel the opacity."""
    y, x = np.mgrid[0:16, 0:16]
    a = 0.5 + 0.5 * np.cos(x * (2 * np.pi / 8)) * np.cos(y * (2 * np.pi / 8)) + 0.25 * np.cos((x + y) * (2 * np.pi / 16))
    alpha = np.clip(np.rint(255 * np.clip(a, 0, 1)), 0, 255).astype(np.uint8)
    rgb = np.stack([40 + 8 * y + 3 * x, 120 + 6 * x, 30 + 5 * ((x * y) % 16)], axis=2).astype(np.uint8)
    return np.ascontiguousarray(rgb), np.ascontiguousarray(alpha)


def mask_of(alpha):
    return np.ascontiguousarray(np.repeat(np.asarray(alpha, np.uint8)[:, :, None], 3, axis=2))


LEAF_V = np.array([(2.5, 3.6, 5.0), (5.3, 3.6, 5.0), (5.3, 6.4, 5.0), (2.5, 6.4, 5.0)], F)
LEAF_F = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
LEAF_UV = np.array([(0, 0), (2, 0), (2, 2), (0, 2)], F)
LEAF_BENT = np.array([(-0.5, -0.4, -1.0), (0.5, -0.4, -1.0), (0.5, 0.4, -1.0), (-0.5, 0.4, -1.0)], F)   # bent about the side that faces the camera


def masked_surfaces(s, p, leaf=True, leaf_mask="alpha", opaque=None):
    """what `masks` adds to the room, through whose holes a ray sees what the cutout room never had behind one.  leaf False: the room without the
    leaf (its material and images stay); leaf_mask: "alpha" or "black"; returns the names of the materials and images."""
    from ray_tracing_v06_amd import image_io as io
    rgb, alpha = leaf_picture()
    img = dict(leaf=s.add_image(rgb, "repeat", "bilinear"), leaf_mask=s.add_image(mask_of(alpha), "repeat", "bilinear"),
               lattice=s.add_image(io.lattice_mask(24, 24, 4, 4, 0.45), "clamp", "nearest"),
               wedge=s.add_image(mask_of([[0, 255, 60, 0], [255, 30, 255, 0], [40, 0, 255, 120]]), "clamp", "nearest"),
               white=s.add_image(mask_of([[255]]), "clamp", "nearest"), black=s.add_image(mask_of([[0]]), "clamp", "nearest"))
    leaf_mat = s.ImageTexture(img["leaf"])                                                  # the leaf: a card of two triangles in front of the moving conductor
    if leaf:
        s.MakeMesh(LEAF_V, LEAF_F, leaf_mat, uvs=LEAF_UV, normals=LEAF_BENT)
    s.set_normal_map(leaf_mat, 1, 1.0)
    s.MakeMovingSphere((4.1, 4.5, 6.0), (4.6, 5.3, 6.0), 0.6, s.Lambertian((0.8, 0.4, 0.5)))   # ... and of one more moving sphere, right behind it
    s.set_cutout(leaf_mat, img["black" if leaf_mask == "black" else "leaf_mask"], 0.5)
    grain = s.NoiseTexture(2.5, (0.6, 0.7, 0.5))                                            # a lattice-masked noise parallelogram under a coat, in front of the medium
    s.MakeQuad((4.9, 4.9, 3.4), (2.6, 0.0, 0.4), (0.5, 2.4, 0.0), grain)
    s.set_microfacet(grain, 0.35, 0.15)
    s.set_cutout(grain, img["lattice"], 0.5)
    steel = s.Metal((0.8, 0.75, 0.7), 0.2)                                                  # a plain triangle of rough conductor, its roughness mapped, in front of the box
    s.MakeTriangle((7.0, 0.05, 0.6), (7.0, 0.05, 6.2), (6.6, 5.0, 3.2), steel)
    s.set_microfacet(steel, 0.5).set_roughness_map(steel, 2)
    s.set_cutout(steel, img["wedge"], 0.3)
    tiles = s.LambertianTexture((0.8, 0.3, 0.2), (0.9, 0.9, 0.8), 2.0)                      # a masked checker parallelogram behind the frosted ball
    s.MakeQuad((0.2, 4.9, 7.9), (1.5, 0.0, 0.3), (0.0, 1.6, 0.0), tiles)
    s.set_cutout(tiles, img["lattice"], 0.5)
    return dict(images=img, leaf=leaf_mat, grain=grain, steel=steel, tiles=tiles)


def room(p, env=False, as_list=False, medium=True, masks=False, leaf=True, leaf_mask="alpha"):
    """env: the sky map for a background (mode 48's world) instead of the constant colour; medium False: the room without its three spheres of medium; masks: the
    masked surfaces of masked_surfaces() and an all-white mask on the metal tetrahedron — an opaque record among the live ones"""
    names = {}

    def more(s):
        io = TW.mesh_io()
        s.MakeMesh(*io.icosphere(1), s.Dielectric((1, 1, 1), 1.5), 1.3, 0.0, (5, 3.6, 7))
        bronze = s.Metal((0.7, 0.6, 0.5), 0.4)
        s.MakeMesh(*io.tetrahedron(), bronze, 1.3, 45.0, (8, 6, 7.5))
        s.set_perlin(SEED)
        s.MakeTriangle((0.05, 0.5, 4), (0.05, 0.5, 8), (0.05, 4.5, 6), s.NoiseTexture(2.0, (0.6, 0.6, 0.6)))
        assert s.add_image(NW.bumps(), "repeat", "bilinear") == 1 and s.add_image(MW.roughness_map(), "repeat", "bilinear") == 2
        marble, veined = s.NoiseTexture(3.0, (0.7, 0.6, 0.5)), s.NoiseTexture(1.5, (0.5, 0.7, 0.6))
        s.MakeQuad((0.05, 5.0, 1.0), (0, 0, 3.0), (0, 3.0, 0), marble)                       # a noise parallelogram under a coat
        s.set_microfacet(marble, 0.3, 0.2)
        s.MakeSphere((3.3, 0.8, 3.4), 0.8, veined)                                          # a noise sphere under a normal map
        s.set_normal_map(veined, 1, 1.0)
        blue, gold = s.Lambertian((0.2, 0.4, 0.8)), s.Metal((0.9, 0.7, 0.4), 0.3)
        s.MakeMovingSphere((2, 2, 7.5), (2, 2.9, 7.5), 0.8, blue)                           # the wide room's moving sphere, now under a normal map and a mapped coat
        s.set_normal_map(blue, 1, 1.5).set_microfacet(blue, 0.8, 0.2).set_roughness_map(blue, 2)
        s.MakeMovingSphere((3.0, 4.6, 8.6), (3.6, 5.1, 8.6), 0.75, gold)                    # a moving rough conductor
        s.set_microfacet(gold, 0.4)
        frosted, solid = s.Dielectric((0.95, 0.98, 1.0), 1.5), s.Dielectric((1, 1, 1), 1.5)
        s.MakeSphere((1.7, 5.6, 6.4), 1.0, frosted)                                         # a frosted ball ...
        s.set_rough_glass(frosted, 0.3)
        s.MakeBox(BOX[0], BOX[1], solid)                                                    # a solid tinted box ...
        s.set_interior(solid, color=(0.3, 0.8, 0.5), at=1.0)
        if medium:
            s.MakeSphere((6.5, 6.5, 6), 1.6, s.Isotropic((0.9, 0.9, 0.9), 0.4))
            s.MakeSphere((1.7, 5.6, 6.4), 0.7, s.Isotropic((0.9, 0.5, 0.3), 2.0))           # ... with a medium inside it
            s.MakeSphere((8.3, 1.9, 3.2), 0.8, s.Isotropic((0.4, 0.5, 0.9), 1.5))           # ... that a sphere of medium pokes through, by its top face
        if masks:
            names.update(masked_surfaces(s, p, leaf, leaf_mask), bronze=bronze)
            s.set_cutout(bronze, names["images"]["white"], 0.5)
        if env:
            s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
        else:
            s.set_background(TW.SKY)
    s = TW.tri_room(p, open_right=True, textured=True, as_list=as_list, more=more)
    s.names = names
    return s


def camera(p, kind, w=W, h=H):
    return TW.camera(p, w, h, kind)


SIGMA_ZERO, RECORDS_OFF = "every sigma zero", "records off"
VARIANTS = TABLES + (SIGMA_ZERO, RECORDS_OFF)
CUTOUTS_OFF, NO_CUTOUTS = "cutouts off", "no cutouts"   # the masked room's own: the cutout table present with every `on` zero, and taken away
CUT_VARIANTS = (ALL, CUTOUTS_OFF, NO_CUTOUTS, SIGMA_ZERO)


def tables_of(table, variant):
    """(normal maps, microfacets, interiors) of a scene as a frame of `variant` has them: one of TABLES, every sigma zero (the facing alone), or the three tables
    still present with every record off.  With a fourth table, the masked room's cutouts, that one too: as it is, every `on` zero under CUTOUTS_OFF, None under
    NO_CUTOUTS."""
    nmaps, mfacs, interiors = (a.copy() for a in table[:3])
    if variant == SIGMA_ZERO:
        interiors["sigma"] = 0.0
    elif variant == RECORDS_OFF:
        nmaps["on"], mfacs["on"], interiors["on"] = 0, 0, 0
    out = nmaps, (None if variant == NO_MICROFACETS else mfacs), (None if variant in (NO_INTERIORS, NO_MICROFACETS) else interiors)
    if len(table) == 3:
        return out
    cutouts = table[3].copy()
    if variant == CUTOUTS_OFF:
        cutouts["on"] = 0
    return out + (None if variant == NO_CUTOUTS else cutouts,)


class CountingRule:
    """a light rule that counts, beside what it does, the light-half picks at hits on a masked image material — the rays the cutout walk marked last"""

    def __init__(self, rule, marks, stats):
        self.rule, self.marks, self.stats, self.images = rule, marks, stats, rule.images

    def pick(self, tape, r, sampled, mt, hit_p, new_d, stats):
        out = self.rule.pick(tape, r, sampled, mt, hit_p, new_d, stats)
        rows, image = self.marks.get("masked_image", (None, None))
        if rows is not None:
            PT.bump(self.stats, "light_picks_at_masked_image", out[0] & np.isin(r, rows[image]))
        return out

    def density(self, *a):
        return self.rule.density(*a)


class Twin:
    """the room of one mode and memory layout and the extended twin's frames of it, cached per (tables, camera) — and per any other variation a test names.
    masks: the masked room, whose table has a fourth member, the cutouts, and whose walk is the composed one; room: further arguments of room()"""

    def __init__(self, mode48, as_list=False, medium=None, masks=False, **room_args):
        p = pkg()
        self.mode48, self.medium, self.masks = mode48, (not mode48 if medium is None else medium), masks
        self.scene = room(p, env=mode48, as_list=as_list, medium=self.medium, masks=masks, **room_args)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        self.vn, self.uv = self.scene.vertex_normals(), self.scene.texture_coords()
        self.table = (self.scene.normal_maps().copy(), self.scene.microfacets().copy(), self.scene.interiors().copy())
        if masks:
            self.table += (self.scene.cutouts().copy(),)
        self.textures = AT.twin_table(self.scene.textures())
        self.sky, self.light, self.tree = SW.lights_of(p, self.scene, self.world, mode48)
        self.cams = {kind: camera(p, kind) for kind in CAMERAS}
        self.eye = tuple(as_oracle_camera(self.cams["pinhole"]).o)
        self.frames = {}

    def marks(self, nmaps, interiors):
        """what the cutout walk counts under (_cutout_twin.closest_intersection): which materials are solid and mapped, which triangles are smooth"""
        n = len(self.table[0])
        vn = NT.ST.table(self.vn)
        return dict(solid=np.zeros(n, bool) if interiors is None else interiors["on"] != 0, mapped=np.zeros(n, bool) if nmaps is None else nmaps["on"] != 0,
                    smooth=(vn != 0).any(axis=(1, 2)))

    def samples(self, kind, table=None, spp=SPP, first_sample=0, stats=None, cam=None, trace_of=None, time0=False, wrong=None, plain_walk=False):
        """((H, W, spp, 3) samples, followed) under camera `kind` and the tables `table` (default: the scene's); cam: another camera in its place; trace_of:
        a function of the walk that gives the walk to use; time0: the motion camera's shutter closed at 0.  Under a cutout table the walk is the composed one:
        the rule in the leaf phase (_cutout_twin), then smooth normal and normal map at the hit the walk kept.  wrong: one of _cutout_twin's wrong walks;
        plain_walk: _nmap_twin.walk_of without `base`, whatever the cutout table says."""
        table = self.table if table is None else table
        nmaps, mfacs, interiors = table[:3]
        cutouts = table[3] if len(table) > 3 and not plain_walk else None
        marks, base = None, None
        if cutouts is not None:
            marks = self.marks(nmaps, interiors) if stats is not None else None
            base = CT.walk_of(self.uv, cutouts, self.textures, stats, self.eye, marks, wrong)
        trace, walk = NT.walk_of(self.vn, self.uv, nmaps, self.textures, base=base)
        trace = trace if trace_of is None else trace_of(trace)
        cam = as_oracle_camera(self.cams[kind] if cam is None else cam)
        if time0:
            cam.t1 = cam.t0 = 0.0
        rule = VT.MapRule(self.world, self.light, self.tree) if self.mode48 else None
        if stats is not None:
            PT.counters(stats, {"misses_by_bounce": np.zeros(DEPTH, np.int64), "charged": 0, **SW.GT.new_stats(), **VT.new_stats()})
            if cutouts is not None:
                PT.counters(stats, CT.new_stats())
                rule = CountingRule(rule, marks, stats) if rule is not None else None
        elif rule is not None:
            stats = PT.counters({}, VT.new_stats())
        return PT.frame_samples(lambda g, s: PT.radiance(self.world, cam, W, H, DEPTH, SEED, g, s, trace, sky=self.sky, rule=rule, tex=NT.tex_of(self.uv, self.textures),
                                                         mfacs=mfacs, walk=walk, glass=True, stats=stats, media=True, interiors=interiors), W, H, spp, first_sample)

    def frame(self, tables, kind):
        """the cached frame of (tables, kind), tables one of VARIANTS (and, of the masked room, CUT_VARIANTS): an object with samples, followed, sums, frame and
        stats"""
        key = (tables, kind)
        if key not in self.frames:
            f = Frame()
            f.stats = {}
            f.samples, f.followed = self.samples(kind, tables_of(self.table, tables), stats=f.stats)
            f.sums = IT.in_order_sums(f.samples)
            f.frame = IT.resolve(f.sums, SPP)
            for a in (f.samples, f.followed, f.sums, f.frame):
                a.setflags(write=False)
            self.frames[key] = f
        return self.frames[key]


class Frame:
    pass


NMAPS_ON, NMAPS_OFF = "normal maps", "no normal maps"


def feature_sums(tw, kind, nmaps=NMAPS_ON, fresh_rng=False, stats=None, cutouts=True):
    """the feature twin's sums (H, W, 8) of mode RT_AOV_FULL (_aov_full_twin.sums) of the room of `tw` under camera `kind`: the first trace of the colour path —
    the composed walk with the tape behind the camera's draws — its albedo, and the smooth and mapped normal (NMAPS_OFF: the smooth normal alone)"""
    import _aov_full_twin as AF
    import _noise_twin as NZ
    tab = NZ.tables(tw.world)
    uv = tw.uv if tw.uv is not None and len(tw.uv) else None
    return AF.sums(tw.world, as_oracle_camera(tw.cams[kind]), W, H, SPP, SEED, uv=uv, cutouts=tw.table[3] if tw.masks and cutouts else None, table=tw.textures,
                   noise=lambda albedo, scale, pts: NZ.value(tab, np.asarray(albedo, F), F(scale), pts), vn=tw.vn, nmaps=tw.table[0] if nmaps == NMAPS_ON else None,
                   fresh_rng=fresh_rng, stats=stats)


@functools.lru_cache(maxsize=None)
def features(as_list, kind, nmaps=NMAPS_ON):
    """feature_sums of the plain masked room, computed once per process and left unchanged"""
    out = feature_sums(run(False, as_list, None, True), kind, nmaps)
    out.setflags(write=False)
    return out


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update((a.view(np.uint32) if a.dtype == F else a).tobytes())
    return h.hexdigest()


def digest_lines():
    """one line per twin frame tests/test_gpu_live_cutouts.py compares a kernel with, as profiles/twin_digests_live_cutouts.txt keeps them: the sha256 of the
    samples' bits and `followed`, or of the feature sums' bits.  `python -c "import _live_worlds as LW; print(*LW.digest_lines(), sep='\\n')"` in tests/ prints them."""
    out = []
    for mode48 in (False, True):
        for as_list in (False, True):
            tw = run(mode48, as_list, None, True)
            for kind in CAMERAS:
                for variant in CUT_VARIANTS:
                    f = tw.frame(variant, kind)
                    out.append(f"{digest(f.samples, f.followed)}  live cutouts {'mode48' if mode48 else 'plain'} {'list' if as_list else 'bvh'} {kind} {variant}")
    for as_list in (False, True):
        for kind in CAMERAS:
            for nmaps in (NMAPS_ON, NMAPS_OFF):
                out.append(f"{digest(features(as_list, kind, nmaps))}  live cutouts features {'list' if as_list else 'bvh'} {kind} {nmaps}")
    return out


def random_masks(seed):
    """what _surface_worlds.random_surface_world(seed, live=True, before_build=...) takes to give its world cutout records: two to four random
    masks — lattices and random opacities of random sizes under random modes, as tools/fuzz_campaign.py --cutouts makes them — at random cutoffs on random
    materials of every kind that takes one, and on one image material the alpha of its own picture: a mask of the size and the modes of the image it names.
    The generator is its own: the world of the seed is the one the unmasked run has."""
    def add(s, mats, table):
        from ray_tracing_v06_amd import image_io as io
        rng = np.random.default_rng(SW.SEED_BASE + seed + (36 << 20))
        cutoff = lambda: float(rng.choice([0.0, 0.25, 0.5, 0.75, 1.0, rng.random()]))   # noqa: E731

        def image(mask, wrap, filt):
            assert s.add_image(mask, *SW.XW.MODE_NAMES[(wrap, filt)]) == len(table)
            table.append((mask, wrap, filt))
            return len(table) - 1
        maskable = mats["surface"] + [mats["noise"], mats["clear"]]
        chosen = []
        for _ in range(int(rng.integers(2, 5))):
            if rng.random() < 0.5:
                mask = io.lattice_mask(int(rng.integers(1, 33)), int(rng.integers(1, 33)), int(rng.integers(0, 6)), int(rng.integers(0, 6)), float(rng.random()))
            else:
                mask = np.repeat(rng.integers(0, 256, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 1)).astype(np.uint8), 3, axis=2)
            m = maskable[int(rng.integers(0, len(maskable)))]
            s.set_cutout(m, image(mask, int(rng.integers(0, 2)), int(rng.integers(0, 2))), cutoff())
            chosen.append(m)
        leaf = sorted(mats["image_of"])[int(rng.integers(0, len(mats["image_of"])))]
        picture, wrap, filt = table[mats["image_of"][leaf]]
        s.set_cutout(leaf, image(mask_of(rng.integers(0, 256, picture.shape[:2])), wrap, filt), cutoff())
        return {"materials": chosen + [leaf], "own_alpha": leaf}
    return add


def random_live_sums(p, seed, stats=None, masks=False):
    """_surface_worlds.random_surface_world(seed, live=True) and the extended twin's in-order sums of it, plain: (scene, camera, (w, h, spp, depth), sums (h, w, 4),
    followed (h, w, spp), recipe); masks: the world under random_masks(seed), and the twin's walk the composed one"""
    scene, table, cam, recipe = SW.random_surface_world(p, seed, live=True, before_build=random_masks(seed) if masks else None)
    w, h, spp, depth = recipe["frame"]
    world = as_oracle_world(scene.getWorldPtr())
    vn, uv = scene.vertex_normals(), scene.texture_coords()
    base = CT.walk_of(uv if uv is not None and len(uv) else None, scene.cutouts(), table, stats, tuple(recipe["eye"])) if masks else None
    trace, walk = NT.walk_of(vn, uv, scene.normal_maps(), table, base=base)
    sky = SW.lights_of(p, scene, world, False)[0]
    samples, followed = PT.frame_samples(lambda g, k: PT.radiance(world, as_oracle_camera(cam), w, h, depth, SEED, g, k, trace, sky=sky, tex=NT.tex_of(uv, table),
                                                                  mfacs=scene.microfacets(), walk=walk, glass=True, stats=stats, media=True,
                                                                  interiors=scene.interiors()), w, h, spp)
    return scene, cam, (w, h, spp, depth), IT.in_order_sums(samples), followed, recipe


@functools.lru_cache(maxsize=None)
def run(mode48, as_list=False, medium=None, masks=False):
    return Twin(mode48, as_list, medium, masks)
