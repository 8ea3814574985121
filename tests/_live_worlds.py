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


def room(p, env=False, as_list=False, medium=True):
    """env: the sky map for a background (mode 48's world) instead of the constant colour; medium False: the room without its three spheres of medium"""
    def more(s):
        io = TW.mesh_io()
        s.MakeMesh(*io.icosphere(1), s.Dielectric((1, 1, 1), 1.5), 1.3, 0.0, (5, 3.6, 7))
        s.MakeMesh(*io.tetrahedron(), s.Metal((0.7, 0.6, 0.5), 0.4), 1.3, 45.0, (8, 6, 7.5))
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
        if env:
            s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
        else:
            s.set_background(TW.SKY)
    return TW.tri_room(p, open_right=True, textured=True, as_list=as_list, more=more)


def camera(p, kind, w=W, h=H):
    return TW.camera(p, w, h, kind)


SIGMA_ZERO, RECORDS_OFF = "every sigma zero", "records off"
VARIANTS = TABLES + (SIGMA_ZERO, RECORDS_OFF)


def tables_of(table, variant):
    """(normal maps, microfacets, interiors) of a scene as a frame of `variant` has them: one of TABLES, every sigma zero (the facing alone), or the three tables
    still present with every record off"""
    nmaps, mfacs, interiors = (a.copy() for a in table)
    if variant == SIGMA_ZERO:
        interiors["sigma"] = 0.0
    elif variant == RECORDS_OFF:
        nmaps["on"], mfacs["on"], interiors["on"] = 0, 0, 0
    return nmaps, (None if variant == NO_MICROFACETS else mfacs), (None if variant in (NO_INTERIORS, NO_MICROFACETS) else interiors)


class Twin:
    """the room of one mode and memory layout and the extended twin's frames of it, cached per (tables, camera) — and per any other variation a test names"""

    def __init__(self, mode48, as_list=False, medium=None):
        p = pkg()
        self.mode48, self.medium = mode48, (not mode48 if medium is None else medium)
        self.scene = room(p, env=mode48, as_list=as_list, medium=self.medium)
        self.world = as_oracle_world(self.scene.getWorldPtr())
        self.vn, self.uv = self.scene.vertex_normals(), self.scene.texture_coords()
        self.table = (self.scene.normal_maps().copy(), self.scene.microfacets().copy(), self.scene.interiors().copy())
        self.textures = AT.twin_table(self.scene.textures())
        self.sky, self.light, self.tree = SW.lights_of(p, self.scene, self.world, mode48)
        self.cams = {kind: camera(p, kind) for kind in CAMERAS}
        self.frames = {}

    def samples(self, kind, table=None, spp=SPP, first_sample=0, stats=None, cam=None, trace_of=None, time0=False):
        """((H, W, spp, 3) samples, followed) under camera `kind` and the three tables `table` (default: the scene's); cam: another camera in its place; trace_of:
        a function of the walk that gives the walk to use; time0: the motion camera's shutter closed at 0"""
        nmaps, mfacs, interiors = self.table if table is None else table
        trace, walk = NT.walk_of(self.vn, self.uv, nmaps, self.textures)
        trace = trace if trace_of is None else trace_of(trace)
        cam = as_oracle_camera(self.cams[kind] if cam is None else cam)
        if time0:
            cam.t1 = cam.t0 = 0.0
        rule = VT.MapRule(self.world, self.light, self.tree) if self.mode48 else None
        if stats is not None:
            PT.counters(stats, {"misses_by_bounce": np.zeros(DEPTH, np.int64), "charged": 0, **SW.GT.new_stats(), **VT.new_stats()})
        elif rule is not None:
            stats = PT.counters({}, VT.new_stats())
        return PT.frame_samples(lambda g, s: PT.radiance(self.world, cam, W, H, DEPTH, SEED, g, s, trace, sky=self.sky, rule=rule, tex=NT.tex_of(self.uv, self.textures),
                                                         mfacs=mfacs, walk=walk, glass=True, stats=stats, media=True, interiors=interiors), W, H, spp, first_sample)

    def frame(self, tables, kind):
        """the cached frame of (tables, kind), tables one of VARIANTS: an object with samples, followed, sums, frame and stats"""
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


def random_live_sums(p, seed, stats=None):
    """_surface_worlds.random_surface_world(seed, live=True) and the extended twin's in-order sums of it, plain: (scene, camera, (w, h, spp, depth), sums (h, w, 4),
    followed (h, w, spp), recipe)"""
    scene, table, cam, recipe = SW.random_surface_world(p, seed, live=True)
    w, h, spp, depth = recipe["frame"]
    world = as_oracle_world(scene.getWorldPtr())
    vn, uv = scene.vertex_normals(), scene.texture_coords()
    trace, walk = NT.walk_of(vn, uv, scene.normal_maps(), table)
    sky = SW.lights_of(p, scene, world, False)[0]
    samples, followed = PT.frame_samples(lambda g, k: PT.radiance(world, as_oracle_camera(cam), w, h, depth, SEED, g, k, trace, sky=sky, tex=NT.tex_of(uv, table),
                                                                  mfacs=scene.microfacets(), walk=walk, glass=True, stats=stats, media=True,
                                                                  interiors=scene.interiors()), w, h, spp)
    return scene, cam, (w, h, spp, depth), IT.in_order_sums(samples), followed, recipe


@functools.lru_cache(maxsize=None)
def run(mode48, as_list=False, medium=None):
    return Twin(mode48, as_list, medium)
