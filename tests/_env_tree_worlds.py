"""The worlds and kernel forms of the tests of the map and the light tree together (mode 48) — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device, and holds no dielectric, noise or medium material: the twin
(tests/_env_tree_twin.py) follows every sample, image-textured hits included.  run(...) is computed once per process and never modified.
"""
import functools

import numpy as np

import _env_light_worlds as LW
import _env_tree_twin as VT
import _env_twin as ET
import _env_worlds as EW
import _tex_twin as XT
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, pkg

F = np.float32
SEED = EW.SEED
W, H, SPP, DEPTH = EW.W, EW.H, EW.SPP, EW.DEPTH   # 24 x 16 at 8 spp and depth 6
ENV_TREE = 48                                     # RT_LIGHT_SAMPLING_ENV_TREE

# The suite's statement of which LTREE && ENVL instantiations of render_kernel_stream exist: one (world, exact, ext, big, wide) key per form of the ENV_TREE family
# of csrc/rt_device.hip, each with _tri_worlds' recipe (kernel variant, environment) that makes a renderer of a background-2 world resolve to it.
# tests/test_env_tree_cpu.py holds the list against the source; tests/test_gpu_env_tree.py renders every key and compares it with the twin.
FORMS = {f: TW.FORMS[f] for f in [(TW.BVH, 0, 2, 0, 0), (TW.BVH, 1, 2, 0, 0), (TW.BVH, 0, 2, 1, 0), (TW.BVH, 1, 2, 1, 0), (TW.BVH, 0, 2, 1, 1), (TW.BVH, 1, 2, 1, 1),
                                  (TW.LIST, 1, 2, 0, 0), (TW.LIST, 1, 2, 1, 1)]}


def image(width, height, seed):
    return np.random.default_rng(7000 + 100 * width + height + seed).integers(0, 256, (height, width, 3)).astype(np.uint8)


IMAGES = [(image(5, 3, 1), XT.CLAMP, XT.NEAREST), (image(8, 4, 2), XT.REPEAT, XT.BILINEAR)]   # the two-image table of every textured world, as the twin takes it


def modest_map(width=16, height=8):
    """every texel positive, a dynamic range of 8: the map of the density pin, under which 1 / pm has a finite variance"""
    rng = np.random.default_rng(48)
    env = (0.25 + 1.75 * rng.random((height, width, 3))).astype(F)
    env.setflags(write=False)
    return env


def triangle_lamp(s):
    s.MakeTriangle((3.5, 6, 4), (6.5, 6.2, 4.5), (5, 5.8, 7), s.DiffuseLight((14, 12, 9)))


def quad_and_sphere(s):
    s.MakeQuad((3.5, 6, 3.5), (3, 0, 0), (0, 0, 3), s.DiffuseLight((8, 8, 8)))
    s.MakeSphere((1.5, 4.5, 7), 0.6, s.DiffuseLight((20, 14, 6)))


def three_kinds(s):
    quad_and_sphere(s)
    s.MakeTriangle((8.5, 3, 5), (8.5, 5, 6), (8.6, 3.5, 8), s.DiffuseLight((4, 8, 12)))


def sixty_five(s):
    """a sphere lamp and a panel of 64 small triangles above the room: more than the 64 lights mode 4 takes"""
    s.MakeSphere((1.5, 4.5, 7), 0.6, s.DiffuseLight((20, 14, 6)))
    emit = s.DiffuseLight((10, 10, 10))
    for c in range(32):
        x = 3 + c * 0.125
        s.MakeTriangle((x, 6, 4), (x + 0.125, 6, 4), (x, 6, 6), emit)
        s.MakeTriangle((x + 0.125, 6, 6), (x, 6, 6), (x + 0.125, 6, 4), emit)


LIGHTS = {0: None, 1: triangle_lamp, 2: quad_and_sphere, 3: three_kinds, 65: sixty_five}


def sky_lamp_room(p, n_l=3, as_list=False, textured=True, env=None, rotate_y=EW.SKY_U0_DEGREES, builder="BuildBVH_SAH"):
    """a checker floor, a Lambertian and a metal sphere under sky_environment(32, 16) at u0 = 0.3, lit as well by LIGHTS[n_l] — 3: a quad light, a sphere lamp and
    a triangle light — and, textured: an image-textured tetrahedron with per-vertex coordinates beyond [0, 1] on image 1 (repeat / bilinear) and an image-textured
    parallelogram on image 0 (clamp / nearest).  Without textures the small mesh is a Lambertian one, so every world is a TRI world of EXT 2."""
    s = p.Scene()
    s.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.5))
    s.MakeSphere((2.2, 1.0, 5.5), 1.0, s.Lambertian((0.7, 0.3, 0.3)))
    s.MakeSphere((8, 1.2, 6), 1.2, s.Metal((0.9, 0.7, 0.4), 0.3))
    m = TW.mesh_io()
    v, f = m.tetrahedron()
    if textured:
        s.set_image(IMAGES[0][0])
        one = s.add_image(IMAGES[1][0], "repeat", "bilinear")
        assert one == 1
        uvs = (np.random.default_rng(4).random((len(v), 2)) * 2.5 - 0.75).astype(F)
        s.MakeMesh(v, f, s.ImageTexture(1), 1.6, 20.0, (5, 1.4, 6.5), uvs=uvs)
        s.MakeQuad((3.0, 0.0, 9.0), (4.0, 0, 0.5), (0, 3.0, 0), s.ImageTexture(0))
    else:
        s.MakeMesh(v, f, s.Lambertian((0.3, 0.4, 0.8)), 1.6, 20.0, (5, 1.4, 6.5))
    if LIGHTS[n_l] is not None:
        LIGHTS[n_l](s)
    s.set_environment(EW.sky_map() if env is None else env, rotate_y=rotate_y)
    if as_list:
        s.MakeHittableList()
    else:
        getattr(s, builder)()
    return s


def window_room(p, image_floor=True):
    """the expectation's room: _tri_worlds' closed room with a window — the right wall is missing — onto the sky, its quad light, a sphere lamp and an
    image-textured parallelogram (image_floor: lying just above the floor, where most paths land)"""
    def more(s):
        s.set_image(IMAGES[0][0])
        one = s.add_image(IMAGES[1][0], "repeat", "bilinear")
        s.MakeQuad((1.0, 0.02, 2.0), (8.0, 0, 0), (0, 0, 7.0), s.ImageTexture(one if image_floor else 0))
        s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    return TW.tri_room(p, open_right=True, lamp=True, plain=True, more=more)


def far_lamp_hall(p):
    """_nee2_worlds' hall of the Cornell box's size under the sky, lit by one sphere of radius 0.05 under where its ceiling would be: D / r is about 10^4, so
    a few of the frame's 569 drawn points come out with disc <= 0 and the walk does not credit them (radius 2, the hall's own, loses none in so small a frame)"""
    s = p.Scene()
    white = s.Lambertian((0.73, 0.73, 0.73))
    s.MakeQuad((0, 0, 0), (555, 0, 0), (0, 0, 555), s.LambertianTexture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 40.0))
    s.MakeQuad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)
    s.MakeQuad((0, 0, 0), (0, 555, 0), (0, 0, 555), s.Lambertian((0.65, 0.05, 0.05)))
    s.MakeSphere((278, 520, 278), 0.05, s.DiffuseLight((9000, 8000, 6000)))
    s.MakeSphere((380, 60, 300), 60.0, white)
    s.set_environment(EW.sky_map(), rotate_y=EW.SKY_U0_DEGREES)
    s.BuildBVH_TopDown()
    return s


HALL_VIEW = ((278, 278, -500), (278, 200, 278), 50.0)


def camera(p, name="room", w=W, h=H):
    if name == "hall":
        return p.PinholeCamera(HALL_VIEW[0], HALL_VIEW[1], (0, 1, 0), HALL_VIEW[2], w / h)
    return EW.camera(p, w, h)


def tex_of(scene):
    """what the twin needs to follow material 7: (the scene's table of texture coordinates or None, the two-image table), or None for a world without images"""
    if scene.textures() is None:
        return None
    uv = scene.texture_coords()
    return (uv if len(uv) else None, IMAGES)


class Run:
    """a world under a map, and the whole-sample twin's samples of it in mode 48"""

    def __init__(self, scene, view="room", w=W, h=H, spp=SPP, depth=DEPTH, first_sample=0):
        p = pkg()
        self.scene, self.view = scene, view
        env, u0 = scene.environment()
        self.env, self.u0 = env, u0
        self.tables = p.api.environment_distribution(env)
        self.world = as_oracle_world(scene.getWorldPtr())
        self.tree = VT.table_of(self.world)
        self.tex = tex_of(scene)
        self.stats = {}
        samples, followed = VT.frame_samples(self.world, as_oracle_camera(camera(p, view, w, h)), w, h, spp, depth, SEED, ET.sky_environment(env, u0),
                                             light=(self.tables, u0), tree=self.tree, tex=self.tex, first_sample=first_sample, stats=self.stats)
        self.samples, self.followed = samples, followed
        self.sums = VT.in_order_sums(samples)
        self.frame = VT.resolve(self.sums, spp)
        for a in (self.samples, self.followed, self.sums, self.frame):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def run(name, as_list=False):
    p = pkg()
    if name == "forms":
        return Run(sky_lamp_room(p, as_list=as_list))
    if name.startswith("n_l="):
        return Run(sky_lamp_room(p, n_l=int(name[4:])))
    if name == "triangle_lamp":   # the world of the test that fails without the mode: no image, one triangle light, which mode 32 leaves to be hit
        return Run(sky_lamp_room(p, n_l=1, textured=False))
    if name == "sun":
        return Run(sky_lamp_room(p, env=LW.sun_map(), rotate_y=0.0))
    if name == "replaced":   # the forms' world after its map was replaced by the sun
        return Run(sky_lamp_room(p, env=LW.sun_map()))
    if name == "silhouette":
        return Run(far_lamp_hall(p), view="hall")
    raise KeyError(name)
