"""The worlds of the triangle tests and the twin's runs of them — test infrastructure only.

Every world is built through the product's host vocabulary, which needs no device, and holds only what tests/_tri_twin.py follows (pinhole camera;
Lambertian, checker, metal and diffuse-light materials), so a test asserts `followed.all()` and leaves no pixel out.  run(...) is computed once per
process and never modified.
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

# The suite's statement of which TRI instantiations of render_kernel_stream exist: one (world, exact, ext, big, wide) key per RT_KERNEL_TRI(...) line of
# csrc/rt_device.hip — and, the same sixteen keys once more, per RT_KERNEL_TRI_NEE(...) line —, each with the recipe (kernel variant, environment) that makes a
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


def tri_room(p, as_list=False, traversal=0, lamp=False, tri_light=False, wall_as_triangles=False, plain=False, textured=False):
    """a closed 10 x 10 x 10 room of quads with one quad light, holding a tetrahedron, an icosphere(1) (80 triangles) of metal and a checker triangle;
    lamp: plus a sphere light; tri_light: plus a triangle with a light material (it emits, no table lists it); wall_as_triangles: the back wall as
    its two triangles; plain: the room without any triangle (the pins' world); textured: plus an image-textured triangle on the back wall and its image
    (an EXT = 2 world; the twin does not follow the samples that meet it)"""
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
    if as_list:
        s.MakeHittableList()
    else:
        s.set_traversal(traversal)
        s.BuildBVH_SAH()
    return s


def camera(p, w=W, h=H):
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
