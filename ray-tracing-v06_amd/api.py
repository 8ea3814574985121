"""Python view of the reference-shaped host API, over the C ABI (used by tests/ and bench.py).

Names follow the reference: Sphere / MovingSphere, material descriptors, SphereHandle-style adders,
BVH_Handle.Factory builders, the three cameras, and Renderer.MakeRenderer / Render /
DownloadRenderbuffer (main/src/Renderer.h:38-46).  The C++ twin of this file is include/rt06/*.hpp.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import Camera, RenderConfig, WorldFlat, check, lib, v3


def PinholeCamera(lookfrom, lookat, up, vfov, aspect_ratio):
    """PinholeCamera ctor, rt_engine/shaders/cu_Cameras.cuh:16-25."""
    c = Camera()
    check(lib().rt_camera_pinhole(v3(lookfrom), v3(lookat), v3(up), vfov, aspect_ratio, C.byref(c)))
    return c


def DefocusBlurCamera(lookfrom, lookat, up, vfov, aspect_ratio, aperture, focus_dist):
    """DefocusBlurCamera ctor, cu_Cameras.cuh:40-52."""
    c = Camera()
    check(lib().rt_camera_defocus(v3(lookfrom), v3(lookat), v3(up), vfov, aspect_ratio, aperture, focus_dist, C.byref(c)))
    return c


def MotionBlurCamera(lookfrom, lookat, up, vfov, aspect_ratio, time0, time1):
    """MotionBlurCamera ctor, cu_Cameras.cuh:73-85."""
    c = Camera()
    check(lib().rt_camera_motion(v3(lookfrom), v3(lookat), v3(up), vfov, aspect_ratio, time0, time1, C.byref(c)))
    return c


# The lens cameras (rt06.h): a projection with an optional thin lens (aperture > 0) and an optional shutter (time0 != time1) on one record.
# Rendered by the streaming variants; the baseline kernel (variant 1) refuses them.
def _lens_camera(ctor, lookfrom, lookat, up, p0, p1, aperture, focus_dist, time0, time1):
    c = Camera()
    check(ctor(v3(lookfrom), v3(lookat), v3(up), p0, p1, aperture, focus_dist, time0, time1, C.byref(c)))
    return c


def PerspectiveCamera(lookfrom, lookat, up, vfov, aspect_ratio, aperture=0.0, focus_dist=1.0, time0=0.0, time1=0.0):
    """rt_camera_perspective: DefocusBlurCamera's basis and viewport, with a shutter."""
    return _lens_camera(lib().rt_camera_perspective, lookfrom, lookat, up, vfov, aspect_ratio, aperture, focus_dist, time0, time1)


def OrthographicCamera(lookfrom, lookat, up, height, aspect_ratio, aperture=0.0, focus_dist=1.0, time0=0.0, time1=0.0):
    """rt_camera_orthographic: parallel rays along lookat - lookfrom through a window `height` world units tall."""
    return _lens_camera(lib().rt_camera_orthographic, lookfrom, lookat, up, height, aspect_ratio, aperture, focus_dist, time0, time1)


def FisheyeCamera(lookfrom, lookat, up, fov, aspect_ratio, aperture=0.0, focus_dist=1.0, time0=0.0, time1=0.0):
    """rt_camera_fisheye: equidistant, `fov` degrees across the image's height; no circular mask."""
    return _lens_camera(lib().rt_camera_fisheye, lookfrom, lookat, up, fov, aspect_ratio, aperture, focus_dist, time0, time1)


def PanoramaCamera(lookfrom, lookat, up, hspan_degrees=360.0, vspan_degrees=180.0, aperture=0.0, focus_dist=1.0, time0=0.0, time1=0.0):
    """rt_camera_panorama: equirectangular; the full sphere by default, oriented like an unrotated environment map when looking along +x with +y up."""
    return _lens_camera(lib().rt_camera_panorama, lookfrom, lookat, up, hspan_degrees, vspan_degrees, aperture, focus_dist, time0, time1)


class Scene:
    """Host scene: what SphereHandle / newOnDevice<Material> / BVH_Handle::Factory / HittableList /
    bvh_node build in the reference, kept as flat arrays."""

    def __init__(self, handle=None):
        if handle is None:
            h = C.c_void_p()
            check(lib().rt_scene_create(C.byref(h)))
            handle = h
        self.h = handle

    # --- prefab scenes (SceneBook2BVH::Factory::MakeScene and friends) ---
    @classmethod
    def book1_final(cls, seed=1984):
        h = C.c_void_p()
        check(lib().rt_scene_book1_final(seed, C.byref(h)))
        return cls(h)

    @classmethod
    def book2_moving(cls, seed=1984):
        h = C.c_void_p()
        check(lib().rt_scene_book2_moving(seed, C.byref(h)))
        return cls(h)

    @classmethod
    def three_spheres(cls):
        h = C.c_void_p()
        check(lib().rt_scene_three_spheres(C.byref(h)))
        return cls(h)

    @classmethod
    def cornell_box(cls):
        """BASELINE.json configs[3] (not in the reference): 18 quads, one light, black background."""
        h = C.c_void_p()
        check(lib().rt_scene_cornell_box(C.byref(h)))
        return cls(h)

    @classmethod
    def cornell_lamp(cls):
        """The Cornell box lit by a lamp (not in the reference): no ceiling quad light, a sphere light of radius 40 at (278, 470, 278)."""
        h = C.c_void_p()
        check(lib().rt_scene_cornell_lamp(C.byref(h)))
        return cls(h)

    @classmethod
    def book2_final(cls, seed=1984):
        """BASELINE.json configs[4] (not in the reference): final_scene() of "The Next Week"."""
        h = C.c_void_p()
        check(lib().rt_scene_book2_final(seed, C.byref(h)))
        return cls(h)

    # --- vocabulary ---
    def add_material(self, mtype, albedo, param=0.0, albedo2=None):
        out = C.c_int32()
        a2 = v3(albedo2) if albedo2 is not None else None
        check(lib().rt_scene_add_material(self.h, mtype, v3(albedo), param, a2, C.byref(out)))
        return out.value

    def Lambertian(self, albedo):
        return self.add_material(capi.MAT_LAMBERTIAN, albedo)

    def Metal(self, albedo, fuzz):
        return self.add_material(capi.MAT_METAL, albedo, fuzz)

    def Dielectric(self, albedo, ior):
        return self.add_material(capi.MAT_DIELECTRIC, albedo, ior)

    def LambertianTexture(self, c1, c2, scale):
        return self.add_material(capi.MAT_LAMBERTIAN_CHECKER, c1, np.float32(1.0) / np.float32(scale), c2)

    def DiffuseLight(self, emit):
        """diffuse_light of "The Next Week" (extension, not in the reference)."""
        return self.add_material(capi.MAT_DIFFUSE_LIGHT, emit)

    def Isotropic(self, albedo, density):
        """isotropic phase function of "The Next Week" (extension): a sphere made of it is a constant_medium of that density."""
        return self.add_material(capi.MAT_ISOTROPIC, albedo, density)

    def MakeConstantMedium(self, center, radius, density, albedo):
        """constant_medium(sphere(center, radius), density, albedo) of "The Next Week" (extension, not in the reference)."""
        return self.MakeSphere(center, radius, self.Isotropic(albedo, density))

    def set_perlin(self, seed=1984):
        """perlin::perlin() of "The Next Week" (extension): the world's noise tables."""
        check(lib().rt_scene_set_perlin(self.h, seed))
        return self

    def NoiseTexture(self, scale, albedo=(0.5, 0.5, 0.5)):
        """lambertian(noise_texture(scale)) of "The Next Week" (extension); needs set_perlin()."""
        return self.add_material(capi.MAT_LAMBERTIAN_NOISE, albedo, scale)

    def set_image(self, rgb):
        """The image of image_texture (extension): uint8 array [H][W][3], row 0 = top."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        check(lib().rt_scene_set_image(self.h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data))
        return self

    def ImageTexture(self, image=0):
        """lambertian(image_texture) of "The Next Week" (extension) on spheres (u, v from the normal), quads (u, v = the planar coordinates of the hit) and triangles
        (DESIGN.md §22).  image: which image of the scene — 0 = the one of set_image(), 1, 2, ... = what add_image() returned."""
        return self.add_material(capi.MAT_LAMBERTIAN_IMAGE, (1, 1, 1), 0.0, (float(image), 0.0, 0.0))   # the index rides in rt_material.albedo2[0]

    def add_image(self, rgb, wrap="clamp", filter="nearest"):
        """One more image (extension): uint8 array [H][W][3], row 0 = top, under a wrap mode ("clamp" / "repeat") and a filter ("nearest" /
        "bilinear").  Returns its index (1, 2, ...) for ImageTexture(image=...); Renderer / MultiRenderer push the table at creation."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("add_image: the image must have shape (H, W, 3)")
        out = C.c_uint32()
        check(lib().rt_scene_add_image(self.h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data, wrap_mode(wrap), filter_mode(filter), C.byref(out)))
        return out.value

    def image_sampling(self, index, wrap="clamp", filter="nearest"):
        """The wrap mode and the filter of image `index` of the scene, 0 (the image of set_image()) included (rt_scene_image_sampling)."""
        check(lib().rt_scene_image_sampling(self.h, index, wrap_mode(wrap), filter_mode(filter)))
        return self

    def textures(self):
        """The scene's texture table (rt_scene_textures) as (records, texels): a structured array of capi.TEXTURE_DT, entry 0 = the image of set_image() (0 x 0 when
        there is none), and all texels (n, 3) uint8, the images back to back; None for a scene without any image and with default modes."""
        rec, n, tex = C.c_void_p(), C.c_uint32(), C.c_void_p()
        check(lib().rt_scene_textures(self.h, C.byref(rec), C.byref(n), C.byref(tex)))
        if n.value == 0:
            return None
        records = self._arr(rec.value, n.value, capi.TEXTURE_DT)
        total = int((records["width"].astype(np.int64) * records["height"]).sum())
        return records, self._arr(tex.value, total * 3, np.dtype(np.uint8)).reshape(-1, 3)

    def set_normal_map(self, material, image, strength=1.0):
        """Attaches image `image` of the scene (set_image() = 0, add_image() = 1, 2, ...) to `material` as its tangent-space normal map (extension; DESIGN.md §28;
        rt_scene_set_normal_map): OpenGL convention, green = +v.  Lambertian (plain, checker, noise, image) and metal materials take one."""
        check(lib().rt_scene_set_normal_map(self.h, material, image, float(strength)))
        return self

    def clear_normal_map(self, material):
        check(lib().rt_scene_clear_normal_map(self.h, material))
        return self

    def normal_maps(self):
        """The scene's normal-map table (rt_scene_normal_maps): one record of capi.NORMAL_MAP_DT per material, or None while no material has a map."""
        rec, n = C.c_void_p(), C.c_uint32()
        check(lib().rt_scene_normal_maps(self.h, C.byref(rec), C.byref(n)))
        return None if n.value == 0 else self._arr(rec.value, n.value, capi.NORMAL_MAP_DT)

    def set_microfacet(self, material, roughness, specular=0.04):
        """Gives `material` a microfacet record (extension; rt_scene_set_microfacet): a metal becomes a rough GGX conductor with F0 = its albedo
        (its fuzz is no longer read, `specular` is ignored); a Lambertian (plain, checker, noise, image) material gets a glossy coat of F0 = specular over it."""
        check(lib().rt_scene_set_microfacet(self.h, material, float(roughness), float(specular)))
        return self

    def set_roughness_map(self, material, image):
        """The green channel of image `image` of the scene scales the roughness of `material`'s record (rt_scene_set_roughness_map; set_microfacet or, on glass, set_rough_glass first)."""
        check(lib().rt_scene_set_roughness_map(self.h, material, image))
        return self

    def set_rough_glass(self, material, roughness):
        """Gives `material`, a Dielectric, a rough-glass record (extension; rt_scene_set_rough_glass): it reflects and refracts about GGX
        micro-normals of that roughness.  set_roughness_map then scales the roughness by an image's green channel; clear_microfacet makes it clear glass again."""
        check(lib().rt_scene_set_rough_glass(self.h, material, float(roughness)))
        return self

    def clear_microfacet(self, material):
        check(lib().rt_scene_clear_microfacet(self.h, material))
        return self

    def microfacets(self):
        """The scene's microfacet table (rt_scene_microfacets): one record of capi.MICROFACET_DT per material, or None while no material has a record."""
        rec, n = C.c_void_p(), C.c_uint32()
        check(lib().rt_scene_microfacets(self.h, C.byref(rec), C.byref(n)))
        return None if n.value == 0 else self._arr(rec.value, n.value, capi.MICROFACET_DT)

    def set_interior(self, material, sigma=None, color=None, at=None):
        """Makes `material`, a Dielectric, solid glass (extension; rt_scene_set_interior): its parallelograms, triangles and meshes know inside from
        outside by their winding, and a segment that ends inside it is absorbed by exp(-sigma distance) per channel.  sigma: the absorption coefficient per unit
        length (one number or three; default 0: facing alone) — or color and at: the tint white light has after `at` units of glass, sigma = -ln(color) / at,
        computed in double."""
        if (color is None) != (at is None) or (sigma is not None and color is not None):
            raise ValueError("set_interior: give sigma, or color and at together")
        if color is not None:
            c = np.broadcast_to(np.asarray(color, np.float64), (3,))
            if not (np.all(c > 0.0) and np.all(c <= 1.0) and float(at) > 0.0):
                raise ValueError("set_interior: a color lies in (0, 1] per channel and `at` is a positive distance")
            sigma = -np.log(c) / float(at) + 0.0
        s3 = np.broadcast_to(np.asarray(0.0 if sigma is None else sigma, np.float64), (3,))
        check(lib().rt_scene_set_interior(self.h, material, (C.c_float * 3)(*[float(x) for x in s3])))
        return self

    def clear_interior(self, material):
        check(lib().rt_scene_clear_interior(self.h, material))
        return self

    def interiors(self):
        """The scene's interior table (rt_scene_interiors): one record of capi.INTERIOR_DT per material, or None while no material has a record."""
        rec, n = C.c_void_p(), C.c_uint32()
        check(lib().rt_scene_interiors(self.h, C.byref(rec), C.byref(n)))
        return None if n.value == 0 else self._arr(rec.value, n.value, capi.INTERIOR_DT)

    def set_cutout(self, material, image, cutoff=0.5):
        """Makes image `image` of the scene (set_image() = 0, add_image() = 1, 2, ...) the opacity mask of `material` (extension; DESIGN.md §34;
        rt_scene_set_cutout): a parallelogram or triangle of that material is there only where the mask's green channel is not below `cutoff`, and a ray goes
        through it elsewhere.  Spheres ignore the record; lights, media and materials with an interior record take none."""
        check(lib().rt_scene_set_cutout(self.h, material, image, float(cutoff)))
        return self

    def clear_cutout(self, material):
        check(lib().rt_scene_clear_cutout(self.h, material))
        return self

    def cutouts(self):
        """The scene's cutout table (rt_scene_cutouts): one record of capi.CUTOUT_DT per material, or None while no material has a record."""
        rec, n = C.c_void_p(), C.c_uint32()
        check(lib().rt_scene_cutouts(self.h, C.byref(rec), C.byref(n)))
        return None if n.value == 0 else self._arr(rec.value, n.value, capi.CUTOUT_DT)

    def MakeBox(self, a, b, mat, rotate_y=0.0, translate=(0, 0, 0)):
        """box(a, b, mat) of "The Next Week" as 6 quads, optionally rotate_y(degrees) then translate; returns the first quad index."""
        out = C.c_int32()
        check(lib().rt_scene_add_box(self.h, v3(a), v3(b), mat, rotate_y, v3(translate), C.byref(out)))
        return out.value

    def MakeQuad(self, Q, u, v, mat):
        """quad(Q,u,v,mat) of "The Next Week" (extension, not in the reference)."""
        out = C.c_int32()
        check(lib().rt_scene_add_quad(self.h, v3(Q), v3(u), v3(v), mat, C.byref(out)))
        return out.value

    def MakeTriangle(self, a, b, c, mat, normals=None, uvs=None):
        """tri of "The Next Week" from its three vertices (extension, not in the reference): a quad of kind 1; returns its quad index.
        normals: one normal per vertex, (3, 3), for smooth shading (rt_scene_add_triangle_smooth).
        uvs: one texture coordinate per vertex, (3, 2), for an image-textured material (rt_scene_add_triangle_uv)."""
        out = C.c_int32()
        if uvs is not None:
            ta, tb, tc = (capi.vec2(*t) for t in np.asarray(uvs, dtype=np.float32).reshape(3, 2))
            if normals is None:
                na = nb = nc = None
            else:
                na, nb, nc = (v3(n) for n in np.asarray(normals, dtype=np.float32).reshape(3, 3))
            check(lib().rt_scene_add_triangle_uv(self.h, v3(a), v3(b), v3(c), na, nb, nc, ta, tb, tc, mat, C.byref(out)))
            self._uv = True
            self._smooth = getattr(self, "_smooth", False) or normals is not None
        elif normals is None:
            check(lib().rt_scene_add_triangle(self.h, v3(a), v3(b), v3(c), mat, C.byref(out)))
        else:
            na, nb, nc = np.asarray(normals, dtype=np.float32).reshape(3, 3)
            check(lib().rt_scene_add_triangle_smooth(self.h, v3(a), v3(b), v3(c), v3(na), v3(nb), v3(nc), mat, C.byref(out)))
            self._smooth = True
        return out.value

    def MakeMesh(self, vertices, faces, mat, scale=1.0, rotate_y=0.0, translate=(0, 0, 0), normals=None, normal_faces=None, uvs=None, uv_faces=None):
        """An indexed triangle mesh (extension): vertices (n, 3), faces (m, 3); every vertex is scaled, rotated about y (degrees) and translated
        as MakeBox does it.  Degenerate faces are skipped.  Returns (index of the first triangle added, number added).
        normals (k, 3): vertex normals for smooth shading, rotated with the mesh and normalised; normal_faces (m, 3): per face the
        indices into them (default: the faces' vertex indices).
        uvs (k, 2): texture coordinates for an image-textured material, taken as they are; uv_faces (m, 3): per face the indices into
        them (default: the faces' vertex indices)."""
        xyz = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        if idx.size and (idx.min() < 0 or idx.max() > 0xffffffff):
            raise ValueError("MakeMesh: a face index is negative or does not fit 32 bits")
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        first, added = C.c_int32(), C.c_uint32()

        def index_triples(name, given):
            if given is None:
                return None
            a = np.ascontiguousarray(given, dtype=np.int64).reshape(-1, 3)
            if a.shape != idx.shape or (a.size and (a.min() < 0 or a.max() > 0xffffffff)):
                raise ValueError(f"MakeMesh: {name} must hold one non-negative 32-bit index triple per face")
            return np.ascontiguousarray(a, dtype=np.uint32)

        if uvs is None and uv_faces is not None:
            raise ValueError("MakeMesh: uv_faces without uvs")
        if uvs is not None:
            if normals is None and normal_faces is not None:
                raise ValueError("MakeMesh: normal_faces without normals")
            tuv = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 2)
            nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3) if normals is not None else None
            nidx, tidx = index_triples("normal_faces", normal_faces), index_triples("uv_faces", uv_faces)
            check(lib().rt_scene_add_mesh_uv(self.h, xyz.shape[0], xyz, nrm.shape[0] if nrm is not None else 0, nrm.ctypes.data if nrm is not None else None,
                                             tuv.shape[0], tuv, idx.shape[0], idx, nidx.ctypes.data if nidx is not None else None,
                                             tidx.ctypes.data if tidx is not None else None, mat, scale, rotate_y, v3(translate), C.byref(first), C.byref(added)))
            self._uv = True
            self._smooth = getattr(self, "_smooth", False) or normals is not None
            return first.value, added.value
        if normals is None:
            if normal_faces is not None:
                raise ValueError("MakeMesh: normal_faces without normals")
            check(lib().rt_scene_add_mesh(self.h, xyz.shape[0], xyz, idx.shape[0], idx, mat, scale, rotate_y, v3(translate), C.byref(first), C.byref(added)))
            return first.value, added.value
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        nidx = None
        if normal_faces is not None:
            nidx = np.ascontiguousarray(normal_faces, dtype=np.int64).reshape(-1, 3)
            if nidx.shape != idx.shape or (nidx.size and (nidx.min() < 0 or nidx.max() > 0xffffffff)):
                raise ValueError("MakeMesh: normal_faces must hold one non-negative 32-bit index triple per face")
            nidx = np.ascontiguousarray(nidx, dtype=np.uint32)
        check(lib().rt_scene_add_mesh_smooth(self.h, xyz.shape[0], xyz, nrm.shape[0], nrm, idx.shape[0], idx, nidx.ctypes.data if nidx is not None else None,
                                             mat, scale, rotate_y, v3(translate), C.byref(first), C.byref(added)))
        self._smooth = True
        return first.value, added.value

    def vertex_normals(self):
        """The scene's vertex normals, one record per triangle of the flat world in its triangle order (rt_scene_vertex_normals): a structured array of
        capi.TRI_NORMALS_DT (n0, n1, n2; nine zeros = a flat triangle); empty when no triangle of the scene has normals."""
        ptr, n = C.c_void_p(), C.c_uint32()
        check(lib().rt_scene_vertex_normals(self.h, C.byref(ptr), C.byref(n)))
        return self._arr(ptr.value, n.value, capi.TRI_NORMALS_DT)

    def texture_coords(self):
        """The scene's texture coordinates, one record per triangle of the flat world in its triangle order (rt_scene_texture_coords): a structured array of
        capi.TRI_UVS_DT (t0, t1, t2; (0,0), (1,0), (0,1) = a triangle without any); empty when every record is that identity."""
        ptr, n = C.c_void_p(), C.c_uint32()
        check(lib().rt_scene_texture_coords(self.h, C.byref(ptr), C.byref(n)))
        return self._arr(ptr.value, n.value, capi.TRI_UVS_DT)

    def n_triangles(self):
        """How many of the flat world's quads are triangles (its last ones): rt_world_triangles."""
        w, n = self.getWorldPtr(), C.c_uint32()
        check(lib().rt_world_triangles(C.byref(w), C.byref(n)))
        return n.value

    def set_environment(self, image, rotate_y=0.0):
        """An environment map (extension): image (H, W, 3) float, fp32 RGB radiance, row 0 at the top, finite and >= 0; rotate_y in degrees about y.
        Sets background mode 2; Renderer / MultiRenderer push the map at creation."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("set_environment: the image must have shape (H, W, 3)")
        check(lib().rt_scene_set_environment(self.h, img.shape[1], img.shape[0], img.ctypes.data, float(rotate_y)))

    def environment(self):
        """What set_environment stored: ((H, W, 3) float32 copy, u0), or None when the scene has no environment map (rt_scene_environment)."""
        w, h, ptr, u0 = C.c_uint32(), C.c_uint32(), C.c_void_p(), C.c_float()
        check(lib().rt_scene_environment(self.h, C.byref(w), C.byref(h), C.byref(ptr), C.byref(u0)))
        if not ptr.value:
            return None
        buf = (C.c_float * (w.value * h.value * 3)).from_address(ptr.value)
        return np.frombuffer(buf, np.float32).reshape(h.value, w.value, 3).copy(), np.float32(u0.value)

    def set_background(self, color=None):
        """None: the reference's sky gradient; a colour: camera::background of "The Next Week"."""
        if color is None:
            check(lib().rt_scene_set_background(self.h, 0, v3((0, 0, 0))))
        else:
            check(lib().rt_scene_set_background(self.h, 1, v3(color)))
        return self

    def MakeSphere(self, center, radius, mat):
        out = C.c_int32()
        check(lib().rt_scene_add_sphere(self.h, v3(center), radius, mat, C.byref(out)))
        return out.value

    def MakeMovingSphere(self, c0, c1, radius, mat):
        out = C.c_int32()
        check(lib().rt_scene_add_moving_sphere(self.h, v3(c0), v3(c1), radius, mat, C.byref(out)))
        return out.value

    def prim_bounds(self, prim):
        mn, mx = capi.vec3(), capi.vec3()
        check(lib().rt_scene_prim_bounds(self.h, prim, mn, mx))
        return np.array(mn[:], dtype=np.float32), np.array(mx[:], dtype=np.float32)

    def BuildBVH_TopDown(self):
        check(lib().rt_scene_build_bvh_topdown(self.h))
        return self

    def BuildBVH_SAH(self):
        check(lib().rt_scene_build_bvh_sah(self.h))
        return self

    def BuildBVH_BottomUp(self):
        check(lib().rt_scene_build_bvh_bottomup(self.h))
        return self

    def MakeHittableList(self):
        check(lib().rt_scene_set_world_list(self.h))
        return self

    def bvh_node(self, left_ref, right_ref, bounds=None):
        out = C.c_int32()
        if bounds is None:
            check(lib().rt_scene_add_bvh_node(self.h, left_ref, right_ref, None, None, C.byref(out)))
        else:
            mn, mx = v3(bounds[0]), v3(bounds[1])
            check(lib().rt_scene_add_bvh_node(self.h, left_ref, right_ref, mn, mx, C.byref(out)))
        return out.value

    @staticmethod
    def prim_ref(prim):
        return -prim - 1

    def set_world_node_tree(self, root_ref):
        check(lib().rt_scene_set_world_node_tree(self.h, root_ref))
        return self

    def set_traversal(self, mode):
        """0 = the live depth-first stack (BVH.cu:54-106), 1 = the reference's disabled distance-sorted queue (BVH.cu:17-49), fixed,
        2 = a 4-wide walk of the same tree (two levels per visit; not in the reference)"""
        check(lib().rt_scene_set_traversal(self.h, mode))
        return self

    # --- flat view ---
    def getWorldPtr(self):
        w = WorldFlat()
        check(lib().rt_scene_get_flat(self.h, C.byref(w)))
        if getattr(self, "_smooth", False):   # the table travels beside the flat world: Renderer / MultiRenderer push it at creation (a scene without normals: no call)
            w.vertex_normals = self.vertex_normals()
        if getattr(self, "_uv", False):       # likewise the texture coordinates (a scene that was given none: no call)
            w.texture_coords = self.texture_coords()
        if w.background == 2:                 # likewise the environment map
            w.environment = self.environment()
        table = self.textures()               # likewise the texture table, when it says more than the flat world does: an image beyond 0 or a mode that is not the default
        if table is not None and (len(table[0]) > 1 or table[0]["wrap"][0] != capi.WRAP_CLAMP or table[0]["filter"][0] != capi.FILTER_NEAREST):
            w.textures = table
        nmaps = self.normal_maps()            # likewise the normal maps, and with them the table they name their images in
        if nmaps is not None:
            w.normal_maps = nmaps
            if table is not None:
                w.textures = table
        mfacs = self.microfacets()            # likewise the microfacet records; the texture table only with a roughness map
        if mfacs is not None:
            w.microfacets = mfacs
            if table is not None and np.isin(mfacs["on"], (capi.MICROFACET_MAPPED, capi.MICROFACET_GLASS_MAPPED)).any():
                w.textures = table
        interiors = self.interiors()          # likewise the interior records, which need no other table
        if interiors is not None:
            w.interiors = interiors
        cutouts = self.cutouts()              # likewise the cutout records, and with them the table they name their masks in
        if cutouts is not None:
            w.cutouts = cutouts
            if table is not None:
                w.textures = table
        return w

    def _arr(self, ptr, n, dt):
        if n == 0 or not ptr:
            return np.zeros(0, dtype=dt)
        buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dt).copy()

    def arrays(self):
        w = self.getWorldPtr()
        return (self._arr(w.nodes, w.n_nodes, capi.NODE_DT), self._arr(w.prims, w.n_prims, capi.PRIM_DT),
                self._arr(w.materials, w.n_materials, capi.MAT_DT))

    def quads(self):
        w = self.getWorldPtr()
        return self._arr(w.quads, w.n_quads, capi.QUAD_DT)

    def light_table(self, mode):
        """(kind, index, area) arrays of the light table of `mode` ("quads" / 1, "all" / 2, "mesh" / 4, "tree" / 16: permuted into the tree's leaf order) as
        rt_renderer_light_sampling_enable would take it (rt_world_light_table; no GPU); RtError with the world's own reason where it refuses."""
        cap = 4096 if light_sampling_mode(mode) == 16 else 64   # RT_MAX_LIGHTS_TREE, RT_MAX_LIGHTS_MESH
        kind, index, area, n = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_float * cap)(), C.c_uint32(0)
        w = self.getWorldPtr()
        check(lib().rt_world_light_table(C.byref(w), light_sampling_mode(mode), cap, kind, index, area, C.byref(n)))
        return (np.array(kind[: n.value], np.uint32), np.array(index[: n.value], np.uint32), np.array(area[: n.value], np.float32))

    def light_tree(self):
        """(nodes (2 n_l - 1, 8) float32 — min.xyz, skip bits, max.xyz, leaf bits —, cdf (n_l,) float32) of mode "tree" over light_table("tree")
        (rt_world_light_tree; no GPU); RtError with the world's own reason where it refuses."""
        cap = 4096   # RT_MAX_LIGHTS_TREE
        nodes, cdf, n = (C.c_float * (8 * (2 * cap - 1)))(), (C.c_float * cap)(), C.c_uint32(0)
        w = self.getWorldPtr()
        check(lib().rt_world_light_tree(C.byref(w), cap, nodes, C.byref(n), cdf))
        n_l = (n.value + 1) // 2
        return np.array(nodes[: 8 * n.value], np.float32).reshape(n.value, 8), np.array(cdf[:n_l], np.float32)

    def perlin_bytes(self):
        w = self.getWorldPtr()
        return bytes((C.c_char * 6144).from_address(w.perlin)) if w.perlin else b""

    def image(self):
        w = self.getWorldPtr()
        if not w.image:
            return np.zeros((0, 0, 3), np.uint8)
        buf = (C.c_char * (w.image_width * w.image_height * 3)).from_address(w.image)
        return np.frombuffer(buf, dtype=np.uint8).reshape(w.image_height, w.image_width, 3).copy()

    def __del__(self):
        try:
            if self.h:
                lib().rt_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass


LIGHT_SAMPLING_MODES = {"off": 0, "quads": 1, "all": 2, "mesh": 4, "tree": 16, "env": 32}   # RT_LIGHT_SAMPLING_* of one light source each
LIGHT_SAMPLING_COMBINED = {"env+tree": 48}   # RT_LIGHT_SAMPLING_ENV_TREE: the map and the light tree together; a table of its own, the one above is held by name


def light_sampling_mode(on):
    """False / 0 / "off" -> 0, True / 1 / "quads" -> 1, 2 / "all" -> 2, 4 / "mesh" -> 4, 16 / "tree" -> 16, 32 / "env" -> 32, 48 / "env+tree" -> 48
    (RT_LIGHT_SAMPLING_*)"""
    if isinstance(on, str):
        if on in LIGHT_SAMPLING_COMBINED:
            return LIGHT_SAMPLING_COMBINED[on]
        if on not in LIGHT_SAMPLING_MODES:
            raise ValueError(f"light sampling mode {on!r}: one of 'off', 'quads', 'all', 'mesh', 'tree', 'env', 'env+tree'")
        return LIGHT_SAMPLING_MODES[on]
    return int(on)


def feature_mode_for(material_types, has_cutouts):
    """The mode of the feature pass a world asks for, as tools/render.py chooses it: 'full' (RT_AOV_FULL) for a world with a cutout table or a
    constant medium, 'textured' (§27) for one with a noise or an image material, 'plain' for every other.  material_types: the type of every material."""
    kinds = {int(k) for k in material_types}
    if has_cutouts or capi.MAT_ISOTROPIC in kinds:
        return "full"
    return "textured" if kinds & {capi.MAT_LAMBERTIAN_NOISE, capi.MAT_LAMBERTIAN_IMAGE} else "plain"


def normals_table(table):
    """a table of vertex normals as float32 (n, 9): from Scene.vertex_normals()'s records or an array of shape (n, 9) / (n, 3, 3)"""
    a = np.asarray(table)
    if a.dtype == capi.TRI_NORMALS_DT:
        return np.ascontiguousarray(a).view(np.float32).reshape(-1, 9)
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 9)


def _push_normals(fn, handle, table):
    if table is None:
        return fn(handle, None, 0)
    t = normals_table(table)
    return fn(handle, t.ctypes.data if len(t) else None, len(t))


def uvs_table(table):
    """a table of texture coordinates as float32 (n, 6): from Scene.texture_coords()'s records or an array of shape (n, 6) / (n, 3, 2)"""
    a = np.asarray(table)
    if a.dtype == capi.TRI_UVS_DT:
        return np.ascontiguousarray(a).view(np.float32).reshape(-1, 6)
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 6)


def _push_uvs(fn, handle, table):
    if table is None:
        return fn(handle, None, 0)
    t = uvs_table(table)
    return fn(handle, t.ctypes.data if len(t) else None, len(t))


def wrap_mode(wrap):
    """"clamp" / 0, "repeat" / 1 -> RT_WRAP_*"""
    return {"clamp": capi.WRAP_CLAMP, "repeat": capi.WRAP_REPEAT}.get(wrap, wrap)


def filter_mode(filter):
    """"nearest" / 0, "bilinear" / 1 -> RT_FILTER_*"""
    return {"nearest": capi.FILTER_NEAREST, "bilinear": capi.FILTER_BILINEAR}.get(filter, filter)


def texture_table(entries):
    """A texture table as (records, texels) from entries (rgb, wrap, filter): rgb a uint8 array [H][W][3] or None for an empty entry; entry 0
    stands for the world's image.  A (records, texels) pair passes through."""
    if isinstance(entries, tuple) and len(entries) == 2 and getattr(entries[0], "dtype", None) == capi.TEXTURE_DT:
        return np.ascontiguousarray(entries[0]), np.ascontiguousarray(entries[1], np.uint8).reshape(-1, 3)
    records, texels, at = np.zeros(len(entries), capi.TEXTURE_DT), [], 0
    for k, (rgb, wrap, filt) in enumerate(entries):
        img = np.zeros((0, 0, 3), np.uint8) if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("texture_table: an image must have shape (H, W, 3)")
        records[k] = (img.shape[1], img.shape[0], wrap_mode(wrap), filter_mode(filt), at)
        texels.append(img.reshape(-1, 3))
        at += img.shape[0] * img.shape[1]
    return records, (np.concatenate(texels) if texels else np.zeros((0, 3), np.uint8))


def _push_textures(fn, handle, table):
    if table is None:
        return fn(handle, None, 0, None)
    records, texels = texture_table(table)
    return fn(handle, records.ctypes.data if len(records) else None, len(records), texels.ctypes.data if len(texels) else None)


def _push_records(fn, handle, table, dtype):
    """a per-material table (normal maps, microfacets, interiors, cutouts) as records of `dtype`; None = off"""
    if table is None:
        return fn(handle, None, 0)
    table = np.ascontiguousarray(table, dtype).reshape(-1)
    return fn(handle, table.ctypes.data if len(table) else None, len(table))


def _info_pair(fn, handle, count):
    """a table's _info query: {'enabled', count}"""
    out = (C.c_uint32 * 2)()
    check(fn(handle, out))
    return {"enabled": bool(out[0]), count: out[1]}


def _kernel_has(fn, handle):
    """a kernel_* query: whether the next launch runs an instantiation of the family"""
    out = C.c_uint32(0)
    check(fn(handle, C.byref(out)))
    return bool(out.value)


def _env_image(image):
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("environment: the image must have shape (H, W, 3)")
    return img


def _push_environment(fn, handle, image, u0):
    if image is None:
        return fn(handle, 0, 0, None, 0.0)
    img = _env_image(image)
    return fn(handle, img.shape[1], img.shape[0], img.ctypes.data, float(u0))


class Renderer:
    """Renderer (main/src/Renderer.h:12-47) over the C ABI."""

    def __init__(self, handle, cfg):
        self.h = handle
        self.cfg = cfg

    @classmethod
    def MakeRenderer(cls, render_width, render_height, samples_per_pixel, max_depth, cam, world,
                     seed=1984, device=0, rank=0, world_size=1, variant=0):
        cfg = RenderConfig(render_width, render_height, samples_per_pixel, max_depth, seed, device, rank, world_size, variant)
        h = C.c_void_p()
        check(lib().rt_renderer_create(C.byref(cfg), C.byref(cam), C.byref(world), C.byref(h)))
        r = cls(h, cfg)
        if len(getattr(world, "vertex_normals", ())):
            r.shading_normals(world.vertex_normals)
        if len(getattr(world, "texture_coords", ())):
            r.texture_coords(world.texture_coords)
        if getattr(world, "environment", None) is not None:
            r.environment(world.environment[0], u0=world.environment[1])
        if getattr(world, "textures", None) is not None:
            r.textures(world.textures)
        if getattr(world, "normal_maps", None) is not None:
            r.normal_maps(world.normal_maps)
        if getattr(world, "microfacets", None) is not None:
            r.microfacets(world.microfacets)
        if getattr(world, "interiors", None) is not None:
            r.interiors(world.interiors)
        if getattr(world, "cutouts", None) is not None:
            r.cutouts(world.cutouts)
        return r

    def Render(self):
        check(lib().rt_renderer_render(self.h))

    def render_async(self, stream=None, d_out=None):
        """Render() on the caller's stream without a host wait.  d_out is written in the stream's order; on a two-slot renderer (run_ahead_info) the
        frame is generated and traced ahead of the stream, on a stream of the renderer's own, and only resolved into d_out in order."""
        check(lib().rt_renderer_render_async(self.h, C.c_void_p(stream or 0), C.c_void_p(d_out or 0)))

    def set_camera(self, cam):
        """`params.cam = *m.cam` (Renderer.cu:117): the camera of every launch from now on; a different camera discards the refinement state."""
        check(lib().rt_renderer_set_camera(self.h, C.byref(cam) if cam is not None else None))

    def refine(self, n_samples):
        """Add n_samples more samples per pixel; the framebuffer then has the bits of ONE render at the accumulated count. Returns that count."""
        check(lib().rt_renderer_refine(self.h, n_samples))
        return self.refine_info()["samples"]

    def refine_async(self, n_samples, stream=None, d_out=None):
        check(lib().rt_renderer_refine_async(self.h, C.c_void_p(stream or 0), C.c_void_p(d_out or 0), n_samples))

    def refine_reset(self):
        check(lib().rt_renderer_refine_reset(self.h))

    def refine_info(self):
        """{'samples', 'pass_spp', 'bytes'}: samples accumulated, samples per pixel of one internal pass, bytes held for refinement."""
        out = (C.c_uint64 * 3)()
        check(lib().rt_renderer_refine_info(self.h, out))
        return {"samples": out[0], "pass_spp": out[1], "bytes": out[2]}

    def refine_sums(self):
        """(H, W, 4) float32: per pixel (sum R, sum G, sum B, sum Y^2) of the samples so far, unscaled (world_size == 1)."""
        out = np.zeros((self.cfg.height, self.cfg.width, 4), dtype=np.float32)
        check(lib().rt_renderer_refine_download_sums(self.h, out, out.size))
        return out

    def noise(self):
        """Relative RMS standard error of the frame's mean luminance after the samples so far (rt_renderer_refine_noise)."""
        out = C.c_double()
        check(lib().rt_renderer_refine_noise(self.h, C.byref(out)))
        return out.value

    def enable_aov(self, max_samples=0, textured=False, full=False):
        """Accumulate first-hit feature buffers alongside every refine step from now on (restarts the refinement); max_samples = 0: every sample.
        textured: mode RT_AOV_TEXTURED, which also covers noise and image materials (the plain mode refuses a world that has one).
        full: mode RT_AOV_FULL, the textured mode that also follows alpha cutouts and constant media.  One mode at a time."""
        if textured and full:
            raise ValueError("enable_aov: textured and full are two modes; pass one of them")
        if full:
            check(lib().rt_renderer_aov_enable_mode(self.h, max_samples, capi.AOV_FULL))
        elif textured:
            check(lib().rt_renderer_aov_enable_mode(self.h, max_samples, capi.AOV_TEXTURED))
        else:
            check(lib().rt_renderer_aov_enable(self.h, max_samples))

    def aov_mode(self):
        """'plain', 'textured' or 'full': the mode of the last successful enable_aov ('plain' before any)."""
        out = C.c_uint32()
        check(lib().rt_renderer_aov_mode(self.h, C.byref(out)))
        return {capi.AOV_PLAIN: "plain", capi.AOV_TEXTURED: "textured", capi.AOV_FULL: "full"}[out.value]

    def aov_info(self):
        """{'enabled', 'samples', 'bytes'}: whether the feature buffers are on, the samples per pixel they cover, bytes held."""
        out = (C.c_uint64 * 3)()
        check(lib().rt_renderer_aov_info(self.h, out))
        return {"enabled": bool(out[0]), "samples": out[1], "bytes": out[2]}

    def aov_sums(self):
        """(H, W, 8) float32, unscaled: (sum Nx, sum Ny, sum Nz, sum t, sum Ar, sum Ag, sum Ab, hits) per pixel (world_size == 1)."""
        out = np.zeros((self.cfg.height, self.cfg.width, 8), dtype=np.float32)
        check(lib().rt_renderer_aov_download(self.h, out, out.size))
        return out

    def aov(self):
        """{'normal' (H,W,3), 'depth' (H,W), 'albedo' (H,W,3), 'coverage' (H,W)}: the feature sums divided by the samples they cover."""
        sums, inv = self.aov_sums(), np.float32(1.0) / np.float32(self.aov_info()["samples"])
        return {"normal": sums[..., 0:3] * inv, "depth": sums[..., 3] * inv, "albedo": sums[..., 4:7] * inv, "coverage": sums[..., 7] * inv}

    @staticmethod
    def denoise_params(**params):
        """rt_denoise_params with the library's defaults, then iterations / sigma_depth / sigma_lum / demodulate as given."""
        dp = capi.DenoiseParams()
        check(lib().rt_denoise_params_default(C.byref(dp)))
        for k, v in params.items():
            if k not in ("iterations", "sigma_depth", "sigma_lum", "demodulate"):
                raise TypeError(f"denoise: unknown parameter {k}")
            setattr(dp, k, v)
        return dp

    def denoise(self, **params):
        """Filter the refined frame (rt_renderer_denoise) and return the denoised image, (H, W, 4) float32; the refined frame stays as it is."""
        check(lib().rt_renderer_denoise(self.h, C.byref(self.denoise_params(**params))))
        out = np.zeros((self.cfg.height, self.cfg.width, 4), dtype=np.float32)
        check(lib().rt_renderer_denoise_download(self.h, out, out.size))
        return out

    def denoise_async(self, stream=None, **params):
        check(lib().rt_renderer_denoise_async(self.h, C.c_void_p(stream or 0), C.byref(self.denoise_params(**params))))

    def light_sampling(self, on=True):
        """Next-event estimation from the next launch on (rt_renderer_light_sampling_enable); a change restarts the refinement.
        False / 0 / "off": off; True / 1 / "quads": over the world's quad lights; 2 / "all": over its quad and sphere lights; 4 / "mesh": over its quad,
        sphere and triangle lights (an emissive mesh); 16 / "tree": over the same lights, up to 4096, chosen by area and found through a light tree;
        32 / "env": over the environment map of a background-2 world alone, directions drawn in proportion to radiance times solid angle;
        48 / "env+tree": over that map and the light tree together, half of the light draws each, at image-textured Lambertian hits too; a world without
        lights is accepted and sampled as the map alone."""
        check(lib().rt_renderer_light_sampling_enable(self.h, light_sampling_mode(on)))

    def light_sampling_mode(self):
        """0 (off), 1 (quad lights), 2 (quad and sphere lights), 4 (quad, sphere and triangle lights), 16 (those, by area, through a light tree), 32 (the
        environment map) or 48 (the map and the light tree together): the mode the next launch runs in."""
        out = (C.c_uint32 * 2)()
        check(lib().rt_renderer_light_sampling_info(self.h, out))
        return out[0]

    def light_sampling_info(self):
        """{'enabled', 'lights'}: whether light sampling is on (in any mode: light_sampling_mode() tells which), and the number of lights in the
        mode's table — off: of quad lights; "env": the texels of the map; "env+tree": of the light tree's table, which may be empty — (0: the world cannot be light-sampled)."""
        return _info_pair(lib().rt_renderer_light_sampling_info, self.h, "lights")

    def shading_normals(self, table):
        """Smooth shading from the next launch on (rt_renderer_shading_normals): table = one record of three vertex normals per triangle of
        the world (Scene.vertex_normals(), or anything of shape (n, 9) / (n, 3, 3)), None = off.  A change restarts the refinement."""
        check(_push_normals(lib().rt_renderer_shading_normals, self.h, table))

    def shading_normals_info(self):
        """{'enabled', 'smooth'}: whether a table of vertex normals is on, and how many of its records are not flat."""
        return _info_pair(lib().rt_renderer_shading_normals_info, self.h, "smooth")

    def texture_coords(self, table):
        """Texture coordinates from the next launch on (rt_renderer_texture_coords): table = one record of three (u, v) per triangle of the
        world (Scene.texture_coords(), or anything of shape (n, 6) / (n, 3, 2)), None = off.  A change restarts the refinement."""
        check(_push_uvs(lib().rt_renderer_texture_coords, self.h, table))

    def texture_coords_info(self):
        """{'enabled', 'mapped'}: whether a table of texture coordinates is on, and how many of its records are not the identity."""
        return _info_pair(lib().rt_renderer_texture_coords_info, self.h, "mapped")

    def environment(self, image, u0=0.0):
        """The environment map of a background-2 world from the next launch on (rt_renderer_environment): image (H, W, 3) float, u0 in [0, 1) the
        rotation about y as a shift of u; None = off (Render() then refuses).  A change restarts the refinement."""
        check(_push_environment(lib().rt_renderer_environment, self.h, image, u0))

    def textures(self, table):
        """The texture table from the next launch on (rt_renderer_textures): (records, texels) as Scene.textures() gives it, or a list of
        (rgb, wrap, filter) entries (api.texture_table); None = off.  A change restarts the refinement; an unchanged table keeps it."""
        check(_push_textures(lib().rt_renderer_textures, self.h, table))

    def normal_maps(self, table):
        """The normal-map table from the next launch on (rt_renderer_normal_maps): one record of capi.NORMAL_MAP_DT per material as Scene.normal_maps()
        gives it; None = off.  The images it names are the texture table's (Renderer.textures).  A change restarts the refinement; an unchanged table keeps it."""
        check(_push_records(lib().rt_renderer_normal_maps, self.h, table, capi.NORMAL_MAP_DT))

    def normal_maps_info(self):
        """{'enabled', 'mapped'} of the renderer's normal-map table: mapped = how many materials have a map."""
        return _info_pair(lib().rt_renderer_normal_maps_info, self.h, "mapped")

    def kernel_normal_map(self):
        """True when the next launch runs the streaming kernel's normal-map family (rt_renderer_kernel_normal_map): a normal-map table is on."""
        return _kernel_has(lib().rt_renderer_kernel_normal_map, self.h)

    def microfacets(self, table):
        """The microfacet table from the next launch on (rt_renderer_microfacets): one record of capi.MICROFACET_DT per material as
        Scene.microfacets() gives it; None = off.  A mapped record names its image in the texture table (Renderer.textures).  A change restarts the refinement."""
        check(_push_records(lib().rt_renderer_microfacets, self.h, table, capi.MICROFACET_DT))

    def microfacets_info(self):
        """{'enabled', 'records'} of the renderer's microfacet table: records = how many materials have one."""
        return _info_pair(lib().rt_renderer_microfacets_info, self.h, "records")

    def interiors(self, table):
        """The interior table from the next launch on (rt_renderer_interiors): one record of capi.INTERIOR_DT per material as Scene.interiors()
        gives it; None = off.  A change restarts the refinement."""
        check(_push_records(lib().rt_renderer_interiors, self.h, table, capi.INTERIOR_DT))

    def interiors_info(self):
        """{'enabled', 'records'} of the renderer's interior table: records = how many materials have one."""
        return _info_pair(lib().rt_renderer_interiors_info, self.h, "records")

    def kernel_interior(self):
        """True when the next launch runs the streaming kernel's solid-glass family (rt_renderer_kernel_interior): an interior table is on."""
        return _kernel_has(lib().rt_renderer_kernel_interior, self.h)

    def cutouts(self, table):
        """The cutout table from the next launch on (rt_renderer_cutouts): one record of capi.CUTOUT_DT per material as Scene.cutouts() gives it;
        None = off.  The masks are entries of the renderer's texture table (textures()).  A change restarts the refinement."""
        check(_push_records(lib().rt_renderer_cutouts, self.h, table, capi.CUTOUT_DT))

    def cutouts_info(self):
        """{'enabled', 'records'} of the renderer's cutout table: records = how many materials have one."""
        return _info_pair(lib().rt_renderer_cutouts_info, self.h, "records")

    def kernel_cutout(self):
        """True when the next launch runs the streaming kernel's cutout family (rt_renderer_kernel_cutout): a cutout table is on.  kernel_interior() and
        kernel_microfacet() are True then too: the cutout forms are those forms, reading one more table."""
        return _kernel_has(lib().rt_renderer_kernel_cutout, self.h)

    def kernel_microfacet(self):
        """True when the next launch runs the streaming kernel's microfacet family (rt_renderer_kernel_microfacet): a microfacet table is on, or an
        interior table — the solid-glass forms (kernel_interior) are microfacet forms that read one more table."""
        return _kernel_has(lib().rt_renderer_kernel_microfacet, self.h)

    def textures_info(self):
        """{'enabled', 'entries'} of the renderer's texture table."""
        return _info_pair(lib().rt_renderer_textures_info, self.h, "entries")

    def environment_info(self):
        """{'enabled', 'width', 'height', 'u0'} of the renderer's environment map."""
        out = (C.c_uint32 * 4)()
        check(lib().rt_renderer_environment_info(self.h, out))
        return {"enabled": bool(out[0]), "width": out[1], "height": out[2], "u0": np.array([out[3]], np.uint32).view(np.float32)[0]}

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib().rt_renderer_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def kernel_times(self, renders_back=0):
        """(primary_rays_kernel, dominant kernel, resolve_kernel) ms of one of the last 32 render calls, by HIP events, summed over its passes."""
        out = (C.c_float * 3)()
        check(lib().rt_renderer_kernel_times(self.h, renders_back, out))
        return tuple(out)

    def pass_info(self):
        """{'n_passes', 'pass_spp', 'bytes_per_sample', 'buffer_bytes'}: how a render is cut into passes (rt_renderer_pass_info)."""
        out = (C.c_uint64 * 4)()
        check(lib().rt_renderer_pass_info(self.h, out))
        return {"n_passes": out[0], "pass_spp": out[1], "bytes_per_sample": out[2], "buffer_bytes": out[3]}

    def run_ahead_info(self):
        """{'slots', 'calls', 'overlapped', 'second_set_bytes'}: frame slots, render_async calls that ran ahead, those that found the call before them
        still in flight when they were enqueued, bytes of the second set of per-pass buffers (rt_renderer_run_ahead_info)."""
        out = (C.c_uint64 * 4)()
        check(lib().rt_renderer_run_ahead_info(self.h, out))
        return {"slots": out[0], "calls": out[1], "overlapped": out[2], "second_set_bytes": out[3]}

    def kernel_info(self):
        """{'variant', 'lds_resident', 'workgroup', 'workgroups_per_cu'} the renderer resolved to."""
        out = (C.c_uint32 * 4)()
        check(lib().rt_renderer_kernel_info(self.h, C.byref(out)))
        return {"variant": out[0], "lds_resident": bool(out[1]), "workgroup": out[2], "workgroups_per_cu": out[3]}

    def kernel_form(self):
        """{'kernel': 'baseline' | 'stream' | 'xchg', 'exact', 'filter', 'world', 'ext', 'big', 'wide', 'tol', 'nee'}: the instantiation the next
        launch runs (rt_renderer_kernel_form); the template arguments are zeros for the baseline and the exchange kernel."""
        out = (C.c_uint32 * 9)()
        check(lib().rt_renderer_kernel_form(self.h, out))
        form = {"kernel": ("baseline", "stream", "xchg")[out[0]]}
        form.update(zip(("exact", "filter", "world", "ext", "big", "wide", "tol", "nee"), out[1:]))
        return form

    def kernel_light_tree(self):
        """True when the next launch runs the streaming kernel's light-tree family (rt_renderer_kernel_light_tree): mode "tree" or "env+tree" is on."""
        return _kernel_has(lib().rt_renderer_kernel_light_tree, self.h)

    def kernel_env_light(self):
        """True when the next launch runs the streaming kernel's environment-sampling family (rt_renderer_kernel_env_light): mode "env" or "env+tree" is on."""
        return _kernel_has(lib().rt_renderer_kernel_env_light, self.h)

    def kernel_triangles(self):
        """True when the next launch runs the streaming kernel's triangle family (rt_renderer_kernel_triangles)."""
        return _kernel_has(lib().rt_renderer_kernel_triangles, self.h)

    def DownloadRenderbuffer(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 4), dtype=np.float32)
        check(lib().rt_renderer_download(self.h, out, out.size))
        return out

    def shard_floats(self):
        n = C.c_size_t()
        check(lib().rt_renderer_shard_floats(self.h, C.byref(n)))
        return n.value

    def assemble(self, d_gathered, d_image, stream=None):
        check(lib().rt_renderer_assemble(self.h, C.c_void_p(d_gathered), C.c_void_p(d_image), C.c_void_p(stream or 0)))

    def close(self):
        if self.h:
            lib().rt_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiRenderer:
    """Renderer over the N GPUs of one node from ONE process (rt_multi_renderer_*): tile shards, one RCCL gather at frame end."""

    def __init__(self, handle, cfg):
        self.h, self.cfg = handle, cfg

    @classmethod
    def MakeRenderer(cls, render_width, render_height, samples_per_pixel, max_depth, cam, world, n_gpus, seed=1984, devices=None, variant=0):
        cfg = RenderConfig(render_width, render_height, samples_per_pixel, max_depth, seed, 0, 0, 1, variant)
        devs = (C.c_int32 * n_gpus)(*devices) if devices is not None else None
        h = C.c_void_p()
        check(lib().rt_multi_renderer_create(C.byref(cfg), C.byref(cam), C.byref(world), n_gpus, devs, C.byref(h)))
        m = cls(h, cfg)
        if len(getattr(world, "vertex_normals", ())):
            m.shading_normals(world.vertex_normals)
        if len(getattr(world, "texture_coords", ())):
            m.texture_coords(world.texture_coords)
        if getattr(world, "environment", None) is not None:
            m.environment(world.environment[0], u0=world.environment[1])
        if getattr(world, "textures", None) is not None:
            m.textures(world.textures)
        if getattr(world, "normal_maps", None) is not None:
            m.normal_maps(world.normal_maps)
        if getattr(world, "microfacets", None) is not None:
            m.microfacets(world.microfacets)
        if getattr(world, "interiors", None) is not None:
            m.interiors(world.interiors)
        if getattr(world, "cutouts", None) is not None:
            m.cutouts(world.cutouts)
        return m

    def Render(self):
        check(lib().rt_multi_renderer_render(self.h))

    def set_camera(self, cam):
        """rt_renderer_set_camera on every rank."""
        check(lib().rt_multi_renderer_set_camera(self.h, C.byref(cam) if cam is not None else None))

    def refine(self, n_samples):
        """rt_renderer_refine on every rank, then the usual gather + assembly."""
        check(lib().rt_multi_renderer_refine(self.h, n_samples))

    def light_sampling(self, on=True):
        """rt_renderer_light_sampling_enable on every rank; `on` as Renderer.light_sampling takes it ("env" included)."""
        check(lib().rt_multi_renderer_light_sampling_enable(self.h, light_sampling_mode(on)))

    def shading_normals(self, table):
        """rt_renderer_shading_normals on every rank; `table` as Renderer.shading_normals takes it."""
        check(_push_normals(lib().rt_multi_renderer_shading_normals, self.h, table))

    def texture_coords(self, table):
        """rt_renderer_texture_coords on every rank; `table` as Renderer.texture_coords takes it."""
        check(_push_uvs(lib().rt_multi_renderer_texture_coords, self.h, table))

    def environment(self, image, u0=0.0):
        """rt_renderer_environment on every rank; arguments as Renderer.environment takes them."""
        check(_push_environment(lib().rt_multi_renderer_environment, self.h, image, u0))

    def textures(self, table):
        """rt_renderer_textures on every rank; `table` as Renderer.textures takes it."""
        check(_push_textures(lib().rt_multi_renderer_textures, self.h, table))

    def normal_maps(self, table):
        """rt_renderer_normal_maps on every rank; `table` as Renderer.normal_maps takes it."""
        check(_push_records(lib().rt_multi_renderer_normal_maps, self.h, table, capi.NORMAL_MAP_DT))

    def normal_maps_info(self):
        """{'enabled', 'mapped'} of the ranks' normal-map table (they hold the same one)."""
        return _info_pair(lib().rt_multi_renderer_normal_maps_info, self.h, "mapped")

    def microfacets(self, table):
        """rt_renderer_microfacets on every rank; `table` as Renderer.microfacets takes it."""
        check(_push_records(lib().rt_multi_renderer_microfacets, self.h, table, capi.MICROFACET_DT))

    def interiors(self, table):
        """rt_renderer_interiors on every rank; `table` as Renderer.interiors takes it."""
        check(_push_records(lib().rt_multi_renderer_interiors, self.h, table, capi.INTERIOR_DT))

    def cutouts(self, table):
        """rt_renderer_cutouts on every rank; `table` as Renderer.cutouts takes it."""
        check(_push_records(lib().rt_multi_renderer_cutouts, self.h, table, capi.CUTOUT_DT))

    def cutouts_info(self):
        """{'enabled', 'records'} of the ranks' cutout table (they hold the same one)."""
        return _info_pair(lib().rt_multi_renderer_cutouts_info, self.h, "records")

    def microfacets_info(self):
        """{'enabled', 'records'} of the ranks' microfacet table (they hold the same one)."""
        return _info_pair(lib().rt_multi_renderer_microfacets_info, self.h, "records")

    def textures_info(self):
        """{'enabled', 'entries'} of the ranks' texture table (they hold the same one)."""
        return _info_pair(lib().rt_multi_renderer_textures_info, self.h, "entries")

    def DownloadRenderbuffer(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 4), dtype=np.float32)
        check(lib().rt_multi_renderer_download(self.h, out, out.size))
        return out

    def times(self):
        """(host wall-clock of Render, slowest rank's kernels, exchange + assembly on GPU 0) in ms"""
        out = (C.c_float * 3)()
        check(lib().rt_multi_renderer_times(self.h, out))
        return tuple(out)

    def close(self):
        if self.h:
            lib().rt_multi_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_info(device=0):
    """rt_device_info: {'compute_units', 'clock_khz', 'memory_mib', 'memory_clock_khz'}"""
    out = (C.c_uint32 * 4)()
    check(lib().rt_device_info(device, out))
    return {"compute_units": out[0], "clock_khz": out[1], "memory_mib": out[2], "memory_clock_khz": out[3]}


def shard_layout(width, height, world_size):
    """rt_shard_layout (host): (tiles_x, n_tiles, n_local_tiles, shard_floats)"""
    out = (C.c_uint32 * 4)()
    check(lib().rt_shard_layout(width, height, world_size, out))
    return tuple(out)


def shard_pixel_map(width, height, world_size, rank):
    """rt_shard_pixel_map (host): global pixel id of every position of rank's shard, 0xffffffff for padding"""
    n = shard_layout(width, height, world_size)[2] * 64
    out = np.zeros(n, np.uint32)
    check(lib().rt_shard_pixel_map(width, height, world_size, rank, out, n))
    return out


# --- device probes -------------------------------------------------------------------------------
def probe_aabb(boxes, rays, max_dist, device=0):
    n = len(boxes)
    hit = np.zeros(n, np.int32); dist = np.zeros(n, np.float32)
    check(lib().rt_probe_aabb(device, n, np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(rays, np.float32),
                              np.ascontiguousarray(max_dist, np.float32), hit, dist))
    return hit, dist


def probe_sphere(rays, spheres, device=0):
    n = len(rays)
    t = np.zeros(n, np.float32)
    check(lib().rt_probe_sphere(device, n, np.ascontiguousarray(rays, np.float32), np.ascontiguousarray(spheres, np.float32), t))
    return t


def probe_trace(world, rays, device=0):
    n = len(rays)
    hit = np.zeros(n, np.int32); t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); nrm = np.zeros((n, 3), np.float32)
    check(lib().rt_probe_trace(device, C.byref(world), n, np.ascontiguousarray(rays, np.float32), hit, t, prim, nrm))
    return hit, t, prim, nrm


def probe_scatter(seed, mats, rays, dist, normals, keys, device=0):
    n = len(rays)
    mats = np.ascontiguousarray(mats, dtype=capi.MAT_DT)
    sc = np.zeros(n, np.int32); orays = np.zeros((n, 7), np.float32); att = np.zeros((n, 3), np.float32); draws = np.zeros(n, np.uint32)
    check(lib().rt_probe_scatter(device, seed, n, mats.ctypes.data, np.ascontiguousarray(rays, np.float32),
                                 np.ascontiguousarray(dist, np.float32), np.ascontiguousarray(normals, np.float32),
                                 np.ascontiguousarray(keys, np.uint32), sc, orays, att, draws))
    return sc, orays, att, draws


def probe_camera(seed, cam, st, keys, device=0):
    n = len(st)
    orays = np.zeros((n, 7), np.float32); draws = np.zeros(n, np.uint32)
    check(lib().rt_probe_camera(device, seed, C.byref(cam), n, np.ascontiguousarray(st, np.float32),
                                np.ascontiguousarray(keys, np.uint32), orays, draws))
    return orays, draws


def probe_sphere_hit(prims, rays, preset, device=0):
    """rt_probe_sphere_hit: (n,) PRIM_DT spheres, (n, 7) rays, (n,) preset rec.distance -> hit, rec.distance, normal (n, 3)"""
    n = len(rays)
    prims = np.ascontiguousarray(prims, dtype=capi.PRIM_DT)
    hit = np.zeros(n, np.int32); dist = np.zeros(n, np.float32); nrm = np.zeros((n, 3), np.float32)
    check(lib().rt_probe_sphere_hit(device, n, prims.ctypes.data, np.ascontiguousarray(rays, np.float32),
                                    np.ascontiguousarray(preset, np.float32), hit, dist, nrm))
    return hit, dist, nrm


def probe_scatter_tape(mats, rays, dist, normals, tape, offsets, device=0):
    """rt_probe_scatter_tape: probe_scatter with uniforms u = k * 2^-24 from `tape` (uint32 k); case i draws
    tape[offsets[i, 0]:][:offsets[i, 1]] (draws > offsets[i, 1] = the case wanted more)"""
    n = len(rays)
    mats = np.ascontiguousarray(mats, dtype=capi.MAT_DT)
    tape = np.ascontiguousarray(tape, np.uint32)
    sc = np.zeros(n, np.int32); orays = np.zeros((n, 7), np.float32); att = np.zeros((n, 3), np.float32); draws = np.zeros(n, np.uint32)
    check(lib().rt_probe_scatter_tape(device, n, mats.ctypes.data, np.ascontiguousarray(rays, np.float32),
                                      np.ascontiguousarray(dist, np.float32), np.ascontiguousarray(normals, np.float32), tape, len(tape),
                                      np.ascontiguousarray(offsets, np.uint32), sc, orays, att, draws))
    return sc, orays, att, draws


def probe_camera_tape(cam, st, tape, offsets, device=0):
    """rt_probe_camera_tape: probe_camera with uniforms from `tape`, as probe_scatter_tape"""
    n = len(st)
    tape = np.ascontiguousarray(tape, np.uint32)
    orays = np.zeros((n, 7), np.float32); draws = np.zeros(n, np.uint32)
    check(lib().rt_probe_camera_tape(device, C.byref(cam), n, np.ascontiguousarray(st, np.float32), tape, len(tape),
                                     np.ascontiguousarray(offsets, np.uint32), orays, draws))
    return orays, draws


def _tape_or_one(tape):
    tape = np.ascontiguousarray(tape, np.uint32)
    return tape if len(tape) else np.array([0x800001], np.uint32), len(tape)   # an empty tape still needs an address


def camera_rays_batch(cam, st, tape, offsets):
    """rt_camera_rays_batch (HOST, no GPU): the camera's rule, any of the seven types, on given (s, t) with uniforms from `tape` as
    probe_camera_tape takes them -> rays (n, 7) = (o, d, time), uniforms consumed (n,)"""
    n = len(st)
    tape, tape_len = _tape_or_one(tape)
    orays = np.zeros((n, 7), np.float32); draws = np.zeros(n, np.uint32)
    check(lib().rt_camera_rays_batch(C.byref(cam), n, np.ascontiguousarray(st, np.float32).reshape(-1), tape, tape_len,
                                     np.ascontiguousarray(offsets, np.uint32).reshape(-1), orays, draws))
    return orays, draws


def probe_camera_lens(cam, st, tape, offsets, device=0):
    """rt_probe_camera_lens: camera_rays_batch for a lens camera (types 16 to 19) on the device, one lane per case"""
    n = len(st)
    tape, tape_len = _tape_or_one(tape)
    orays = np.zeros((n, 7), np.float32); draws = np.zeros(n, np.uint32)
    check(lib().rt_probe_camera_lens(device, C.byref(cam), n, np.ascontiguousarray(st, np.float32).reshape(-1), tape, tape_len,
                                     np.ascontiguousarray(offsets, np.uint32).reshape(-1), orays, draws))
    return orays, draws


def probe_radiance(cfg, cam, world, keys):
    n = len(keys)
    out = np.zeros((n, 3), np.float32)
    check(lib().rt_probe_radiance(C.byref(cfg), C.byref(cam), C.byref(world), n, np.ascontiguousarray(keys, np.uint32), out))
    return out


def probe_sphere_index(cam, width, height, spheres, device=0):
    out = np.zeros(width * height, np.int32)
    spheres = np.ascontiguousarray(spheres, np.float32)
    check(lib().rt_probe_sphere_index(device, C.byref(cam), width, height, len(spheres), spheres, out))
    return out.reshape(height, width)


def probe_rng(seed, keys, n_draws, device=0):
    n = len(keys)
    out = np.zeros((n, n_draws), np.float32)
    check(lib().rt_probe_rng(device, seed, n, np.ascontiguousarray(keys, np.uint32), n_draws, out))
    return out


def probe_math(fn, a, b=None, device=0):
    """rt_probe_math: fn 0 log, 1 sin, 2 acos, 3 atan2(a, b)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(a if b is None else b, np.float32)
    out = np.zeros_like(a)
    check(lib().rt_probe_math(device, fn, len(a), a, b, out))
    return out


GLM_FUNCTIONS = ("dot", "cross", "normalize", "reflect", "refract", "mix3", "mix1", "min3", "max3", "compmax", "compmin",
                 "clamp01_sqrt", "near_zero", "length2", "lerp", "radians", "ray")
_GLM_SHAPES = ((6, 1), (6, 3), (3, 3), (6, 3), (7, 3), (7, 3), (3, 1), (6, 3), (6, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (7, 3), (1, 1), (10, 4))


def probe_glm(name, inputs, device=0):
    """rt_probe_glm: one function of the device math vocabulary (GLM_FUNCTIONS) over an (n, nin) array -> (n, nout)."""
    fn = GLM_FUNCTIONS.index(name)
    nin, nout = _GLM_SHAPES[fn]
    a = np.ascontiguousarray(inputs, np.float32).reshape(-1, nin)
    out = np.zeros((len(a), nout), np.float32)
    check(lib().rt_probe_glm(device, fn, len(a), a, out))
    return out


def probe_aabb_misc(boxes):
    """rt_probe_aabb_misc (host): (n, 12) boxes a, b -> (n, 20) [axis, area, centroid, union, a += b, compares]."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 12)
    out = np.zeros((len(b), 20), np.float32)
    check(lib().rt_probe_aabb_misc(len(b), b, out))
    return out


def device_count():
    n = C.c_int()
    check(lib().rt_device_count(C.byref(n)))
    return n.value


def probe_aabb_regular(boxes, rays, max_dist, device=0):
    n = len(boxes)
    reg = np.zeros(n, np.int32); hit = np.zeros(n, np.int32); dist = np.zeros(n, np.float32)
    check(lib().rt_probe_aabb_regular(device, n, np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(rays, np.float32),
                                      np.ascontiguousarray(max_dist, np.float32), reg, hit, dist))
    return reg, hit, dist


def selftest_fastdiv(first_den, n_den, num_exp=0, den_exp=0, device=0, four=False):
    """(mismatching pairs, example) over n_den divisor significands x all 2^23 numerator significands;
    four=True checks the 4-instruction two-word-reciprocal form (fast_div_exact4)."""
    bad = C.c_uint64()
    ex = np.zeros(2, np.uint32)
    fn = lib().rt_selftest_fastdiv4 if four else lib().rt_selftest_fastdiv
    check(fn(device, first_den, n_den, num_exp, den_exp, C.byref(bad), ex))
    return bad.value, ex


def selftest_fastrcp(device=0):
    """rt_selftest_fastrcp: (values checked, mismatches, example bits)."""
    n, bad, ex = C.c_uint64(), C.c_uint64(), C.c_uint32()
    check(lib().rt_selftest_fastrcp(device, C.byref(n), C.byref(bad), C.byref(ex)))
    return n.value, bad.value, ex.value


def probe_boxpair_certified(boxes, rays, max_dist, device=0):
    """rt_probe_boxpair_certified: the default hot loop's box pair next to the verbatim box tests, (n, 8) int32."""
    n = len(boxes)
    out = np.zeros((n, 8), np.int32)
    check(lib().rt_probe_boxpair_certified(device, n, np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(rays, np.float32),
                                           np.ascontiguousarray(max_dist, np.float32), out))
    return out


def probe_boxpair_certified_fma(boxes, rays, max_dist, device=0):
    """rt_probe_boxpair_certified_fma: the same pair with the far parameters as one fma each, as the hot loop takes it, (n, 8) int32."""
    n = len(boxes)
    out = np.zeros((n, 8), np.int32)
    check(lib().rt_probe_boxpair_certified_fma(device, n, np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(rays, np.float32),
                                               np.ascontiguousarray(max_dist, np.float32), out))
    return out


def probe_boxpair_filtered(boxes, rays, max_dist, device=0):
    n = len(boxes)
    out = np.zeros((n, 8), np.int32)
    check(lib().rt_probe_boxpair_filtered(device, n, np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(rays, np.float32),
                                          np.ascontiguousarray(max_dist, np.float32), out))
    return out


def shading_normal_batch(tris, vn, rays, t):
    """rt_shading_normal_batch (host only): the smooth-shading rule on hit i of triangle record tris[i] (capi.QUAD_DT) with vertex normals vn[i], ray rays[i]
    (o, d) and hit distance t[i] -> (normal (n, 3) float32, interpolated (n,) uint32)"""
    tris = np.ascontiguousarray(tris, dtype=capi.QUAD_DT)
    vn, rays, t = normals_table(vn), np.ascontiguousarray(rays, np.float32).reshape(-1, 6), np.ascontiguousarray(t, np.float32)
    n = len(tris)
    assert len(vn) == n and len(rays) == n and len(t) == n
    normal, took = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    check(lib().rt_shading_normal_batch(n, tris.ctypes.data, vn.ctypes.data, rays, t, normal, took))
    return normal, took


def probe_shading_normal(world, table, rays, device=0):
    """rt_probe_shading_normal: the world's walk, then the smooth-shading rule on a triangle hit -> (hit int32, normal (n, 3), interpolated uint32)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
    n = len(rays)
    tab = normals_table(table) if table is not None else np.zeros((0, 9), np.float32)
    hit, normal, took = np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    check(lib().rt_probe_shading_normal(device, C.byref(world), tab.ctypes.data if len(tab) else None, len(tab), n, rays, hit, normal, took))
    return hit, normal, took


def tri_uv_batch(tris, uv, rays, t):
    """rt_tri_uv_batch (host only): the texture-coordinate rule on hit i of triangle record tris[i] (capi.QUAD_DT) with the record uv[i], ray rays[i] (o, d)
    and hit distance t[i] -> (n, 2) float32: (tu, tv) before the clamp"""
    tris = np.ascontiguousarray(tris, dtype=capi.QUAD_DT)
    uv, rays, t = uvs_table(uv), np.ascontiguousarray(rays, np.float32).reshape(-1, 6), np.ascontiguousarray(t, np.float32)
    n = len(tris)
    assert len(uv) == n and len(rays) == n and len(t) == n
    out = np.zeros((n, 2), np.float32)
    check(lib().rt_tri_uv_batch(n, tris.ctypes.data, uv.ctypes.data, rays, t, out))
    return out


def probe_tri_uv(world, table, rays, device=0):
    """rt_probe_tri_uv: the world's walk, then the texture-coordinate rule on a triangle hit -> (hit int32, uv (n, 2): before the clamp; planar on a parallelogram)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
    n = len(rays)
    tab = uvs_table(table) if table is not None else np.zeros((0, 6), np.float32)
    hit, uv = np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
    check(lib().rt_probe_tri_uv(device, C.byref(world), tab.ctypes.data if len(tab) else None, len(tab), n, rays, hit, uv))
    return hit, uv


def _texture_lookup(fn, table, index, u, v):
    records, texels = texture_table(table)
    index, u, v = np.ascontiguousarray(index, np.uint32).reshape(-1), np.ascontiguousarray(u, np.float32).reshape(-1), np.ascontiguousarray(v, np.float32).reshape(-1)
    if not (len(index) == len(u) == len(v)):
        raise ValueError("texture lookup: index, u and v must have one length")
    rgb = np.zeros((len(index), 3), np.float32)
    check(fn(records.ctypes.data if len(records) else None, len(records), texels.ctypes.data if len(texels) else None, index, u, v, len(index), rgb))
    return rgb


def texture_lookup_batch(table, index, u, v):
    """rt_texture_lookup_batch (host only): the texture rule — entry index[i] of `table` (as Renderer.textures takes it) at (u[i], v[i]) -> (n, 3) float32"""
    return _texture_lookup(lib().rt_texture_lookup_batch, table, index, u, v)


def probe_texture(table, index, u, v, device=0):
    """rt_probe_texture: texture_lookup_batch on the device, one lane per lookup"""
    return _texture_lookup(lambda *a: lib().rt_probe_texture(device, *a), table, index, u, v)


def _normal_map(fn, table, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength):
    records, texels = texture_table(table)
    surface, index = np.ascontiguousarray(surface, np.uint32).reshape(-1), np.ascontiguousarray(index, np.uint32).reshape(-1)
    n = len(surface)
    a, b, normal, ray_d = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (a, b, normal, ray_d))
    u, v, strength = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (u, v, strength))
    tri_uv = None if tri_uv is None else np.ascontiguousarray(tri_uv, np.float32).reshape(-1, 6)
    if not all(len(x) == n for x in (a, b, normal, ray_d, u, v, index, strength)) or (tri_uv is not None and len(tri_uv) != n):
        raise ValueError("normal map: every array must have one entry per case")
    out, path = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    check(fn(records.ctypes.data if len(records) else None, len(records), texels.ctypes.data if len(texels) else None, n, surface, a, b,
             None if tri_uv is None else tri_uv.ctypes.data, normal, ray_d, u, v, index, strength, out, path))
    return out, path


def normal_map_batch(table, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength):
    """rt_normal_map_batch (host only): the normal-map rule on n cases — per case its surface (capi.NMAP_SURFACE_*), a and b (a sphere's normal; a
    record's u and v; given tangents), tri_uv (n, 6) or None, the normal, the ray's direction, the lookup's (u, v), the entry of `table` (as Renderer.textures
    takes it) and the strength -> (normals (n, 3), path (n,) of capi.NMAP_*: replaced where path == capi.NMAP_REPLACED)"""
    return _normal_map(lib().rt_normal_map_batch, table, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength)


def probe_normal_map(table, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength, device=0):
    """rt_probe_normal_map: normal_map_batch on the device, one lane per case"""
    return _normal_map(lambda *args: lib().rt_probe_normal_map(device, *args), table, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength)


def _microfacet(fn, normal, ray_d, roughness, f0, coat, tapes):
    normal, ray_d, f0 = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (normal, ray_d, f0))
    roughness = np.ascontiguousarray(roughness, np.float32).reshape(-1)
    coat = np.ascontiguousarray(coat, np.uint32).reshape(-1)
    n = len(roughness)
    if not all(len(x) == n for x in (normal, ray_d, f0, coat, tapes)):
        raise ValueError("microfacet: every array must have one entry per case")
    lengths = np.array([len(t) for t in tapes], np.uint32)
    offsets = np.zeros((n, 2), np.uint32)
    offsets[:, 1] = lengths
    offsets[1:, 0] = np.cumsum(lengths, dtype=np.uint64)[:-1]
    tape = np.ascontiguousarray(np.concatenate([np.asarray(t, np.uint32) for t in tapes] + [np.array([0x800001], np.uint32)]), np.uint32)
    out_dir, weight, path, draws = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    check(fn(n, normal, ray_d, roughness, f0, coat, tape, len(tape), offsets, out_dir, weight, path, draws))
    return out_dir, weight, path, draws


def microfacet_batch(normal, ray_d, roughness, f0, coat, tapes):
    """rt_microfacet_batch (host only): the microfacet rule on n cases — per case the normal, the ray's direction, the roughness, F0 (n, 3; a coat
    reads its first component), coat != 0 for a coat, and tapes[i] = its uniforms as words k in [1, 2^24] (u = k 2^-24) -> (directions (n, 3), weights (n, 3),
    path (n,) of capi.MFAC_*, uniforms consumed (n,))"""
    return _microfacet(lib().rt_microfacet_batch, normal, ray_d, roughness, f0, coat, tapes)


def probe_microfacet(normal, ray_d, roughness, f0, coat, tapes, device=0):
    """rt_probe_microfacet: microfacet_batch on the device, one lane per case"""
    return _microfacet(lambda *args: lib().rt_probe_microfacet(device, *args), normal, ray_d, roughness, f0, coat, tapes)


def _interior(fn, Ng, n, ray_d, t, ior, sigma, sphere):
    Ng, n, ray_d, sigma = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (Ng, n, ray_d, sigma))
    t, ior = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (t, ior))
    sphere = np.ascontiguousarray(sphere, np.uint32).reshape(-1)
    k = len(t)
    if not all(len(x) == k for x in (Ng, n, ray_d, sigma, ior, sphere)):
        raise ValueError("interior: every array must have one entry per case")
    back, eta, T = np.zeros(k, np.uint32), np.zeros(k, np.float32), np.zeros((k, 3), np.float32)
    check(fn(k, Ng, n, ray_d, t, ior, sigma, sphere, back, eta, T))
    return back, eta, T


def interior_batch(Ng, n, ray_d, t, ior, sigma, sphere):
    """rt_interior_batch (host only): the solid-glass rule on k cases — per case the stored normal Ng, the shading normal n (a sphere's outward
    normal), the ray's direction, the hit's parameter t, the index of refraction, sigma (k, 3) and sphere != 0 for a hit on a sphere -> (back (k,) 0 / 1,
    eta (k,), T (k, 3))"""
    return _interior(lib().rt_interior_batch, Ng, n, ray_d, t, ior, sigma, sphere)


def probe_interior(Ng, n, ray_d, t, ior, sigma, sphere, device=0):
    """rt_probe_interior: interior_batch on the device, one lane per case"""
    return _interior(lambda *args: lib().rt_probe_interior(device, *args), Ng, n, ray_d, t, ior, sigma, sphere)


def _expf(fn, x):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros(len(x), np.float32)
    check(fn(len(x), x, out))
    return out


def expf_batch(x):
    """rt_expf_batch (host only): rt_expf of every x, the library's own exponential (rt_math.hpp)"""
    return _expf(lib().rt_expf_batch, x)


def probe_expf(x, device=0):
    """rt_probe_expf: expf_batch on the device, one lane per value"""
    return _expf(lambda *args: lib().rt_probe_expf(device, *args), x)


def _cutout(fn, table, quads, uv, rays, t, records, material):
    tex, texels = texture_table(table)
    quads = np.ascontiguousarray(quads, capi.QUAD_DT).reshape(-1)
    rays, t = np.ascontiguousarray(rays, np.float32).reshape(-1, 6), np.ascontiguousarray(t, np.float32).reshape(-1)
    records, material = np.ascontiguousarray(records, capi.CUTOUT_DT).reshape(-1), np.ascontiguousarray(material, np.uint32).reshape(-1)
    k = len(t)
    if uv is not None:
        uv = np.ascontiguousarray(np.asarray(uv, np.float32).reshape(-1, 6))
    if not (len(quads) == len(rays) == len(material) == k and (uv is None or len(uv) == k)):
        raise ValueError("cutout: every array must have one entry per case")
    keep, out_uv, value = np.zeros(k, np.uint32), np.zeros((k, 2), np.float32), np.zeros(k, np.float32)
    check(fn(tex.ctypes.data if len(tex) else None, len(tex), texels.ctypes.data if len(texels) else None, k, quads.ctypes.data if k else None,
             uv.ctypes.data if uv is not None and k else None, rays, t, records.ctypes.data if len(records) else None, len(records), material, keep, out_uv, value))
    return keep, out_uv, value


def cutout_batch(table, quads, uv, rays, t, records, material):
    """rt_cutout_batch (host only): the cutout rule on k cases — `table` as Renderer.textures takes it; per case the surface quads[i]
    (capi.QUAD_DT), its texture coordinates uv[i] ((k, 3, 2); None: the planar coordinates for every case), the ray rays[i] (o, d), the candidate's t[i] and
    material[i], an index into `records` (capi.CUTOUT_DT) -> (keep (k,) 0 / 1, uv (k, 2), value (k,): the mask's green; zeros where the record is off)"""
    return _cutout(lib().rt_cutout_batch, table, quads, uv, rays, t, records, material)


def probe_cutout(table, quads, uv, rays, t, records, material, device=0):
    """rt_probe_cutout: cutout_batch on the device, one lane per case"""
    return _cutout(lambda *args: lib().rt_probe_cutout(device, *args), table, quads, uv, rays, t, records, material)


def _rough_glass(fn, normal, ray_d, roughness, ior, tapes):
    normal, ray_d = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (normal, ray_d))
    roughness, ior = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (roughness, ior))
    n = len(roughness)
    if not all(len(x) == n for x in (normal, ray_d, ior, tapes)):
        raise ValueError("rough glass: every array must have one entry per case")
    offsets = np.zeros((n, 2), np.uint32)
    if isinstance(tapes, np.ndarray) and tapes.ndim == 2:   # tapes of one length, as one array: a million cases need no million arrays
        offsets[:, 1] = tapes.shape[1]
        offsets[:, 0] = np.arange(n, dtype=np.uint64) * tapes.shape[1]
        words = [np.ascontiguousarray(tapes, np.uint32).reshape(-1)]
    else:
        lengths = np.array([len(t) for t in tapes], np.uint32)
        offsets[:, 1] = lengths
        offsets[1:, 0] = np.cumsum(lengths, dtype=np.uint64)[:-1]
        words = [np.asarray(t, np.uint32) for t in tapes]
    tape = np.ascontiguousarray(np.concatenate(words + [np.array([0x800001], np.uint32)]), np.uint32)
    out_dir, weight, path, draws = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    check(fn(n, normal, ray_d, roughness, ior, tape, len(tape), offsets, out_dir, weight, path, draws))
    return out_dir, weight, path, draws


def rough_glass_batch(normal, ray_d, roughness, ior, tapes):
    """rt_rough_glass_batch (host only): the rough-glass rule on n cases — per case the normal, the ray's direction, the roughness, the index of
    refraction, and tapes[i] = its uniforms as words k in [1, 2^24] (a list of arrays, or one (n, L) array) -> (directions (n, 3), weights (n,), path (n,) of
    capi.MFAC_*, uniforms consumed (n,))"""
    return _rough_glass(lib().rt_rough_glass_batch, normal, ray_d, roughness, ior, tapes)


def probe_rough_glass(normal, ray_d, roughness, ior, tapes, device=0):
    """rt_probe_rough_glass: rough_glass_batch on the device, one lane per case"""
    return _rough_glass(lambda *args: lib().rt_probe_rough_glass(device, *args), normal, ray_d, roughness, ior, tapes)


def _noise_value(fn, world, albedo, scale, points):
    perlin = world.perlin if hasattr(world, "perlin") else world   # a world (rt_world_flat) or the address of its rt_perlin
    if not perlin:
        raise ValueError("noise value: the world has no Perlin tables (Scene.set_perlin)")
    albedo, points = np.ascontiguousarray(albedo, np.float32).reshape(3), np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rgb = np.zeros((len(points), 3), np.float32)
    if len(points):
        check(fn(perlin, albedo.ctypes.data, float(scale), points.ctypes.data, len(points), rgb.ctypes.data))
    return rgb


def noise_value_batch(world, albedo, scale, points):
    """rt_noise_value_batch (host only): the marble of RT_MAT_LAMBERTIAN_NOISE — the world's Perlin tables, the material's albedo and param
    (`scale`) at points (n, 3) -> (n, 3) float32"""
    return _noise_value(lib().rt_noise_value_batch, world, albedo, scale, points)


def probe_noise_value(world, albedo, scale, points, device=0):
    """rt_probe_noise_value: noise_value_batch on the device, one lane per point"""
    return _noise_value(lambda *a: lib().rt_probe_noise_value(device, *a), world, albedo, scale, points)


def environment_batch(image, u0, dirs):
    """rt_environment_batch (host only): the environment rule on directions (n, 3) -> (rgb (n, 3) float32, texel (n,) uint32 = j * W + i)"""
    img = _env_image(image)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(dirs)
    rgb, texel = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    check(lib().rt_environment_batch(n, img.shape[1], img.shape[0], img.ctypes.data, float(u0), dirs, rgb, texel))
    return rgb, texel


def probe_environment(image, u0, dirs, device=0):
    """rt_probe_environment: environment_batch on the device, one lane per direction"""
    img = _env_image(image)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(dirs)
    rgb, texel = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    check(lib().rt_probe_environment(device, n, img.shape[1], img.shape[0], img.ctypes.data, float(u0), dirs, rgb, texel))
    return rgb, texel


def environment_distribution(image):
    """rt_environment_distribution (host only): the sampling distribution of an environment map, image (H, W, 3) ->
    {'rowc' (H,), 'rowy' (H + 1,), 'colc' (H, W), 'density' (H, W)} float32; RtError for an all-black map"""
    img = _env_image(image)
    h, w = img.shape[:2]
    rowc, rowy, colc, density = np.zeros(h, np.float32), np.zeros(h + 1, np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    check(lib().rt_environment_distribution(w, h, img.ctypes.data, rowc, rowy, colc.reshape(-1), density.reshape(-1)))
    return {"rowc": rowc, "rowy": rowy, "colc": colc, "density": density}


def _env_uniforms(uniforms):
    return np.ascontiguousarray(uniforms, np.float32).reshape(-1, 4)


def environment_sample_batch(image, u0, uniforms):
    """rt_environment_sample_batch (host only): the sampling rule on uniforms (n, 4) = (x1, x2, a, b) in (0, 1] ->
    (directions (n, 3) float32, drawn texel (n,) uint32 = j * W + i, density of the direction (n,) float32)"""
    img, u = _env_image(image), _env_uniforms(uniforms)
    n = len(u)
    d, texel, density = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    check(lib().rt_environment_sample_batch(n, img.shape[1], img.shape[0], img.ctypes.data, float(u0), u.reshape(-1), d.reshape(-1), texel, density))
    return d, texel, density


def probe_environment_sample(image, u0, uniforms, device=0):
    """rt_probe_environment_sample: environment_sample_batch on the device, one lane per quadruple"""
    img, u = _env_image(image), _env_uniforms(uniforms)
    n = len(u)
    d, texel, density = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    check(lib().rt_probe_environment_sample(device, n, img.shape[1], img.shape[0], img.ctypes.data, float(u0), u.reshape(-1), d.reshape(-1), texel, density))
    return d, texel, density
