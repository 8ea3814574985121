"""A numpy float32 twin of the feature sums in both modes — test infrastructure only.

Per (pixel, sample): the pinhole primary ray as _tex_twin.first_hit_frame builds it, the first hit by _tri_twin.closest_intersection (a world that twin does not
walk — a bvh_node tree, the queue or the 4-wide walk — is traced by the oracle's orc_trace_batch, as tests/test_gpu_aov.py does), then what a hit adds: the
trace's normal (with `vn`: _smooth_twin's shading normal on a triangle), t, 1 and the first-hit albedo —
  Lambertian, metal: the material's; checker: checker_value restated here; dielectric, light, and a miss: (1, 1, 1)      [aov_albedo]
  image (mode RT_AOV_TEXTURED): _tex_twin.hit_uv — the sphere map of the OUTWARD normal, the planar coordinates, rt_tri_uvs' rule under `uv` — then
    _tex_twin.lookup in `table`, or, without a table, _uv_twin.texel of the world's `image`
  noise (mode RT_AOV_TEXTURED): `noise(albedo, scale, points)` at the fp32 hit point o + d * t — the product's host batch (api.noise_value_batch), which is
    pinned to the CPU oracle by tests/test_aov_textured_cpu.py; nobody restates the library's sine in numpy
The sums are fp32, added in sample order; a miss adds its albedo only.  In mode RT_AOV_PLAIN a hit on a noise or image material is an error, as the enable is.
"""
import ctypes as C

import numpy as np

import _path_twin as PT
import _smooth_twin as ST
import _tex_twin as XT
import _tri_twin as TT
import _uv_twin as UT
from _nee2_twin import world_arrays
from _nee_twin import F, PRIM_MOVING, oracle_trace

MAT_LAMBERTIAN, MAT_METAL, MAT_CHECKER, MAT_NOISE, MAT_IMAGE = 0, 1, 3, 6, 7


def twin_table(textures):
    """Scene.textures() = (records, texels) -> the table as _tex_twin.lookup takes it: [(image [H][W][3] uint8, wrap, filter)]; an empty entry is a 1 x 1 image
    nobody may name"""
    if textures is None:
        return None
    records, texels = textures
    texels = np.asarray(texels, np.uint8).reshape(-1, 3)
    out = []
    for r in records:
        w, h, first = int(r["width"]), int(r["height"]), int(r["first"])
        out.append((texels[first:first + w * h].reshape(h, w, 3) if w else np.zeros((1, 1, 3), np.uint8), int(r["wrap"]), int(r["filter"])))
    return out


def world_image(world_flat):
    """the world's own image (rt_scene_set_image) of a product rt_world_flat as uint8 [H][W][3], or None"""
    if not world_flat.image:
        return None
    n = world_flat.image_width * world_flat.image_height * 3
    return np.frombuffer((C.c_char * n).from_address(world_flat.image), np.uint8).reshape(world_flat.image_height, world_flat.image_width, 3).copy()


def primary_rays(cam, width, height, spp, seed, first_sample=0):
    """rays (width * height * spp, 7) float32 of samples [first_sample, first_sample + spp) of every pixel, pixel-major: jitter, then the pinhole ray"""
    _, ray_o, ray_d = PT.primary_rays(cam, width, height, seed, *PT.keys(width, height, spp, first_sample))
    rays = np.zeros((len(ray_o), 7), F)
    rays[:, 0:3], rays[:, 3:6] = ray_o, ray_d
    return rays


def first_hits(world, rays, trace=TT.closest_intersection):
    """(hit, t, prim, normal) of the world's own walk: `trace` where _tri_twin walks the world, the oracle's elsewhere"""
    if world.kind in (0, 1) and world.traversal == 0:
        return trace(world, rays)
    return oracle_trace(world, np.ascontiguousarray(rays, F))


def checker_value(even, odd, inv_scale, pos):
    """checker_texture::value as the kernels compute it: ivec3 truncates toward zero, the sum of the three decides"""
    with np.errstate(all="ignore"):
        sp = (pos * inv_scale[:, None]).astype(F)
        cell = np.trunc(sp).astype(np.int64).sum(axis=1)
    return np.where((cell % 2 == 0)[:, None], even, odd).astype(F)


def albedo_of_hits(world, rays, hit, t, prim, normal, textured, uv=None, table=None, image=None, noise=None):
    """the first-hit albedo of every ray (n, 3) float32; a miss is (1, 1, 1)"""
    prims, quads, mats = world_arrays(world)
    n = len(rays)
    alb = np.ones((n, 3), F)
    h = np.nonzero(hit != 0)[0]
    on_sphere = prim[h] < len(prims)
    mat = np.zeros(len(h), np.int64)
    mat[on_sphere] = prims["mat"][prim[h][on_sphere]] & ~np.uint32(PRIM_MOVING)   # a moving sphere's material; where it stood at the ray's time is the walk's to know
    mat[~on_sphere] = quads["mat"][prim[h][~on_sphere] - len(prims)]
    mtype = mats["type"][mat]
    with np.errstate(all="ignore"):
        pos = (rays[h, 0:3] + rays[h, 3:6] * t[h][:, None]).astype(F)   # Ray::at, each operation rounded on its own
    plain = (mtype == MAT_LAMBERTIAN) | (mtype == MAT_METAL)
    alb[h[plain]] = mats["albedo"][mat[plain]]
    chk = mtype == MAT_CHECKER
    if chk.any():
        m = mats[mat[chk]]
        alb[h[chk]] = checker_value(m["albedo"].astype(F), m["albedo2"].astype(F), m["param"].astype(F), pos[chk])
    tex = (mtype == MAT_NOISE) | (mtype == MAT_IMAGE)
    assert textured or not tex.any(), "mode RT_AOV_PLAIN refuses a world with a noise or an image texture"
    for k in np.unique(mat[mtype == MAT_NOISE]):
        rows = mat == k
        alb[h[rows]] = noise(mats["albedo"][k], float(mats["param"][k]), pos[rows])
    img = mtype == MAT_IMAGE
    if img.any():
        tuv = XT.hit_uv(world, uv, rays, hit, t, prim, normal)[h][img]
        if table is not None:
            alb[h[img]] = XT.lookup(table, mats["albedo2"][mat[img]][:, 0].astype(np.int64), tuv[:, 0], tuv[:, 1])
        else:
            assert (mats["albedo2"][mat[img]][:, 0] == 0).all(), "without a table an image material names image 0"
            alb[h[img]] = UT.texel(image, tuv[:, 0], tuv[:, 1])
    return alb


def sums(world, cam, width, height, spp, seed, textured, uv=None, table=None, image=None, noise=None, vn=None, first_sample=0, start=None,
         trace=TT.closest_intersection):
    """(H, W, 8) float32: (sum Nx, sum Ny, sum Nz, sum t, sum Ar, sum Ag, sum Ab, hits) of samples [first_sample, first_sample + spp), continued from `start`;
    also the fraction of rays that hit"""
    rays = primary_rays(cam, width, height, spp, seed, first_sample)
    hit, t, prim, normal = first_hits(world, rays, trace)
    alb = albedo_of_hits(world, rays, hit, t, prim, normal, textured, uv, table, image, noise)
    if vn is not None:   # the smooth form changes the normal sum only
        prims, quads, _ = world_arrays(world)
        first_tri = len(prims) + int((quads["kind"] == 0).sum())
        rows = np.nonzero((hit != 0) & (prim >= first_tri))[0]
        if len(rows):
            normal = normal.copy()
            normal[rows] = ST.shading_normal(quads[prim[rows] - len(prims)], ST.table(vn)[prim[rows] - first_tri], rays[rows, 0:3], rays[rows, 3:6], t[rows])[0]
    n = len(rays)
    h = hit != 0
    contrib = np.zeros((n, 8), F)
    contrib[h, 0:3], contrib[h, 3], contrib[h, 7] = normal[h], t[h], F(1)
    contrib[:, 4:7] = alb
    contrib = contrib.reshape(width * height, spp, 8)
    acc = np.zeros((width * height, 8), F) if start is None else np.asarray(start, F).reshape(width * height, 8).copy()
    for s in range(spp):   # in sample order; a miss adds zeros to normal, depth and hits (x + 0 keeps x's bits: no sum is -0)
        acc = (acc + contrib[:, s]).astype(F)
    return acc.reshape(height, width, 8), float(h.mean())
