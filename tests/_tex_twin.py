"""A numpy float32 twin of the texture table's rule — test infrastructure only.

value() restates texture_value of include/rt06.h (rt_scene_add_image) in float32 numpy, every operation rounded on its own: wrap (REPEAT: x - floor x; then
!(x > 0) ? 0 : (x > 1 ? 1 : x), so a coordinate that is not a number is 0: column 0 and, after the flip, the bottom row), flip v, then the nearest texel or the
bilinear lerp(lerp(c00, c10, fx), lerp(c01, c11, fx), fy) with lerp(a, b, t) = a + (b - a) * t.  value64() is the same formula in float64.  first_hit_frame() is
the whole of a depth-2 sample in an open world under a constant background whose only surfaces are image-textured spheres, parallelograms and triangles, each on
an image of the table; it counts the samples that take the REPEAT and the bilinear-border branches.
"""
import numpy as np

import _env_twin as ET
import _tri_twin as TT
import _uv_twin as UT
from _nee2_twin import world_arrays
from _nee_twin import F, _Tape, near_zero

CLAMP, REPEAT = 0, 1
NEAREST, BILINEAR = 0, 1
MODES = [(CLAMP, NEAREST), (CLAMP, BILINEAR), (REPEAT, NEAREST), (REPEAT, BILINEAR)]
SCALE = F(float.fromhex("0x1.010102p-8"))
MAT_IMAGE = 7
MAT_LIGHT = 4
in_order_sums, resolve = TT.in_order_sums, TT.resolve


def wrap_coord(x, wrap):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        if wrap == REPEAT:
            x = (x - np.floor(x)).astype(F)
        return np.where(~(x > F(0)), F(0), np.where(x > F(1), F(1), x)).astype(F)


def _lerp(a, b, t):
    return (a + (b - a) * t).astype(F)


def value(image, wrap, filt, u, v, stats=None):
    """the rule: image [H][W][3] uint8 under (wrap, filt) at (u, v) -> (n, 3) float32.  stats: a dict whose 'repeat' (a coordinate outside [0, 1] wrapped) and
    'border' (a bilinear column or row clamped or wrapped) counts grow"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[0], image.shape[1]
    u0, v0 = np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    with np.errstate(all="ignore"):
        u, v = wrap_coord(u0, wrap), wrap_coord(v0, wrap)
        if stats is not None and wrap == REPEAT:
            stats["repeat"] = stats.get("repeat", 0) + int(((u0 < 0) | (u0 > 1) | (v0 < 0) | (v0 > 1)).sum())
        v = F(1) - v
        if filt == NEAREST:
            i = np.minimum((u * F(W)).astype(np.int64), W - 1)
            j = np.minimum((v * F(H)).astype(np.int64), H - 1)
            return image[j, i].astype(F) * SCALE
        x, y = u * F(W) - F(0.5), v * F(H) - F(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0).astype(F), (y - y0).astype(F)
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        i1, j1 = i0 + 1, j0 + 1
        if stats is not None:
            stats["border"] = stats.get("border", 0) + int(((i0 < 0) | (i1 > W - 1) | (j0 < 0) | (j1 > H - 1)).sum())
        lo_x, hi_x, lo_y, hi_y = (W - 1, 0, H - 1, 0) if wrap == REPEAT else (0, W - 1, 0, H - 1)
        i0, i1 = np.where(i0 < 0, lo_x, i0), np.where(i1 > W - 1, hi_x, i1)
        j0, j1 = np.where(j0 < 0, lo_y, j0), np.where(j1 > H - 1, hi_y, j1)
        c = lambda j, i: image[j, i].astype(F) * SCALE   # noqa: E731
        top = _lerp(c(j0, i0), c(j0, i1), fx[:, None])
        bottom = _lerp(c(j1, i0), c(j1, i1), fx[:, None])
        return _lerp(top, bottom, fy[:, None])


def value64(image, wrap, u, v):
    """the bilinear formula in float64 on coordinates that are numbers"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[0], image.shape[1]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if wrap == REPEAT:
        u, v = u - np.floor(u), v - np.floor(v)
    u, v = np.clip(u, 0, 1), 1 - np.clip(v, 0, 1)
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    i1, j1 = i0 + 1, j0 + 1
    if wrap == REPEAT:
        i0, i1, j0, j1 = i0 % W, i1 % W, j0 % H, j1 % H
    else:
        i0, i1, j0, j1 = np.clip(i0, 0, W - 1), np.clip(i1, 0, W - 1), np.clip(j0, 0, H - 1), np.clip(j1, 0, H - 1)
    c = lambda j, i: image[j, i].astype(np.float64) / 255.0   # noqa: E731
    top = c(j0, i0) + (c(j0, i1) - c(j0, i0)) * fx
    bottom = c(j1, i0) + (c(j1, i1) - c(j1, i0)) * fx
    return top + (bottom - top) * fy


def lookup(table, index, u, v, stats=None):
    """the rule over a table [(image, wrap, filt), ...]: entry index[i] at (u[i], v[i]) -> (n, 3) float32"""
    index = np.asarray(index).reshape(-1)
    u, v = np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    out = np.zeros((len(index), 3), F)
    for k, (image, wrap, filt) in enumerate(table):
        rows = np.nonzero(index == k)[0]
        if len(rows):
            out[rows] = value(image, wrap, filt, u[rows], v[rows], stats)
    return out


def sphere_uv(normal):
    """image_value's coordinates of an outward unit normal (n, 3): (u, v) float32"""
    n = np.ascontiguousarray(normal, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        cy = -n[:, 1]
        cy = np.where(cy < F(-1), F(-1), np.where(cy > F(1), F(1), cy)).astype(F)
        theta = ET._math(2, cy)
        phi = ET._math(3, -n[:, 2], n[:, 0]) + ET.PI
        return (phi / ET.TWO_PI).astype(F), (theta / ET.PI).astype(F)


def hit_uv(world, uv, rays, hit, t, prim, normal):
    """(u, v) before any clamp of every hit: the sphere map, the planar coordinates, or the rule of rt_tri_uvs on a triangle (uv: the scene's table or None)"""
    prims, quads, _ = world_arrays(world)
    first_tri = len(prims) + int((quads["kind"] == 0).sum())
    out = np.zeros((len(rays), 2), F)
    sph = np.nonzero((hit != 0) & (prim < len(prims)))[0]
    if len(sph):
        su, sv = sphere_uv(normal[sph])
        out[sph] = np.stack([su, sv], axis=1)
    rows = np.nonzero((hit != 0) & (prim >= len(prims)))[0]
    if len(rows):
        q = quads[prim[rows] - len(prims)]
        a, b = UT.planar(q, rays[rows, 0:3], rays[rows, 3:6], t[rows])
        out[rows] = np.stack([a, b], axis=1)
        if uv is not None and len(uv):
            tab = UT.table(uv)
            tr = prim[rows] >= first_tri
            out[rows[tr]] = UT.tri_uv(q[tr], tab[prim[rows[tr]] - first_tri], rays[rows[tr], 0:3], rays[rows[tr], 3:6], t[rows[tr]])
    return out


def prefer_walk_uv(tuv, walk, sel):
    """The kernels' order on a mapped hit: (u, v) is computed once, from the normal the walk found, BEFORE the normal map replaces that normal, and
    the image lookup and the roughness map of the hit take that same (u, v).  walk: the dict _nmap_twin.mapped_walk leaves its (u, v) in — walk["uv"] = (given
    (k,) bool, uv (k, 2), on a sphere (k,) bool) over the k rays of its last call, or None — or None for a run without a normal-map table; sel: the rows of
    those rays that tuv = hit_uv(...) stands for.  Returns (tuv with the walk's (u, v) on the rows it gave one for, (len(sel),) bool: such a row on a sphere —
    the one surface whose hit_uv reads the normal).  walk["after_map"] (a test's switch) keeps hit_uv's, the order the kernels do NOT have."""
    if not walk or walk.get("uv") is None or walk.get("after_map"):
        return tuv, np.zeros(len(sel), bool)
    given, uv, sphere = walk["uv"]
    return np.where(given[sel][:, None], uv[sel], tuv).astype(F), (given & sphere)[sel]


def count_walk_uv(walk, n):
    """walk's counter of the image and roughness lookups that took the walk's (u, v) on a sphere"""
    if walk is not None:
        walk["uv_lookups"] = walk.get("uv_lookups", 0) + int(n)


def first_hit_frame(world, uv, table, cam, width, height, spp, seed, stats=None):
    """Every sample of a depth-2 frame of an open world under a constant background whose surfaces are image-textured (a sphere, a parallelogram or a
    triangle; material.albedo2[0] = its image of `table`): a primary miss is the background; a hit scatters as a Lambertian does (one on_unit3 draw; near-zero = a
    failed scatter = 0) and the scattered ray misses: the rule's colour * background — or meets a surface again and ends at the depth limit: 0.
    Returns (samples (H, W, spp, 3) float32, decided (H, W, spp) bool): a sample whose first hit is on another material, or whose scattered ray meets a light, is
    undecided; stats as value() counts them, plus 'colours': the distinct looked-up colours."""
    assert cam.type == 0 and world.background == 1
    prims, quads, mats = world_arrays(world)
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), width * height)
    n = len(gids)
    tape = _Tape(seed, gids, smp)
    rows = np.arange(n)
    sky = np.array(list(world.background_color), F)
    with np.errstate(all="ignore"):
        x, y = (gids % np.uint32(width)).astype(F), (gids // np.uint32(width)).astype(F)
        psx, psy = F(1) / F(width), F(1) / F(height)
        ndcx = ((x + F(0.5)) * psx) * F(2) - F(1)
        ndcy = ((y + F(0.5)) * psy) * F(2) - F(1)
        jx, jy = tape.in_unit2(rows)
        sx, sy = ndcx + jx * psx, ndcy + jy * psy
        co, cu, cv, cw = (np.array(list(v), F) for v in (cam.o, cam.u, cam.v, cam.w))
        rays = np.zeros((n, 7), F)
        rays[:, 0:3] = co
        rays[:, 3:6] = (cw[None, :] + cu[None, :] * sx[:, None]) + cv[None, :] * sy[:, None]
        hit, t, prim, normal = TT.closest_intersection(world, rays)
        out = np.zeros((n, 3), F)
        decided = np.ones(n, bool)
        miss = hit == 0
        out[miss] = np.ones(3, F) * sky + np.zeros(3, F)
        h = np.nonzero(~miss)[0]
        mat = np.zeros(len(h), np.int64)
        on_sphere = prim[h] < len(prims)
        mat[on_sphere] = prims["mat"][prim[h][on_sphere]]
        mat[~on_sphere] = quads["mat"][prim[h][~on_sphere] - len(prims)]
        on_image = mats["type"][mat] == MAT_IMAGE
        decided[h[~on_image]] = False   # a first hit on anything but an image-textured surface: not this twin's to say
        index = np.where(on_image, mats["albedo2"][mat][:, 0], -1).astype(np.int64)   # (-1: no entry; such a sample's colour stays 0 and is undecided)
        tuv = hit_uv(world, uv, rays, hit, t, prim, normal)[h]
        albedo = lookup(table, index, tuv[:, 0], tuv[:, 1], stats)
        if stats is not None:
            stats["colours"] = len(np.unique(albedo, axis=0))
        o, d = rays[h, 0:3], rays[h, 3:6]
        hit_p = o + d * t[h][:, None]
        new_d = normal[h] + tape.on_unit3(h)
        ok = ~near_zero(new_d)
        out[h[~ok]] = 0
        h, new_d, hit_p, albedo = h[ok], new_d[ok], hit_p[ok], albedo[ok]
        second = np.zeros((len(h), 7), F)
        second[:, 0:3], second[:, 3:6] = hit_p + new_d * F(0.001), new_d
        hit2, _, prim2, _ = TT.closest_intersection(world, second)
        mat2 = np.where(prim2 < len(prims), prims["mat"][np.clip(prim2, 0, max(len(prims) - 1, 0))] if len(prims) else 0,
                        quads["mat"][np.clip(prim2 - len(prims), 0, max(len(quads) - 1, 0))] if len(quads) else 0)
        decided[h[(hit2 != 0) & (mats["type"][mat2] == MAT_LIGHT)]] = False   # a scatter that meets a light collects its emission: not this twin's to say
        atten = np.ones((len(h), 3), F) * albedo
        out[h] = atten * sky + np.zeros(3, F)
        out[h[hit2 != 0]] = 0   # a scatter that meets a surface again ends at the depth limit, having met no light: nothing accumulated
    return out.reshape(height, width, spp, 3), decided.reshape(height, width, spp)
