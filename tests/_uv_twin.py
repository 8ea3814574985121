"""A numpy float32 twin of the texture-coordinate rule — test infrastructure only.

tri_uv() restates the rule of include/rt06.h (rt_tri_uvs) in float32 numpy, every operation rounded on its own: image_value_quad's planar coordinates, then
tu = (t0.u * ((1 - alpha) - beta) + t1.u * alpha) + t2.u * beta and tv likewise.  texel() restates image_texel (clamp, flip v, nearest texel, 1/255).
tri_uv64() is the same mathematics in float64, for the property no kernel shares: coordinates that are an affine function of position interpolate to that
function of the hit point.  first_hit_frame() is the whole of a depth-2 sample in an open world whose only surfaces are image-textured triangles: the first
hit's texel times the background, or 0 for a failed scatter; it refuses (returns undecided rows) anything else.
"""
import numpy as np

import _tri_twin as TT
from _nee2_twin import world_arrays
from _nee_twin import F, _Tape, cross, dot, near_zero

IDENTITY = np.array([[0, 0], [1, 0], [0, 1]], F)
MAT_IMAGE = 7
in_order_sums, resolve = TT.in_order_sums, TT.resolve


def table(uv):
    """a table of texture coordinates as float32 (n, 3, 2): t0, t1, t2 of every triangle"""
    a = np.asarray(uv)
    if a.dtype.names:
        a = np.stack([a["t0"], a["t1"], a["t2"]], axis=1)
    return np.ascontiguousarray(a, F).reshape(-1, 3, 2)


def planar(tris, o, d, t):
    """image_value_quad's three lines on hit i of record tris[i]: (alpha, beta) float32"""
    o, d, t = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3), np.ascontiguousarray(t, F).reshape(-1)
    with np.errstate(all="ignore"):
        hit_p = o + d * t[:, None]
        u, v, w = tris["u"].astype(F), tris["v"].astype(F), tris["w"].astype(F)
        pl = hit_p - tris["Q"].astype(F)
        return dot(w, cross(pl, v)), dot(w, cross(u, pl))


def tri_uv(tris, uv, o, d, t):
    """The rule on hit i: triangle record tris[i] (Q, u, v, w), texture coordinates uv[i] (3, 2), ray (o[i], d[i]), distance t[i] -> (n, 2) float32, before the clamp"""
    uv = table(uv)
    alpha, beta = planar(tris, o, d, t)
    with np.errstate(all="ignore"):
        gamma = (F(1) - alpha) - beta
        tu = (uv[:, 0, 0] * gamma + uv[:, 1, 0] * alpha) + uv[:, 2, 0] * beta
        tv = (uv[:, 0, 1] * gamma + uv[:, 1, 1] * alpha) + uv[:, 2, 1] * beta
    return np.stack([tu, tv], axis=1).astype(F)


def texel_index(width, height, u, v):
    """image_texel's choice: (column, row) of the texel (u, v) selects"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        u = np.where(u < F(0), F(0), np.where(u > F(1), F(1), u)).astype(F)
        v = np.where(v < F(0), F(0), np.where(v > F(1), F(1), v)).astype(F)
        v = F(1) - v
        i = np.trunc(u * F(width)).astype(np.int64)
        j = np.trunc(v * F(height)).astype(np.int64)
    return np.minimum(i, width - 1), np.minimum(j, height - 1)


def texel(image, u, v):
    """image_texel: the albedo (n, 3) float32 the image [H][W][3] uint8 gives at (u, v)"""
    image = np.asarray(image, np.uint8)
    i, j = texel_index(image.shape[1], image.shape[0], u, v)
    return image[j, i].astype(F) * F(float.fromhex("0x1.010102p-8"))


def tri_uv64(Q, u, v, t0, t1, t2, hit_p):
    """the rule in float64 (w from u, v): (n, 2)"""
    Q, u, v, t0, t1, t2, hit_p = (np.asarray(a, np.float64) for a in (Q, u, v, t0, t1, t2, hit_p))
    n = np.cross(u, v)
    w = n / (n * n).sum(axis=-1, keepdims=True)
    pl = hit_p - Q
    alpha = (w * np.cross(pl, v)).sum(axis=-1)
    beta = (w * np.cross(u, pl)).sum(axis=-1)
    return t0 * (1 - alpha - beta)[..., None] + t1 * alpha[..., None] + t2 * beta[..., None]


def closest_intersection_uv(world, uv, rays):
    """_tri_twin.closest_intersection, then per hit the texture coordinates before the clamp: the rule on a triangle (uv = None: every record the identity's planar
    lookup), the planar coordinates on a parallelogram, 0 elsewhere -> (hit, t, prim, (n, 2) float32)"""
    hit, t, prim, _ = TT.closest_intersection(world, rays)
    prims, quads, _ = world_arrays(world)
    first_tri = len(prims) + int((quads["kind"] == 0).sum())
    out = np.zeros((len(rays), 2), F)
    rows = np.nonzero((hit != 0) & (prim >= len(prims)))[0]
    if len(rows):
        q = quads[prim[rows] - len(prims)]
        a, b = planar(q, rays[rows, 0:3], rays[rows, 3:6], t[rows])
        out[rows] = np.stack([a, b], axis=1)
        if uv is not None:
            tab = table(uv)
            assert len(tab) == len(prims) + len(quads) - first_tri, "one record per triangle of the flat world"
            tr = prim[rows] >= first_tri
            out[rows[tr]] = tri_uv(q[tr], tab[prim[rows[tr]] - first_tri], rays[rows[tr], 0:3], rays[rows[tr], 3:6], t[rows[tr]])
    return hit, t, prim, out


def first_hit_frame(world, uv, image, cam, width, height, spp, seed):
    """Every sample of a depth-2 frame of an open world under a constant background whose surfaces are image-textured triangles: a primary miss is the background,
    a hit scatters as a Lambertian does (one on_unit3 draw; near-zero = a failed scatter = 0) and the scattered ray misses: texel * background — or meets such
    a triangle again and ends at the depth limit with nothing accumulated: 0.
    Returns (samples (H, W, spp, 3) float32, decided (H, W, spp) bool) — a sample that meets anything else is undecided."""
    assert cam.type == 0 and world.background == 1
    prims, quads, mats = world_arrays(world)
    first_tri = len(prims) + int((quads["kind"] == 0).sum())
    tab = table(uv)
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
        on_image_triangle = (prim[h] >= first_tri) & (mats["type"][quads["mat"][np.maximum(prim[h] - len(prims), 0)]] == MAT_IMAGE)
        decided[h[~on_image_triangle]] = False
        h = h[on_image_triangle]
        q = quads[prim[h] - len(prims)]
        o, d = rays[h, 0:3], rays[h, 3:6]
        hit_p = o + d * t[h][:, None]
        new_d = normal[h] + tape.on_unit3(h)
        ok = ~near_zero(new_d)
        tuv = tri_uv(q, tab[prim[h] - first_tri], o, d, t[h])
        albedo = texel(image, tuv[:, 0], tuv[:, 1])
        out[h[~ok]] = 0
        h, new_d, hit_p, albedo = h[ok], new_d[ok], hit_p[ok], albedo[ok]
        second = np.zeros((len(h), 7), F)
        second[:, 0:3], second[:, 3:6] = hit_p + new_d * F(0.001), new_d
        hit2, _, prim2, _ = TT.closest_intersection(world, second)
        again = (hit2 != 0) & (prim2 >= first_tri) & (mats["type"][quads["mat"][np.maximum(prim2 - len(prims), 0)]] == MAT_IMAGE)
        decided[h[(hit2 != 0) & ~again]] = False   # anything but another image-textured triangle: not this twin's to say
        atten = np.ones((len(h), 3), F) * albedo
        out[h] = atten * sky + np.zeros(3, F)
        out[h[again]] = 0   # a grazing scatter that meets the plane again ends at the depth limit, having met no light: nothing accumulated
    return out.reshape(height, width, spp, 3), decided.reshape(height, width, spp)
