"""A numpy float32 twin of the smooth-shading rule — test infrastructure only.

shading_normal() restates the rule of include/rt06.h (rt_tri_normals) in float32 numpy, every operation rounded on its own: image_value_quad's planar
coordinates, g = (n0 * ((1 - alpha) - beta) + n1 * alpha) + n2 * beta, the two ways back to the flat normal.  closest_intersection_smooth() is
_tri_twin.closest_intersection followed by that on triangle hits.  radiance() for modes 0, 1, 2, 4 and 16 is _light_tree_twin's with that walk passed to it.
The oracle does not know the rule, so nothing here asks it about one; the twin is pinned before use (tests/test_smooth_normals_cpu.py): with a
table of zeros it IS _tri_twin, bit for bit, and rt_shading_normal_batch — the kernels' own function on the host — equals shading_normal() bit for bit.

Scope, as the twins have it: pinhole camera, static spheres, Lambertian, checker, metal and light materials, stack traversal.
"""
import numpy as np

import _light_tree_twin as LT
import _path_twin as PT
import _tri_twin as TT
from _nee2_twin import world_arrays
from _nee_twin import F, cross, dot

in_order_sums, resolve = TT.in_order_sums, TT.resolve
_flat_walk = TT.closest_intersection


def table(vn):
    """a table of vertex normals as float32 (n, 3, 3): n0, n1, n2 of every triangle"""
    a = np.asarray(vn)
    if a.dtype.names:
        a = np.stack([a["n0"], a["n1"], a["n2"]], axis=1)
    return np.ascontiguousarray(a, F).reshape(-1, 3, 3)


def shading_normal(tris, vn, o, d, t):
    """The rule on hit i: triangle record tris[i] (Q, u, v, normal, w), vertex normals vn[i] (3, 3), ray (o[i], d[i]), distance t[i].
    Returns (normal (n, 3) float32, interpolated (n,) bool, fallback (n,) int: 0 interpolated, 1 `!(l2 > 0)`, 2 `!(dot(ray.d, s) < 0)`)."""
    vn = table(vn)
    o, d, t = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3), np.ascontiguousarray(t, F).reshape(-1)
    with np.errstate(all="ignore"):
        nrm = tris["normal"].astype(F)
        f = np.where((dot(d, nrm) > F(0))[:, None], -nrm, nrm)
        hit_p = o + d * t[:, None]
        u, v, w = tris["u"].astype(F), tris["v"].astype(F), tris["w"].astype(F)
        planar = hit_p - tris["Q"].astype(F)
        alpha = dot(w, cross(planar, v))
        beta = dot(w, cross(u, planar))
        g = (vn[:, 0] * ((F(1) - alpha) - beta)[:, None] + vn[:, 1] * alpha[:, None]) + vn[:, 2] * beta[:, None]
        l2 = dot(g, g)
        has_dir = l2 > F(0)
        s = g / np.sqrt(l2)[:, None]
        s = np.where((dot(s, f) < F(0))[:, None], -s, s)
        faces = dot(d, s) < F(0)
        took = has_dir & faces
        fallback = np.where(~has_dir, 1, np.where(~faces, 2, 0))
        return np.where(took[:, None], s, f).astype(F), took, fallback


def closest_intersection_smooth(world, vn, rays, preset=None, info=None, base=None, **draws):
    """_tri_twin.closest_intersection, then the rule on the hits whose primitive is a triangle; vn: one record per triangle of the flat world.
    info (a dict): gets added up 'smooth' (hits on triangles with a non-zero record), 'interpolated' and 'fallback2' (of those), and 'fallback1' — every
    triangle hit that `!(l2 > 0)` sends back to the flat normal: all-zero records are the rule's own first case of it, and between three unit normals of one
    record g vanishes only on a set of measure zero, which no rendered frame meets.  base: the walk this one post-processes (default: _tri_twin's) —
    _cutout_twin.walk_of(...) for a world under a cutout table, whose rule runs in the leaf phase, before the normal of the hit the walk kept."""
    hit, t, prim, normal = (_flat_walk if base is None else base)(world, rays, preset, **draws)   # draws: the tape and its rows, for a world with a constant medium (_tri_twin)
    vn = table(vn)
    prims, quads, _ = world_arrays(world)
    first_tri = len(prims) + int((quads["kind"] == 0).sum())
    assert len(vn) == len(prims) + len(quads) - first_tri, "one record per triangle of the flat world"
    rows = np.nonzero((hit != 0) & (prim >= first_tri))[0]
    if len(rows):
        q = quads[prim[rows] - len(prims)]
        rec = vn[prim[rows] - first_tri]
        n, took, fb = shading_normal(q, rec, rays[rows, 0:3], rays[rows, 3:6], t[rows])
        normal = normal.copy()
        normal[rows] = n
        if info is not None:
            nonflat = (rec != 0).any(axis=(1, 2))
            for key, add in (("smooth", nonflat.sum()), ("interpolated", (took & nonflat).sum()), ("fallback1", (fb == 1).sum()), ("fallback2", ((fb == 2) & nonflat).sum())):
                info[key] = info.get(key, 0) + int(add)
    return hit, t, prim, normal


def smooth_walk(vn, info=None, base=None):
    """closest_intersection_smooth under the table vn as a walk (world, rays[, preset]) -> (hit, t, prim, normal), the way the whole-sample twins take one"""
    return lambda world, rays, preset=None, **draws: closest_intersection_smooth(world, vn, rays, preset, info, base, **draws)


def radiance(world, vn, cam, width, height, max_depth, seed, gids, samples, mode=0, info=None):
    """_light_tree_twin.radiance (modes 0, 1, 2, 4 and 16) over the smooth walk: ((n, 3) float32, followed (n,) bool)"""
    return LT.radiance(world, cam, width, height, max_depth, seed, gids, samples, mode, trace=smooth_walk(vn, info))


def frame_samples(world, vn, cam, width, height, spp, max_depth, seed, mode=0, first_sample=0, info=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, vn, cam, width, height, max_depth, seed, g, s, mode, info), width, height, spp, first_sample)


def first_hit_sums(world, vn, cam, width, height, spp, seed, first_sample=0):
    """_tri_twin.first_hit_sums with the rule applied to the first hits: (H, W, 5) float32 = (sum Nx, sum Ny, sum Nz, sum t, hits)"""
    return TT.first_hit_sums(world, cam, width, height, spp, seed, first_sample, trace=smooth_walk(vn))


def shading_normal64(Q, u, v, n0, n1, n2, d, hit_p):
    """the rule in float64 (w from u, v), for the mathematics no kernel shares: (normal, interpolated)"""
    Q, u, v, n0, n1, n2, d, hit_p = (np.asarray(a, np.float64) for a in (Q, u, v, n0, n1, n2, d, hit_p))
    n = np.cross(u, v)
    w = n / (n * n).sum(axis=-1, keepdims=True)
    unit = n / np.linalg.norm(n, axis=-1, keepdims=True)
    f = np.where(((d * unit).sum(axis=-1) > 0)[..., None], -unit, unit)
    planar = hit_p - Q
    alpha = (w * np.cross(planar, v)).sum(axis=-1)
    beta = (w * np.cross(u, planar)).sum(axis=-1)
    g = n0 * (1 - alpha - beta)[..., None] + n1 * alpha[..., None] + n2 * beta[..., None]
    l2 = (g * g).sum(axis=-1)
    with np.errstate(all="ignore"):
        s = g / np.sqrt(l2)[..., None]
    s = np.where(((s * f).sum(axis=-1) < 0)[..., None], -s, s)
    took = (l2 > 0) & ((d * s).sum(axis=-1) < 0)
    return np.where(took[..., None], s, f), took, g
