"""A numpy float32 twin of the solid-glass rule and of whole samples under it — test infrastructure only.

expf() and interior_hit() restate rt_expf (csrc/rt_math.hpp) and interior_hit (csrc/rt_device_funcs.hpp; include/rt06.h: rt_scene_set_interior) in float32 numpy,
every operation rounded on its own.  Two whole-sample functions:

facing_radiance(): the FACING alone, through the loop of tests/_path_twin.py unedited.  solid_walk() wraps the walk: for a hit on a parallelogram or triangle whose
material has a record and whose stored normal says back, it returns the facing normal negated; the loop's own `behind = dot(d, n) > 0` then takes the rule's
decision and turns the normal back (negation is exact).  It serves every world that loop follows: smooth and frosted solids, maps, mode 48.

radiance(): the facing AND the absorption, as the `interiors` argument of that same loop: per glass hit the facing from the stored normal and the factor
expf(-(sigma * dist)) on the albedo.  With every sigma 0 it equals facing_radiance() bit for bit (tests/test_interiors_cpu.py).
"""
import numpy as np

import _env_tree_twin as VT
import _path_twin as PT
import _rglass_twin as RG
import _tri_twin as TT
from _nee2_twin import world_arrays
from _nee_twin import F, PRIM_MOVING, dot

INTERIOR_DT = np.dtype([("on", "<u4"), ("sigma", "<f4", 3)])
OFF, SOLID = 0, 1
LOG2E, LN2_HI, LN2_LO = (F(float.fromhex(h)) for h in ("0x1.715476p+0", "0x1.62e4p-1", "0x1.7f7d1cp-20"))
C3, C4, C5, C6, C7 = (F(float.fromhex(h)) for h in ("0x1.555556p-3", "0x1.555556p-5", "0x1.111112p-7", "0x1.6c16c2p-10", "0x1.a01a02p-13"))
# where floor(x log2 e + 1/2) steps: x = (k - 1/2) ln 2, k = 0 ... -125 — the reduction boundaries, whose neighbours the error test visits
BOUNDARIES = ((np.arange(0, -126, -1, dtype=np.float64) - 0.5) * np.log(2.0)).astype(F)


def expf(x):
    """rt_expf, operation for operation"""
    x = np.ascontiguousarray(x, F)
    with np.errstate(all="ignore"):
        live = x > F(-87.0)
        xs = np.where(live, x, F(0)).astype(F)
        kf = np.floor(xs * LOG2E + F(0.5))
        r = xs - kf * LN2_HI
        r = r - kf * LN2_LO
        p = F(1) + r * (F(1) + r * (F(0.5) + r * (C3 + r * (C4 + r * (C5 + r * (C6 + r * C7))))))
        scale = ((kf.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F)
        return np.where(live, p * scale, F(0)).astype(F)


def interior_hit(back, ray_d, t, ior, sigma):
    """steps 1 and 2 of the rule from the facing: (eta (k,), T (k, 3)); T is ones where not back"""
    d, sigma = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (ray_d, sigma))
    t, ior = (np.ascontiguousarray(a, F).reshape(-1) for a in (t, ior))
    back = np.asarray(back, bool).reshape(-1)
    with np.errstate(all="ignore"):
        eta = np.where(back, ior, F(1) / ior).astype(F)
        dist = t * np.sqrt(dot(d, d))
        T = expf((-(sigma * dist[:, None])).reshape(-1)).reshape(-1, 3)
    return eta, np.where(back[:, None], T, F(1)).astype(F)


def case(Ng, n, ray_d, t, ior, sigma, sphere):
    """rt_interior_batch: (back uint32, eta, T)"""
    Ng, n, d = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (Ng, n, ray_d))
    with np.errstate(all="ignore"):
        back = dot(d, np.where(np.asarray(sphere).reshape(-1, 1) != 0, n, Ng).astype(F)) > F(0)
    eta, T = interior_hit(back, d, t, ior, sigma)
    return back.astype(np.uint32), eta, T


# ---- whole samples --------------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    return {name: 0 for name in ("tri_front", "tri_back", "quad_front", "quad_back", "sphere_front", "sphere_back", "smooth_back", "total_inside", "charged",
                                 "frosted_front", "frosted_back", "unrecorded_mesh")}


def _materials(world):
    prims, quads, mats = world_arrays(world)
    return prims, quads, mats, np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)


def solid_walk(trace, interiors, info=None):
    """`trace` with the rule's facing folded into the normal it returns (see the module's text).  info (a dict): 'turned' counts the hits it negated."""
    def walk(world, rays, preset=None, **draws):
        hit, t, prim, normal = trace(world, rays, **draws) if preset is None else trace(world, rays, preset, **draws)
        prims, quads, _, mat_of_prim = _materials(world)
        rows = np.nonzero((hit != 0) & (prim >= len(prims)))[0]
        rows = rows[interiors["on"][mat_of_prim[prim[rows]]] != OFF]
        if len(rows):
            with np.errstate(all="ignore"):
                back = dot(np.ascontiguousarray(rays[rows, 3:6], F), quads["normal"][prim[rows] - len(prims)].astype(F)) > F(0)
            normal = normal.copy()
            normal[rows[back]] = -normal[rows[back]]
            if info is not None:
                info["turned"] = info.get("turned", 0) + int(back.sum())
        return hit, t, prim, normal
    return walk


def facing_radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, interiors, light=None, tree=None, tex=None, mfacs=None, stats=None, walk=None,
                    trace=TT.closest_intersection, info=None):
    """_rglass_twin.radiance over the wrapped walk: the facing of every record, no absorption"""
    return RG.radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light, tree, tex, mfacs, stats, walk, solid_walk(trace, interiors, info))


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, interiors, light=None, tree=None, mfacs=None, stats=None, trace=TT.closest_intersection,
             smooth_tris=None):
    """Radiance of sample samples[i] of pixel gids[i] under the whole rule: ((n, 3) float32, followed (n,) bool) — _path_twin's loop with the records as its
    `interiors` argument.  trace: the UNWRAPPED walk (flat, or smooth under a table of vertex normals); light, tree: mode 48's, as _rglass_twin takes them; mfacs:
    the microfacet and rough-glass records (a mapped one needs a texture table, which this signature does not carry); stats: new_stats()'s counters grow.
    smooth_tris: per triangle of the world, whether it has vertex normals, for the smooth_back counter."""
    rule = VT.MapRule(world, light, tree) if light is not None else None
    run = None if stats is None else PT.counters(dict(stats), VT.new_stats())   # the light rule counts into its own names; the caller's dict keeps this module's
    out = PT.radiance(world, cam, width, height, max_depth, seed, gids, samples, trace, sky=sky, rule=rule, mfacs=mfacs, glass=True, stats=run,
                      interiors=interiors, smooth_tris=smooth_tris)
    if stats is not None:
        stats.update({key: run[key] for key in stats})
    return out


in_order_sums, resolve = VT.in_order_sums, VT.resolve
