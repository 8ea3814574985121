"""A numpy float32 twin of environment light sampling and of one whole sample under it — test infrastructure only.

draw() restates environment_sample() of csrc/rt_device_funcs.hpp operation by operation on the tables rt_environment_distribution gave: the two products, the
float just below the total where a product reaches it, the two searches (numpy's searchsorted on non-decreasing sums finds the same smallest index), the point in
the texel, the sine from the oracle's orc_math_batch (pinned to the device's rt_sinf by tests/test_gpu_cornell.py).  density_of() is the density of the texel
_env_twin.texel_of puts a direction in.  Nothing of it is shared with the library.

radiance() is the loop of tests/_path_twin.py with the mixture step of §24: with `light` None it is _env_twin.radiance — tests/test_env_light_cpu.py holds that bit
for bit — and with `light` = (tables, u0) a Lambertian or checker hit draws c, takes the map's half below 0.5, and weighs the path by sp / pdf
(_env_tree_twin.MapRule without a table).  `stats` counts what a run exercised.
"""
import numpy as np

import _env_twin as ET
import _path_twin as PT
import _tri_twin as TT
from _env_twin import _math, primary_rays, texel_of  # noqa: F401
from _nee_twin import F

PI = F(float.fromhex("0x1.921fb6p+1"))
TWO_PI = F(float.fromhex("0x1.921fb6p+2"))
HALF_PI = F(float.fromhex("0x1.921fb6p+0"))


def _below(x):
    """the float just below a positive float: bit pattern - 1"""
    return (np.asarray(x, F).view(np.uint32) - np.uint32(1)).view(F)


def draw(tables, u0, uniforms):
    """the rule on uniforms (n, 4) = (x1, x2, a, b): (directions (n, 3) float32, drawn texel (n,) uint32 = j * W + i)"""
    rowc, rowy, colc = (np.ascontiguousarray(tables[k], F) for k in ("rowc", "rowy", "colc"))
    h, w = colc.shape
    u = np.ascontiguousarray(uniforms, F).reshape(-1, 4)
    x1, x2, a, b = u[:, 0], u[:, 1], u[:, 2], u[:, 3]
    with np.errstate(all="ignore"):
        A = rowc[h - 1]
        x = x1 * A
        x = np.where(x < A, x, _below(A)).astype(F)
        j = np.minimum(np.searchsorted(rowc, x, side="right"), h - 1)   # the smallest j with rowc[j] > x
        R = colc[j, w - 1]
        x = x2 * R
        x = np.where(x < R, x, _below(R)).astype(F)
        i = np.zeros(len(u), np.int64)
        for row in np.unique(j):
            m = j == row
            i[m] = np.minimum(np.searchsorted(colc[row], x[m], side="right"), w - 1)
        uu = (i.astype(F) + a) / F(w)
        y1 = rowy[j + 1]
        y = y1 + (rowy[j] - y1) * b
        s2 = F(1) - y * y
        s = np.sqrt(np.where(s2 > F(0), s2, F(0)).astype(F))
        t = uu - F(u0)
        t = np.where(t < F(0), t + F(1), t).astype(F)
        psi = t * TWO_PI - PI
        d = np.stack([s * _math(1, psi + HALF_PI), y, -(s * _math(1, psi))], axis=1).astype(F)
    return d, (j * w + i).astype(np.uint32)


def density_of(tables, u0, dirs):
    """the density of directions (n, 3): that of the texel §23's lookup puts each in"""
    dens = np.ascontiguousarray(tables["density"], F)
    h, w = dens.shape
    return dens.reshape(-1)[texel_of(w, h, u0, dirs)]


def new_stats():
    """light_half: draws of the map's half; light_half_hit: of those, directions that met geometry at the next trace; below_surface: paths ended with sp == 0;
    checker_light_half: checker hits that took the map's half; misses_by_bounce as _env_twin counts them"""
    return {"light_half": 0, "light_half_hit": 0, "below_surface": 0, "checker_light_half": 0}


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, stats=None):
    """Radiance of sample samples[i] of pixel gids[i] with the miss colour sky(directions) and, light = (tables, u0), §24's mixture at Lambertian and checker
    hits: ((n, 3) float32, followed (n,) bool)"""
    import _env_tree_twin as VT   # (the map's rule stands above this module: it serves mode 48 as well)
    return PT.radiance(world, cam, width, height, max_depth, seed, gids, samples, TT.closest_intersection, sky=sky,
                       rule=VT.MapRule(world, light) if light is not None else None,
                       stats=PT.counters(stats, {"misses_by_bounce": np.zeros(max_depth, np.int64), **new_stats()}))


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, light=None, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, sky, light, stats), width, height, spp, first_sample)


in_order_sums, resolve = ET.in_order_sums, ET.resolve
