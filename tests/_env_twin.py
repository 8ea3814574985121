"""A numpy float32 twin of the environment-map rule and of one whole sample under a map — test infrastructure only.

lookup() restates environment_value() of csrc/rt_device_funcs.hpp operation by operation: the gradient's normalize, image_value's sphere map and constants with
acos / atan2 from the oracle's orc_math_batch (pinned to the device's rt_acosf / rt_atan2f by tests/test_gpu_cornell.py), the rotation added to u, then
image_texel's clamp, flip, truncation and caps.  Nothing of it is shared with the library.

radiance() is the loop of tests/_path_twin.py over _tri_twin's walk, without a light rule, with the colour of a miss from the parameter `sky`, a function of the
missing rays' directions: sky_constant, sky_gradient (the world's own backgrounds, as that loop states them) or sky_environment.  tests/test_environment_cpu.py
holds it to _tri_twin.radiance bit for bit with the constant and the gradient backgrounds passed as that parameter.  `stats`, if given, counts the misses by the
bounce they happen at.
"""
import numpy as np

import _oracle as O
import _path_twin as PT
import _tri_twin as TT
from _nee_twin import F, dot
from _path_twin import primary_rays, sky_constant, sky_gradient  # noqa: F401

PI = F(float.fromhex("0x1.921fb6p+1"))
TWO_PI = F(float.fromhex("0x1.921fb6p+2"))


def _math(fn, a, b=None):
    a = np.ascontiguousarray(a, F)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, F)
    out = np.zeros(len(a), F)
    if len(a):
        O.lib().orc_math_batch(fn, len(a), a, b, out)
    return out


def _clamp01(x):
    """!(x > 0) ? 0 : (x > 1 ? 1 : x): a NaN lands on 0"""
    return np.where(~(x > F(0)), F(0), np.where(x > F(1), F(1), x)).astype(F)


def uv_of(u0, dirs):
    """(u, v) of the rule BEFORE the clamps, float32"""
    d = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt(dot(d, d))
        n = d * inv[:, None]
        cy = -n[:, 1]
        cy = np.where(cy < F(-1), F(-1), np.where(cy > F(1), F(1), cy)).astype(F)
        theta = _math(2, cy)
        phi = _math(3, -n[:, 2], n[:, 0]) + PI
        u = phi / TWO_PI + F(u0)
        u = np.where(u >= F(1), u - F(1), u).astype(F)
        v = theta / PI
    return u, v


def texel_of(width, height, u0, dirs):
    """the texel index j * width + i the rule picks, uint32"""
    u, v = uv_of(u0, dirs)
    with np.errstate(all="ignore"):
        u, v = _clamp01(u), _clamp01(v)
        v = F(1) - v
        i = (u * F(width)).astype(np.int32)   # (int): truncation; the operands are in [0, width]
        j = (v * F(height)).astype(np.int32)
    i, j = np.minimum(i, width - 1), np.minimum(j, height - 1)
    return (j.astype(np.uint32) * np.uint32(width) + i.astype(np.uint32)).astype(np.uint32)


def lookup(env, u0, dirs):
    """the rule on directions (n, 3): (rgb (n, 3) float32 as stored, texel (n,) uint32)"""
    env = np.ascontiguousarray(env, F)
    h, w, _ = env.shape
    texel = texel_of(w, h, u0, dirs)
    return env.reshape(-1, 3)[texel], texel


def sky_environment(env, u0):
    return lambda d: lookup(env, u0, d)[0]


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, stats=None):
    """Radiance of sample samples[i] of pixel gids[i] with the miss colour sky(directions (k, 3)) -> (k, 3): ((n, 3) float32, followed (n,) bool)"""
    return PT.radiance(world, cam, width, height, max_depth, seed, gids, samples, TT.closest_intersection, sky=sky,
                       stats=PT.counters(stats, {"misses_by_bounce": np.zeros(max_depth, np.int64)}))


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, sky, stats), width, height, spp, first_sample)


in_order_sums, resolve = TT.in_order_sums, TT.resolve
