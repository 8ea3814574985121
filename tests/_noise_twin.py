"""A numpy float32 twin of the marble of RT_MAT_LAMBERTIAN_NOISE — test infrastructure only.

noise(), turb() and value() restate perlin_noise, perlin_turb and noise_value (oracle/rt_oracle.c; csrc: the function rt_noise_value_batch calls) in float32
numpy, every operation rounded on its own, in their one evaluation order, with the project's deterministic sine (orc_math_batch fn 1 = rt_sinf).  Pinned to
rt_noise_value_batch bit for bit before the whole-sample loop uses it (tests/test_path_twin_oracle_cpu.py).
"""
import ctypes as C

import numpy as np

import _oracle as O

F = np.float32


def tables(world):
    """(randvec (256, 3) float32, perm (3, 256) int64) of a flat world's rt_perlin"""
    assert world.perlin, "the world has no Perlin tables"
    buf = bytes((C.c_char * 6144).from_address(world.perlin))
    return np.frombuffer(buf[:3072], "<f4").reshape(256, 3).copy(), np.frombuffer(buf[3072:], "<i4").reshape(3, 256).astype(np.int64)


def _sin(x):
    x = np.ascontiguousarray(x, F)
    out = np.zeros(len(x), F)
    O.lib().orc_math_batch(1, len(x), x, x, out)
    return out


def noise(tab, p):
    """perlin::noise with the Hermite-smoothed trilinear interpolation of the eight lattice vectors: (n,) float32"""
    randvec, perm = tab
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        fl = np.floor(p)
        uvw = p - fl
        ijk = fl.astype(np.int64)
        h = (uvw * uvw) * (F(3) - F(2) * uvw)
        accum = np.zeros(len(p), F)
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    idx = perm[0][(ijk[:, 0] + di) & 255] ^ perm[1][(ijk[:, 1] + dj) & 255] ^ perm[2][(ijk[:, 2] + dk) & 255]
                    c = randvec[idx]
                    wx, wy, wz = uvw[:, 0] - F(di), uvw[:, 1] - F(dj), uvw[:, 2] - F(dk)
                    d = (c[:, 0] * wx + c[:, 1] * wy) + c[:, 2] * wz
                    wi = h[:, 0] if di else F(1) - h[:, 0]
                    wj = h[:, 1] if dj else F(1) - h[:, 1]
                    wk = h[:, 2] if dk else F(1) - h[:, 2]
                    accum = accum + ((wi * wj) * wk) * d
    return accum


def turb(tab, p, depth=7):
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        accum, weight = np.zeros(len(p), F), F(1)
        for _ in range(depth):
            accum = accum + weight * noise(tab, p)
            weight = weight * F(0.5)
            p = p * F(2)
        return np.abs(accum)


def value(tab, albedo, scale, p):
    """noise_texture::value: albedo * (1 + sin(scale * z + 10 * turb(p, 7))); albedo (n, 3) or (3,), scale (n,) or a number, p (n, 3) -> (n, 3) float32"""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    albedo = np.broadcast_to(np.asarray(albedo, F), (len(p), 3))
    scale = np.broadcast_to(np.asarray(scale, F), (len(p),))
    with np.errstate(all="ignore"):
        return (albedo * (F(1) + _sin(scale * p[:, 2] + F(10) * turb(tab, p)))[:, None]).astype(F)
