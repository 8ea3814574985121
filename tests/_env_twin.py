"""A numpy float32 twin of the environment-map rule and of one whole sample under a map — test infrastructure only.

lookup() restates environment_value() of csrc/rt_device_funcs.hpp operation by operation: the gradient's normalize, image_value's sphere map and constants with
acos / atan2 from the oracle's orc_math_batch (pinned to the device's rt_acosf / rt_atan2f by tests/test_gpu_cornell.py), the rotation added to u, then
image_texel's clamp, flip, truncation and caps.  Nothing of it is shared with the library.

radiance() is a COPY of _tri_twin.radiance at mode 0 (the older twins stay untouched, so it cannot be a call with a hook) with ONE change: the colour of a miss
comes from the parameter `sky`, a function of the missing rays' directions.  tests/test_environment_cpu.py pins the copy to _tri_twin.radiance bit for bit with the
constant and the gradient backgrounds passed as that parameter; the light-sampling branches, which mode 0 never takes, are left out.  `stats`, if given, counts the
misses by the bounce they happen at.
"""
import numpy as np

import _oracle as O
import _tri_twin as TT
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, PRIM_MOVING, _Tape, dot, near_zero

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


def sky_constant(color):
    c = np.array(list(color), F)
    return lambda d: np.broadcast_to(c, d.shape)


def sky_gradient(d):
    """the reference's two-colour sky, as _tri_twin.radiance states it"""
    inv = F(1) / np.sqrt(dot(d, d))
    tt = (d[:, 1] * inv) * F(0.5) + F(0.5)
    a, b = np.array([0.1, 0.2, 0.4], F), np.array([0.9, 0.9, 0.99], F)
    return a[None, :] + (b - a)[None, :] * tt[:, None]


def sky_environment(env, u0):
    return lambda d: lookup(env, u0, d)[0]


def primary_rays(cam, width, height, seed, gids, samples):
    """the pinhole camera's primary rays as radiance() below draws them: (tape, origin (n, 3), direction (n, 3))"""
    n = len(gids)
    tape = _Tape(seed, gids, samples)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        x, y = (gids % np.uint32(width)).astype(F), (gids // np.uint32(width)).astype(F)
        psx, psy = F(1) / F(width), F(1) / F(height)
        ndcx = ((x + F(0.5)) * psx) * F(2) - F(1)
        ndcy = ((y + F(0.5)) * psy) * F(2) - F(1)
        jx, jy = tape.in_unit2(rows)
        sx, sy = ndcx + jx * psx, ndcy + jy * psy
        co, cu, cv, cw = (np.array(list(v), F) for v in (cam.o, cam.u, cam.v, cam.w))
        ray_o = np.broadcast_to(co, (n, 3)).copy()
        ray_d = (cw[None, :] + cu[None, :] * sx[:, None]) + cv[None, :] * sy[:, None]
    return tape, ray_o, ray_d


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, stats=None):
    """Radiance of sample samples[i] of pixel gids[i] with the miss colour sky(directions (k, 3)) -> (k, 3): ((n, 3) float32, followed (n,) bool).
    _tri_twin.radiance at mode 0 statement by statement, but for the line marked below."""
    assert cam.type == 0, "the twin restates the pinhole camera"
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)
    if stats is not None:
        stats.setdefault("misses_by_bounce", np.zeros(max_depth, np.int64))
    tape, ray_o, ray_d = primary_rays(cam, width, height, seed, gids, samples)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        atten = np.ones((n, 3), F)
        accum = np.zeros((n, 3), F)
        out = np.zeros((n, 3), F)
        followed = np.ones(n, bool)
        live = rows.copy()
        for bounce in range(max_depth):
            if len(live) == 0:
                break
            k = len(live)
            rays = np.zeros((k, 7), F)
            rays[:, 0:3], rays[:, 3:6] = ray_o[live], ray_d[live]
            hit, t, prim, normal = TT.closest_intersection(world, rays)
            o, d = rays[:, 0:3], rays[:, 3:6]
            miss = hit == 0
            if miss.any():
                out[live[miss]] = atten[live[miss]] * np.asarray(sky(d[miss]), F) + accum[live[miss]]   # the one line that is not _tri_twin's: the miss colour
                if stats is not None:
                    stats["misses_by_bounce"][bounce] += int(miss.sum())
            mi = mat_of_prim[np.where(miss, 0, prim)]
            mt = np.where(miss, -1, m_type[mi])
            lit = mt == MAT_DIFFUSE_LIGHT   # a light of either kind: emits, never scatters
            accum[live[lit]] = accum[live[lit]] + atten[live[lit]] * m_albedo[mi[lit]]
            out[live[lit]] = accum[live[lit]]
            other = ~miss & ~lit & ~np.isin(mt, (0, 1, 3))
            followed[live[other]] = False
            out[live[other]] = np.nan
            go = np.isin(mt, (0, 1, 3))
            if bounce + 1 >= max_depth:
                out[live[go]] = accum[live[go]]
                break
            sel = np.nonzero(go)[0]
            r = live[sel]
            o, d, t, normal, mi, mt = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel]
            hit_p = o + d * t[:, None]
            k = len(r)
            lamb = mt != 1
            ok = np.ones(k, bool)
            new_d = np.zeros((k, 3), F)
            s = np.arange(k)
            if len(s):
                on_unit = tape.on_unit3(r[s])
                sl, sm = s[lamb[s]], s[~lamb[s]]
                new_d[sl] = normal[sl] + on_unit[lamb[s]]
                ok[sl] = ~near_zero(new_d[sl])
                dn = dot(normal[sm], d[sm])
                refl = d[sm] - (normal[sm] * dn[:, None]) * F(2)
                new_d[sm] = refl + on_unit[~lamb[s]] * m_param[mi[sm]][:, None]
                ok[sm] = ~((dot(new_d[sm], normal[sm]) < F(0)) | near_zero(new_d[sm]))
            albedo = m_albedo[mi].copy()
            chk = np.nonzero(mt == 3)[0]
            if len(chk):
                sp = hit_p[chk] * m_param[mi[chk]][:, None]
                ssum = np.trunc(sp).astype(np.int64).sum(axis=1)
                albedo[chk] = np.where((ssum % 2 == 0)[:, None], m_albedo[mi[chk]], m_albedo2[mi[chk]])
            out[r[~ok]] = accum[r[~ok]]
            r, new_d, hit_p, albedo = r[ok], new_d[ok], hit_p[ok], albedo[ok]
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = r
    return out, followed


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    rad, ok = radiance(world, cam, width, height, max_depth, seed, gids, smp, sky, stats)
    return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)


in_order_sums, resolve = TT.in_order_sums, TT.resolve
