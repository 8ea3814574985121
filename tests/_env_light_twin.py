"""A numpy float32 twin of environment light sampling and of one whole sample under it — test infrastructure only.

draw() restates environment_sample() of csrc/rt_device_funcs.hpp operation by operation on the tables rt_environment_distribution gave: the two products, the
float just below the total where a product reaches it, the two searches (numpy's searchsorted on non-decreasing sums finds the same smallest index), the point in
the texel, the sine from the oracle's orc_math_batch (pinned to the device's rt_sinf by tests/test_gpu_cornell.py).  density_of() is the density of the texel
_env_twin.texel_of puts a direction in.  Nothing of it is shared with the library.

radiance() is a COPY of _env_twin.radiance (the older twins stay untouched) with the mixture step of §24 added: with `light` None it is that function statement by
statement — tests/test_env_light_cpu.py pins that bit for bit — and with `light` = (tables, env, u0) a Lambertian or checker hit draws c, takes the map's half below
0.5, and weighs the path by sp / pdf.  `stats` counts what a run exercised.
"""
import numpy as np

import _env_twin as ET
import _tri_twin as TT
from _env_twin import _math, primary_rays, texel_of
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, PRIM_MOVING, dot, near_zero

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
    hits: ((n, 3) float32, followed (n,) bool).  _env_twin.radiance statement by statement, but for the blocks marked §24."""
    assert cam.type == 0, "the twin restates the pinhole camera"
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)
    if stats is not None:
        stats.setdefault("misses_by_bounce", np.zeros(max_depth, np.int64))
        for key, zero in new_stats().items():
            stats.setdefault(key, zero)
    tape, ray_o, ray_d = primary_rays(cam, width, height, seed, gids, samples)
    rows = np.arange(n)
    from_light = np.zeros(n, bool)   # §24 (stats only): the ray being traced was drawn from the map
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
            if stats is not None:
                stats["light_half_hit"] += int((from_light[live] & ~miss).sum())
            if miss.any():
                out[live[miss]] = atten[live[miss]] * np.asarray(sky(d[miss]), F) + accum[live[miss]]
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
            # §24: the first draw of a Lambertian / checker hit picks the half; the map's half draws x1, x2, a, b and no on-unit vector
            weight = np.ones(k, F)
            weighted = np.zeros(k, bool)
            to_light = np.zeros(k, bool)
            if light is not None and lamb.any():
                c = tape.next(r[lamb])
                to_light[np.nonzero(lamb)[0]] = c < F(0.5)
            if to_light.any():
                s = np.nonzero(to_light)[0]
                four = np.stack([tape.next(r[s]) for _ in range(4)], axis=1)
                new_d[s] = draw(light[0], light[1], four)[0]
                if stats is not None:
                    stats["light_half"] += len(s)
                    stats["checker_light_half"] += int((mt[s] == 3).sum())
            s = np.nonzero(~to_light)[0]
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
            if light is not None:   # §24: the densities of the direction under both halves
                s = np.nonzero(lamb & ok)[0]
                if len(s):
                    dd, nn = new_d[s], normal[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    pdf_light = density_of(light[0], light[1], dd)
                    pdf = F(0.5) * pdf_cos + F(0.5) * pdf_light
                    good = ~(pdf_cos == F(0)) & (pdf > F(0))
                    if stats is not None:
                        stats["below_surface"] += int((pdf_cos == F(0)).sum())
                    ok[s[~good]] = False
                    weight[s[good]] = pdf_cos[good] / pdf[good]
                    weighted[s[good]] = True
                albedo = np.where(weighted[:, None], albedo * weight[:, None], albedo)
            out[r[~ok]] = accum[r[~ok]]
            from_light[r] = to_light
            r, new_d, hit_p, albedo = r[ok], new_d[ok], hit_p[ok], albedo[ok]
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = r
    return out, followed


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, light=None, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    rad, ok = radiance(world, cam, width, height, max_depth, seed, gids, smp, sky, light, stats)
    return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)


in_order_sums, resolve = ET.in_order_sums, ET.resolve
