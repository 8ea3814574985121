"""A numpy float32 twin of the solid-glass rule and of whole samples under it — test infrastructure only.

expf() and interior_hit() restate rt_expf (csrc/rt_math.hpp) and interior_hit (csrc/rt_device_funcs.hpp; include/rt06.h: rt_scene_set_interior) in float32 numpy,
every operation rounded on its own.  Two whole-sample functions:

facing_radiance(): the FACING alone, through the loop of tests/_path_twin.py unedited.  solid_walk() wraps the walk: for a hit on a parallelogram or triangle whose
material has a record and whose stored normal says back, it returns the facing normal negated; the loop's own `behind = dot(d, n) > 0` then takes the rule's
decision and turns the normal back (negation is exact).  It serves every world that loop follows: smooth and frosted solids, maps, mode 48.

radiance(): the facing AND the absorption, through a short loop of its own — _path_twin takes a glass hit's factor per material and a transmittance is per hit,
so the unedited loop cannot carry it.  It follows a miss, a light, Lambertian, metal, smooth glass and rough glass of constant roughness, plain or under
_path_twin's light rules, and nothing else.  With every sigma 0 it equals facing_radiance() bit for bit (tests/test_interiors_cpu.py).  A later refactor folds it
into the one loop as an argument.
"""
import numpy as np

import _env_tree_twin as VT
import _mfac_twin as MT
import _path_twin as PT
import _rglass_twin as RG
import _tri_twin as TT
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, PRIM_MOVING, count, dot, near_zero

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
    def walk(world, rays, preset=None):
        hit, t, prim, normal = trace(world, rays) if preset is None else trace(world, rays, preset)
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
    """Radiance of sample samples[i] of pixel gids[i] under the whole rule: ((n, 3) float32, followed (n,) bool).  trace: the UNWRAPPED walk (flat, or smooth under
    a table of vertex normals); light, tree: mode 48's, as _rglass_twin takes them; mfacs: rough-glass records of constant roughness are followed, any other
    record is not; stats: new_stats()'s counters grow.  smooth_tris: per triangle of the world, whether it has vertex normals, for the smooth_back counter."""
    gids, samples = np.ascontiguousarray(gids, np.uint32), np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats, mat_of_prim = _materials(world)
    n_prims = len(prims)
    first_tri = n_prims + int((quads["kind"] == 0).sum())
    m_type, m_albedo, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["param"].astype(F)
    rule = VT.MapRule(world, light, tree) if light is not None else None
    tape, ray_o, ray_d = PT.primary_rays(cam, width, height, seed, gids, samples)
    with np.errstate(all="ignore"):
        atten, accum, out = np.ones((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
        followed = np.ones(n, bool)
        live = np.arange(n)
        for bounce in range(max_depth):
            if len(live) == 0:
                break
            k = len(live)
            rays = np.zeros((k, 7), F)
            rays[:, 0:3], rays[:, 3:6] = ray_o[live], ray_d[live]
            hit, t, prim, normal = trace(world, rays)
            o, d = rays[:, 0:3], rays[:, 3:6]
            miss = hit == 0
            out[live[miss]] = atten[live[miss]] * np.asarray(sky(d[miss]), F) + accum[live[miss]]
            mi = mat_of_prim[np.where(miss, 0, prim)]
            mt = np.where(miss, -1, m_type[mi])
            lit = mt == MAT_DIFFUSE_LIGHT
            accum[live[lit]] = accum[live[lit]] + atten[live[lit]] * m_albedo[mi[lit]]
            out[live[lit]] = accum[live[lit]]
            go = np.isin(mt, (0, PT.MAT_METAL))
            through = mt == PT.MAT_DIELECTRIC
            rec_mf = mfacs[mi] if mfacs is not None else None
            if rec_mf is not None:   # a record this loop has no rule for: the sample is left out
                strange = ~miss & (((rec_mf["on"] != MT.OFF) & ~through) | (through & ~np.isin(rec_mf["on"], (MT.OFF, RG.GLASS))))
                go, through = go & ~strange, through & ~strange
            other = ~miss & ~lit & ~through & ~go
            followed[live[other]] = False
            out[live[other]] = np.nan
            if bounce + 1 >= max_depth:
                out[live[go | through]] = accum[live[go | through]]
                break
            carried = []
            gl = np.nonzero(through)[0]
            if len(gl):
                rg, dg, ng, tg, pm = live[gl], d[gl], normal[gl], t[gl], prim[gl]
                pg = o[gl] + dg * tg[:, None]
                rec = interiors[mi[gl]]
                solid, flat = rec["on"] != OFF, pm >= n_prims
                stored = quads["normal"][np.where(flat, pm - n_prims, 0)].astype(F) if len(quads) else np.zeros((len(gl), 3), F)
                kept = solid & flat                                          # 1: the facing from the stored normal; the shading normal stays
                back = np.where(kept, dot(dg, stored) > F(0), dot(dg, ng) > F(0))
                ng = np.where((back & ~kept)[:, None], -ng, ng)
                ior = m_param[mi[gl]]
                ratio, T = interior_hit(back, dg, tg, ior, rec["sigma"])
                charged = solid & back                                       # 2
                albedo_g = np.where(charged[:, None], m_albedo[mi[gl]] * T, m_albedo[mi[gl]]).astype(F)
                smooth = np.ones(len(gl), bool)
                frosted = np.zeros(len(gl), bool)
                total_rough = np.zeros(len(gl), bool)
                if mfacs is not None:
                    has = np.nonzero(mfacs["on"][mi[gl]] == RG.GLASS)[0]
                    if len(has):
                        frosted[has] = True
                        det = {}
                        new_w, g1, way = RG.faced(ng[has], ratio[has], dg[has], mfacs["roughness"][mi[gl[has]]].astype(F), tape, rg[has], det)
                        goes, gone = (way == RG.SPECULAR) | (way == RG.TRANSMITTED), way == RG.ABSORBED
                        smooth[has] = ~(goes | gone)
                        total_rough[has] = det["total"]
                        out[rg[has][gone]] = accum[rg[has][gone]]
                        carried.append((rg[has][goes], new_w[goes], pg[has][goes], (albedo_g[has] * g1[:, None]).astype(F)[goes]))
                unit = MT.normalize(dg)
                cos_t = np.minimum(dot(-unit, ng), F(1))
                sin_t = np.sqrt(F(1) - cos_t * cos_t)
                r0 = (F(1) - ratio) / (F(1) + ratio)
                r0 = r0 * r0
                x1 = F(1) - cos_t
                x2 = x1 * x1
                prob = r0 + (F(1) - r0) * ((x2 * x2) * x1)
                must = ratio * sin_t > F(1)
                reflects = must.copy()
                free = np.nonzero(~must & smooth)[0]
                if len(free):
                    reflects[free] = prob[free] > tape.next(rg[free])
                refl = unit - (ng * dot(ng, unit)[:, None]) * F(2)
                dv = dot(ng, unit)
                kk = F(1) - (ratio * ratio) * (F(1) - dv * dv)
                refr = np.where((kk >= F(0))[:, None], unit * ratio[:, None] - ng * (ratio * dv + np.sqrt(kk))[:, None], F(0)).astype(F)
                carried.append((rg[smooth], np.where(reflects[:, None], refl, refr).astype(F)[smooth], pg[smooth], albedo_g[smooth]))
                if stats is not None:
                    tri, quad, sph = solid & flat & (pm >= first_tri), solid & flat & (pm < first_tri), solid & ~flat
                    for name, sel in (("tri", tri), ("quad", quad), ("sphere", sph)):
                        stats[name + "_front"] += int((sel & ~back).sum())
                        stats[name + "_back"] += int((sel & back).sum())
                    if smooth_tris is not None and len(smooth_tris):
                        stats["smooth_back"] += int((tri & back & smooth_tris[np.clip(pm - first_tri, 0, len(smooth_tris) - 1)]).sum())
                    stats["total_inside"] += int((solid & back & ((must & smooth) | total_rough)).sum())
                    stats["charged"] += int(charged.sum())
                    stats["frosted_front"] += int((solid & frosted & ~back).sum())
                    stats["frosted_back"] += int((solid & frosted & back).sum())
                    stats["unrecorded_mesh"] += int((~solid & flat & (pm >= first_tri)).sum())
            sel = np.nonzero(go)[0]
            r = live[sel]
            o, d, t, normal, mi, mt = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel]
            hit_p = o + d * t[:, None]
            k = len(r)
            lamb = mt != PT.MAT_METAL
            ok = np.ones(k, bool)
            new_d = np.zeros((k, 3), F)
            weight, weighted = np.ones(k, F), np.zeros(k, bool)
            to_light = np.zeros(k, bool)
            if rule is not None:
                sampled = lamb.copy()
                to_light, _, picked = rule.pick(tape, r, sampled, mt, hit_p, new_d, None)
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
            if rule is not None:
                s = np.nonzero(sampled & ok)[0]
                if len(s):
                    dd, nn = new_d[s], normal[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    pdf_light, own_lost = rule.density(picked, s, hit_p[s], dd, len2, ln, pdf_cos, None)
                    pdf = F(0.5) * pdf_cos + F(0.5) * pdf_light
                    good = ~(pdf_cos == F(0)) & (pdf > F(0)) & ~own_lost
                    ok[s[~good]] = False
                    weight[s[good]] = pdf_cos[good] / pdf[good]
                    weighted[s[good]] = True
                albedo = np.where(weighted[:, None], albedo * weight[:, None], albedo)
            out[r[~ok]] = accum[r[~ok]]
            carried.append((r[ok], new_d[ok], hit_p[ok], albedo[ok]))
            r = np.concatenate([c[0] for c in carried])
            new_d, hit_p, albedo = (np.concatenate([c[i] for c in carried]).astype(F) for i in (1, 2, 3))
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = np.sort(r)
    if stats is not None:
        count(stats, "not_followed", int((~followed).sum()))
    return out, followed


in_order_sums, resolve = VT.in_order_sums, VT.resolve
