"""The numpy float32 twin of one whole sample for light sampling over quad, sphere AND triangle lights (mode 4) — test infrastructure only.

tests/_tri_twin.py restates §18 (worlds with triangles; modes 0, 1 and 2, whose tables leave triangles out) and stays as it is.  This module has a radiance()
of its own that also takes mode 4 = RT_LIGHT_SAMPLING_MESH: mode 2's table, then every triangle whose material is a diffuse light, in quad-index order, with
area = 0.5f * sqrt(dot(n, n)), n = cross(u, v).  The two rules mode 4 adds are functions of their own, so that a test can hold them to mathematics no kernel
shares (tests/test_mesh_lights_cpu.py: uniformity over the triangle, and the mean of 1 / pl against the solid angle):

    _tri_point(a, b, Q, u, v, hit_p)   the fold `if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }` — one fp32 add, a sum of exactly 1 is not folded — and
                                       d = ((Q + u * a) + v * b) - hit_p, not normalised
    _tri_pl(q, area, hp, dd, len2, ln) the library's quad test with the triangle kind on (hp, dd) over a fresh trace's interval; on a hit
                                       pl = ((t * t) * len2) / ((|dot(dd, n)| / ln) * area), on a miss 0

radiance() below is a COPY of _tri_twin.radiance (the older twins stay untouched, so it cannot be a call with a hook): all but the lines marked §19 are its text.
tests/test_mesh_lights_cpu.py pins it before anything is compared with it: in modes 0, 1 and 2 it equals _tri_twin on every world, and in mode 4 it equals
_tri_twin's mode 2 on worlds without a triangle light, bit for bit.

Scope: _tri_twin's.
"""
import numpy as np

import _nee2_twin as T2
import _nee_twin as T
import _tri_twin as TT
from _nee2_twin import QUAD, SPHERE, MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, MAX_LIGHTS, MISS, PRIM_MOVING, _Tape, cross, dot, near_zero
from _tri_twin import closest_intersection, first_hit_sums, kinds

TRIANGLE = 2            # RT_LIGHT_TRIANGLE
MAX_LIGHTS_MESH = 64    # RT_MAX_LIGHTS_MESH
_quad_hit = T._quad_hit


def triangle_lights(quads, mats):
    """(quad indices, areas): the triangles whose material is a diffuse light, in quad-index order; area = 0.5f * sqrt(dot(n, n)), n = cross(u, v)"""
    idx = np.array([i for i in range(len(quads)) if quads["kind"][i] == 1 and mats["type"][quads["mat"][i]] == MAT_DIFFUSE_LIGHT], dtype=np.uint32)
    if len(idx) == 0:
        return idx, np.zeros(0, F)
    n = cross(quads["u"][idx].astype(F), quads["v"][idx].astype(F))
    return idx, (F(0.5) * np.sqrt(dot(n, n))).astype(F)


def lights_of(prims, quads, mats, mode):
    """(kind, index, area) of the light table of `mode`: _tri_twin.lights_of for modes 1 and 2; mode 4: mode 2's table, then the triangle lights"""
    if mode != 4:
        return TT.lights_of(prims, quads, mats, mode)
    kind, index, area = TT.lights_of(prims, quads, mats, 2)
    t_idx, t_area = triangle_lights(quads, mats)
    return (np.concatenate([kind, np.full(len(t_idx), TRIANGLE, np.int64)]), np.concatenate([index, t_idx.astype(np.int64)]),
            np.concatenate([area, t_area]).astype(F))


def new_stats():
    """_nee2_twin's counters with light_samples[i] over a table of 64, and for triangle lights: tri_light_half: light-half draws sent to a triangle light;
    tri_folded: of those, the draws with a + b > 1; tri_own_missed: light-half draws whose own triangle's test rejects the direction (a point that rounding put
    just outside: pl_j = 0, the direction is still taken); two_tri_crossings: directions that meet two or more triangle lights (both crossings of a closed
    mesh); tri_and_other: directions that meet a triangle light and a light of another kind"""
    st = T2.new_stats()
    st["light_samples"] = np.zeros(MAX_LIGHTS_MESH, np.int64)
    st.update({"tri_light_half": 0, "tri_folded": 0, "tri_own_missed": 0, "two_tri_crossings": 0, "tri_and_other": 0})
    return st


def _tri_point(a, b, Q, u, v, hit_p):
    """§19's drawn point: a, b (n,) uniforms; Q, u, v (n, 3) or (3,); hit_p (n, 3): the unnormalised direction (n, 3) to the folded point"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    Q, u, v = (np.broadcast_to(np.asarray(x, F), hit_p.shape) for x in (Q, u, v))
    fold = (a + b) > F(1)   # one fp32 add; exactly 1 stays
    a2 = np.where(fold, F(1) - a, a).astype(F)
    b2 = np.where(fold, F(1) - b, b).astype(F)
    return ((Q + u * a2[:, None]) + v * b2[:, None]) - hit_p


def _tri_hit(q, o, d):
    """quad_closest_intersection with RT_QUAD_TRIANGLE of one record on rays (o, d) over a fresh trace's interval: _nee_twin._quad_hit's arithmetic and the
    kind rule !(alpha + beta <= 1)"""
    n = np.broadcast_to(q["normal"].astype(F), d.shape)
    denom = dot(n, d)
    t = (F(q["D"]) - dot(n, o)) / denom
    hit = ~(np.abs(denom) < F(1e-8)) & ~(t < F(0)) & ~(t >= MISS)
    planar = (o + d * t[:, None]) - q["Q"].astype(F)[None, :]
    w = np.broadcast_to(q["w"].astype(F), d.shape)
    alpha = dot(w, cross(planar, np.broadcast_to(q["v"].astype(F), d.shape)))
    beta = dot(w, cross(np.broadcast_to(q["u"].astype(F), d.shape), planar))
    hit &= (alpha >= F(0)) & (alpha <= F(1)) & (beta >= F(0)) & (beta <= F(1))
    hit &= (alpha + beta) <= F(1)
    return hit, t


def _tri_pl(q, area, hp, dd, len2, ln):
    """§19's density of one triangle light (flat record q, area) along rays (hp, dd): (pl_j, hit)"""
    thit, t = _tri_hit(q, hp, dd)
    nj = np.broadcast_to(q["normal"].astype(F), dd.shape)
    pl = ((t * t) * len2) / ((np.abs(dot(dd, nj)) / ln) * F(area))
    return np.where(thit, pl, F(0)).astype(F), thit


def radiance(world, cam, width, height, max_depth, seed, gids, samples, mode=0, stats=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 / 4 as rt_renderer_light_sampling_enable takes it.
    _tri_twin.radiance statement by statement, but for the lines marked §19 below."""
    assert cam.type == 0, "the twin restates the pinhole camera"
    assert mode in (0, 1, 2, 4)   # §19
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    l_kind, l_index, l_area = lights_of(prims, quads, mats, mode)   # §19: mode 4 lists the triangle lights behind mode 2's table
    n_l = len(l_kind)
    if mode:
        assert 1 <= n_l <= (MAX_LIGHTS_MESH if mode == 4 else MAX_LIGHTS)   # §19
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)

    if stats is not None:
        for key, zero in new_stats().items():   # §19
            stats.setdefault(key, zero)
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
            hit, t, prim, normal = closest_intersection(world, rays)   # the one step that is not _nee2_twin's: the walk below, which knows the kind
            o, d = rays[:, 0:3], rays[:, 3:6]
            miss = hit == 0
            if miss.any():
                dm = d[miss]
                if world.background == 1:
                    sky = np.broadcast_to(np.array(list(world.background_color), F), dm.shape)
                else:
                    inv = F(1) / np.sqrt(dot(dm, dm))
                    tt = (dm[:, 1] * inv) * F(0.5) + F(0.5)
                    a, b = np.array([0.1, 0.2, 0.4], F), np.array([0.9, 0.9, 0.99], F)
                    sky = a[None, :] + (b - a)[None, :] * tt[:, None]
                out[live[miss]] = atten[live[miss]] * sky + accum[live[miss]]
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
            weight = np.ones(k, F)
            weighted = np.zeros(k, bool)
            to_light = np.zeros(k, bool)
            drawn = np.full(k, -1, np.int64)   # the light a light-half draw went to
            if mode and lamb.any():
                c = tape.next(r[lamb])
                to_light[np.nonzero(lamb)[0]] = c < F(0.5)
            if to_light.any():
                s = np.nonzero(to_light)[0]
                li = np.zeros(len(s), np.int64)
                if n_l > 1:
                    scaled = (tape.next(r[s]) * F(n_l)).astype(np.uint32)
                    li = np.minimum(scaled, np.uint32(n_l - 1)).astype(np.int64)
                    if stats is not None:
                        stats["index_clamped"] += int((scaled >= n_l).sum())
                drawn[s] = li
                if stats is not None:
                    stats["light_samples"] += np.bincount(li, minlength=MAX_LIGHTS_MESH)   # §19
                    stats["checker_light_half"] += int((mt[s] == 3).sum())
                    stats["sphere_light_half"] += int((l_kind[li] == SPHERE).sum())
                sq_, ss_ = s[l_kind[li] == QUAD], s[l_kind[li] == SPHERE]
                st_ = s[l_kind[li] == TRIANGLE]   # §19, to the end of the block
                if len(st_):   # a, b folded into the triangle: a point uniform over its area; no on-unit draw
                    la = tape.next(r[st_])
                    lb = tape.next(r[st_])
                    q = quads[l_index[drawn[st_]]]
                    new_d[st_] = _tri_point(la, lb, q["Q"].astype(F), q["u"].astype(F), q["v"].astype(F), hit_p[st_])
                    if stats is not None:
                        stats["tri_light_half"] += len(st_)
                        stats["tri_folded"] += int(((la + lb) > F(1)).sum())
                if len(sq_):   # a, b: a point of the parallelogram
                    la = tape.next(r[sq_])
                    lb = tape.next(r[sq_])
                    q = quads[l_index[drawn[sq_]]]
                    new_d[sq_] = ((q["Q"].astype(F) + q["u"].astype(F) * la[:, None]) + q["v"].astype(F) * lb[:, None]) - hit_p[sq_]
                if len(ss_):   # rng_on_unit3, rejection loop and all: a point of the sphere, uniform over its area
                    u = tape.on_unit3(r[ss_])
                    sp_ = prims[l_index[drawn[ss_]]]
                    new_d[ss_] = (sp_["c0"].astype(F) + u * sp_["radius"].astype(F)[:, None]) - hit_p[ss_]
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
            if mode:
                s = np.nonzero(lamb & ok)[0]
                if len(s):
                    dd, nn, hp = new_d[s], normal[s], hit_p[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    pdf_light = np.zeros(len(s), F)
                    met = np.zeros(len(s), np.int64)          # lights the direction meets (stats only)
                    met_sphere = np.zeros(len(s), np.int64)
                    met_tri = np.zeros(len(s), np.int64)      # §19 (stats only)
                    own_lost = np.zeros(len(s), bool)         # light-half draws whose own sphere gives !(disc > 0): a failed scatter
                    for j in range(n_l):
                        if l_kind[j] == QUAD:
                            q = quads[l_index[j]]
                            qhit, qt = _quad_hit(q, hp, dd)
                            nj = np.broadcast_to(q["normal"].astype(F), dd.shape)
                            pl = ((qt * qt) * len2) / ((np.abs(dot(dd, nj)) / ln) * l_area[j])
                            pdf_light = pdf_light + np.where(qhit, pl, F(0)).astype(F)
                            met += qhit
                        elif l_kind[j] == TRIANGLE:   # §19, to the end of the branch
                            q = quads[l_index[j]]
                            pl, thit = _tri_pl(q, l_area[j], hp, dd, len2, ln)
                            pdf_light = pdf_light + pl
                            met += thit
                            met_tri += thit
                            if stats is not None:
                                stats["tri_own_missed"] += int((to_light[s] & (drawn[s] == j) & ~thit).sum())
                        else:
                            pr = prims[l_index[j]]
                            pl, pos, t1, t2 = T2._sphere_pl(pr["c0"].astype(F), F(pr["radius"]), l_area[j], hp, dd, len2, ln)
                            pdf_light = pdf_light + pl
                            front1, front2 = pos & (t1 > F(0)), pos & (t2 > F(0))
                            own_lost |= to_light[s] & (drawn[s] == j) & ~pos
                            met += front2
                            met_sphere += front2
                            if stats is not None:
                                mine = to_light[s] & (drawn[s] == j)
                                stats["both_roots"] += int((front1 & front2).sum())
                                stats["one_root"] += int((~front1 & front2).sum())
                                stats["no_root"] += int((pos & ~front2).sum())
                                ocj = pr["c0"].astype(F)[None, :] - hp
                                ccj = dot(ocj, ocj) - F(pr["radius"]) * F(pr["radius"])
                                stats["near_surface"] += int(((ccj >= F(0)) & (ccj < F(0.21) * (F(pr["radius"]) * F(pr["radius"])))).sum())
                                stats["disc_nonpos_light_half"] += int((mine & ~pos).sum())
                                stats["far_side_sample"] += int((mine & front1 & front2 & (np.abs(t2 - F(1)) < np.abs(t1 - F(1)))).sum())
                    pdf_light = pdf_light / F(n_l)
                    pdf = F(0.5) * pdf_cos + F(0.5) * pdf_light
                    good = ~(pdf_cos == F(0)) & (pdf > F(0)) & ~own_lost
                    if stats is not None:
                        stats["below_surface"] += int((to_light[s] & (pdf_cos == F(0))).sum())
                        stats["light_half_unmet"] += int((to_light[s] & (met == 0)).sum())
                        stats["cos_one_light"] += int((~to_light[s] & (met == 1)).sum())
                        stats["cos_many_lights"] += int((~to_light[s] & (met >= 2)).sum())
                        stats["sphere_and_other"] += int(((met_sphere >= 1) & (met >= 2)).sum())
                        stats["two_tri_crossings"] += int((met_tri >= 2).sum())   # §19
                        stats["tri_and_other"] += int(((met_tri >= 1) & (met > met_tri)).sum())   # §19
                    ok[s[~good]] = False
                    weight[s[good]] = pdf_cos[good] / pdf[good]
                    weighted[s[good]] = True
            albedo = np.where(weighted[:, None], albedo * weight[:, None], albedo)
            out[r[~ok]] = accum[r[~ok]]
            r, new_d, hit_p, albedo = r[ok], new_d[ok], hit_p[ok], albedo[ok]
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = r
    if stats is not None:
        stats["not_followed"] += int((~followed).sum())
    return out, followed


def frame_samples(world, cam, width, height, spp, max_depth, seed, mode=0, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    rad, ok = radiance(world, cam, width, height, max_depth, seed, gids, smp, mode, stats)
    return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)


luminance, in_order_sums, resolve = T.luminance, T.in_order_sums, T.resolve
