"""The numpy float32 twin of one whole sample for light sampling over quad AND sphere lights (mode 2) — test infrastructure only.

tests/_nee_twin.py restates §16 (quad lights) and stays as it is; this module has a radiance() of its own that knows both kinds of light and takes
a `mode`: 0 = sampling off, 1 = §16's quad lights, 2 = §17's table (the quad lights, then the static sphere lights).  The tape of uniforms, the
quad test and the vector helpers are _nee_twin's; every closest intersection still comes from orc_trace_batch, which hits emitting spheres as it hits
any other.  tests/test_light_sampling_spheres_cpu.py pins it — mode 0 to orc_radiance_batch, mode 1 to _nee_twin, bit for bit — before anything is
compared with it.

Scope: _nee_twin's (pinhole cameras; spheres and quads with Lambertian, checker, metal and diffuse-light materials).
"""
import ctypes as C

import numpy as np

import _nee_twin as T
import _oracle as O
from _nee_twin import F, INV_PI, MAX_LIGHTS, PRIM_MOVING, _quad_hit, _Tape, dot, near_zero

QUAD, SPHERE = 0, 1
FOUR_PI = F(12.566371)
MAT_DIFFUSE_LIGHT = 4


def sphere_lights(prims, mats):
    """(primitive indices, areas): the static spheres with radius > 0 whose material is a diffuse light, in primitive order;
    area = (12.566371f * r) * r"""
    idx = [i for i in range(len(prims)) if not (int(prims["mat"][i]) & PRIM_MOVING) and prims["radius"][i] > 0 and mats["type"][int(prims["mat"][i])] == MAT_DIFFUSE_LIGHT]
    idx = np.array(idx, dtype=np.uint32)
    r = prims["radius"][idx].astype(F) if len(idx) else np.zeros(0, F)
    return idx, ((FOUR_PI * r) * r).astype(F)


def lights_of(prims, quads, mats, mode):
    """(kind, index, area) of the light table of `mode`: the quad lights as §16 lists them, then (mode 2) the sphere lights"""
    q_idx, q_area = T.quad_lights(quads, mats)
    kind, index, area = [QUAD] * len(q_idx), list(q_idx), list(q_area)
    if mode == 2:
        s_idx, s_area = sphere_lights(prims, mats)
        kind, index, area = kind + [SPHERE] * len(s_idx), index + list(s_idx), area + list(s_area)
    return np.array(kind, np.int64), np.array(index, np.int64), np.array(area, F)


def world_arrays(world):
    prims = np.frombuffer((C.c_char * (world.n_prims * O.PRIM_DT.itemsize)).from_address(world.prims), O.PRIM_DT) if world.n_prims else np.zeros(0, O.PRIM_DT)
    quads = np.frombuffer((C.c_char * (world.n_quads * O.QUAD_DT.itemsize)).from_address(world.quads), O.QUAD_DT) if world.n_quads else np.zeros(0, O.QUAD_DT)
    mats = np.frombuffer((C.c_char * (world.n_materials * O.MAT_DT.itemsize)).from_address(world.materials), O.MAT_DT)
    return prims, quads, mats


def new_stats():
    """_nee_twin's counters (light_samples[i] counts both kinds), and for sphere lights, per evaluated (direction, sphere light) pair or light-half draw:
    both_roots: the line meets the sphere twice in front of the hit point (two summands); one_root: only the far crossing is in front (the hit
    point is inside the sphere); no_root: disc > 0 but both crossings behind; disc_nonpos_light_half: a light-half draw whose OWN sphere gives
    disc <= 0 (a silhouette point, lost to rounding: the path ends like a failed scatter); far_side_sample: a light-half draw whose sampled point is the far crossing (t2 is the
    root nearer 1); near_surface: the hit point lies outside the sphere and within a tenth of its radius of its surface (0 <= cc < 0.21 r^2, as beside the point where a
    light touches a wall: the light fills nearly half the sky and cc is what cancellation leaves); sphere_light_half: light-half draws sent to a sphere light; sphere_and_other: directions that meet a sphere light and at least one more light (a pl of two or more terms)"""
    st = T.new_stats()
    st.update({"both_roots": 0, "one_root": 0, "no_root": 0, "disc_nonpos_light_half": 0, "far_side_sample": 0, "sphere_and_other": 0, "sphere_light_half": 0, "near_surface": 0})
    return st


def _sphere_pl(center, r, area, hp, dd, len2, ln):
    """§17's density of one sphere light along rays (hp, dd): (pl_j, disc > 0, t1, t2)"""
    oc = center[None, :] - hp
    h = dot(dd, oc)
    cr = T.cross(oc, dd)
    disc = (r * r) * len2 - dot(cr, cr)
    pos = disc > F(0)
    sq = np.sqrt(np.where(pos, disc, F(0)).astype(F))
    cosl = (sq / r) / ln
    den = cosl * area
    t1 = (h - sq) / len2
    t2 = (h + sq) / len2
    pl = np.zeros(len(hp), F)
    pl = np.where(pos & (t1 > F(0)), pl + ((t1 * t1) * len2) / den, pl).astype(F)
    pl = np.where(pos & (t2 > F(0)), pl + ((t2 * t2) * len2) / den, pl).astype(F)
    return pl, pos, t1, t2


def radiance(world, cam, width, height, max_depth, seed, gids, samples, mode=0, stats=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 as rt_renderer_light_sampling_enable takes it"""
    assert cam.type == 0, "the twin restates the pinhole camera"
    assert mode in (0, 1, 2)
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    l_kind, l_index, l_area = lights_of(prims, quads, mats, mode)
    n_l = len(l_kind)
    if mode:
        assert 1 <= n_l <= MAX_LIGHTS
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)

    if stats is not None:
        for key, zero in new_stats().items():
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
            hit, t, prim, normal = np.zeros(k, np.int32), np.zeros(k, F), np.zeros(k, np.int32), np.zeros((k, 3), F)
            assert O.lib().orc_trace_batch(C.byref(world), k, rays, hit, t, prim, normal) == 0
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
                    stats["light_samples"] += np.bincount(li, minlength=MAX_LIGHTS)
                    stats["checker_light_half"] += int((mt[s] == 3).sum())
                    stats["sphere_light_half"] += int((l_kind[li] == SPHERE).sum())
                sq_, ss_ = s[l_kind[li] == QUAD], s[l_kind[li] == SPHERE]
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
                    own_lost = np.zeros(len(s), bool)         # light-half draws whose own sphere gives !(disc > 0): a failed scatter
                    for j in range(n_l):
                        if l_kind[j] == QUAD:
                            q = quads[l_index[j]]
                            qhit, qt = _quad_hit(q, hp, dd)
                            nj = np.broadcast_to(q["normal"].astype(F), dd.shape)
                            pl = ((qt * qt) * len2) / ((np.abs(dot(dd, nj)) / ln) * l_area[j])
                            pdf_light = pdf_light + np.where(qhit, pl, F(0)).astype(F)
                            met += qhit
                        else:
                            pr = prims[l_index[j]]
                            pl, pos, t1, t2 = _sphere_pl(pr["c0"].astype(F), F(pr["radius"]), l_area[j], hp, dd, len2, ln)
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
