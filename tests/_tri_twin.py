"""A numpy float32 twin of closest intersection and of one whole sample for worlds with TRIANGLES — test infrastructure only.

Nothing here asks the oracle for a closest intersection: the twin is an independent statement of the triangle rule, and the oracle's own (orc_quad::kind) is pinned
to it (tests/test_triangles_cpu.py, pins 3 and 4).  closest_intersection()
walks the flat world itself — RT_WORLD_BVH as BVH::ClosestIntersection does (BVH.cu:54-106: root box, pop, leaf -> primitive, inner -> both child boxes
against rec.distance, near first, push far then near iff dist < rec.distance, no re-check at pop), RT_WORLD_LIST as HittableList.cuh:21-34 (bounds, then every
object in order) — with box decisions from orc_aabb_batch, sphere roots from orc_sphere_batch and the quad test of _nee_twin._quad_hit's arithmetic plus the
caller's rec.distance and the kind rule: kind 1 also rejects alpha + beta > 1 (one fp32 add).  radiance() is _nee2_twin.radiance with that walk in the place of
orc_trace_batch and a light table that leaves triangles out.

It is pinned before anything is compared with it (tests/test_triangles_cpu.py): on worlds without triangles closest_intersection() equals orc_trace_batch in
hit, t, primitive and normal on every ray, and radiance() equals orc_radiance_batch (mode 0) and _nee2_twin (modes 1, 2), bit for bit.  After the pins the
only thing the twin adds is the interior rule.

radiance() below is a COPY of _nee2_twin.radiance (the older twins stay untouched, so it cannot be a call with a hook): all but the two marked lines are its text.
Nothing but pin 2 ties the two together — whoever changes _nee2_twin.radiance mirrors the change here, and the pin fails until that is done.

Scope: _nee_twin's (pinhole cameras; Lambertian, checker, metal and diffuse-light materials) and static spheres; stack traversal.
"""
import ctypes as C

import numpy as np

import _nee2_twin as T2
import _nee_twin as T
import _oracle as O
from _nee2_twin import QUAD, SPHERE, MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, MAX_LIGHTS, MISS, PRIM_MOVING, _Tape, cross, dot, near_zero

_quad_hit = T._quad_hit   # the density step's per-light test: a light of the table is a parallelogram


def kinds(quads):
    """rt_quad::kind of every record"""
    return quads["kind"]


def lights_of(prims, quads, mats, mode):
    """_nee2_twin.lights_of over the parallelograms: the triangles follow them in a flat world, so the quad indices stay what they are"""
    k = kinds(quads)
    n_plain = int((k == 0).sum())
    assert (k[:n_plain] == 0).all() and (k[n_plain:] == 1).all(), "the triangles follow the parallelograms"
    return T2.lights_of(prims, quads[:n_plain], mats, mode)


def _boxes_hit(mn, mx, o, d, maxd):
    """aabb::intersects per row through orc_aabb_batch: (hit bool, dist float32; MISS where not hit)"""
    n = len(o)
    boxes = np.ascontiguousarray(np.concatenate([mn, mx], axis=1), F)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), F)
    hit, dist = np.zeros(n, np.int32), np.zeros(n, F)
    O.lib().orc_aabb_batch(n, boxes, rays, np.ascontiguousarray(maxd, F), hit, dist)
    return hit != 0, np.where(hit != 0, dist, MISS).astype(F)


def _leaf(prims, quads, idx, o, d, rec_t, rec_prim, rec_n, rows):
    """any_prim_closest_intersection of primitive idx[i] on ray rows[i], against the caller's rec.distance; updates the records in place"""
    n_prims = len(prims)
    with np.errstate(all="ignore"):
        sp = idx < n_prims
        if sp.any():
            r, pr = rows[sp], prims[idx[sp]]
            c, rad = pr["c0"].astype(F), pr["radius"].astype(F)
            rays = np.ascontiguousarray(np.concatenate([o[r], d[r]], axis=1), F)
            t = np.zeros(len(r), F)
            O.lib().orc_sphere_batch(len(r), rays, np.ascontiguousarray(np.concatenate([c, rad[:, None]], axis=1), F), t)
            ok = ~(t >= rec_t[r])
            r, t, c, rad = r[ok], t[ok], c[ok], rad[ok]
            rec_t[r], rec_prim[r] = t, idx[sp][ok]
            rec_n[r] = ((o[r] + d[r] * t[:, None]) - c) / rad[:, None]
        qd = ~sp
        if qd.any():
            r, q, ui = rows[qd], quads[idx[qd] - n_prims], idx[qd]
            oo, dd = o[r], d[r]
            nrm, w, u, v = q["normal"].astype(F), q["w"].astype(F), q["u"].astype(F), q["v"].astype(F)
            denom = dot(nrm, dd)
            t = (q["D"].astype(F) - dot(nrm, oo)) / denom
            ok = ~(np.abs(denom) < F(1e-8)) & ~(t < F(0)) & ~(t >= rec_t[r])
            planar = (oo + dd * t[:, None]) - q["Q"].astype(F)
            alpha = dot(w, cross(planar, v))
            beta = dot(w, cross(u, planar))
            ok &= (alpha >= F(0)) & (alpha <= F(1)) & (beta >= F(0)) & (beta <= F(1))
            ok &= ~((kinds(q) == 1) & ~((alpha + beta) <= F(1)))   # the kind rule: all this twin adds
            r, t, nrm, dd, ui = r[ok], t[ok], nrm[ok], dd[ok], ui[ok]
            rec_t[r], rec_prim[r] = t, ui
            rec_n[r] = np.where((dot(dd, nrm) > F(0))[:, None], -nrm, nrm)


def closest_intersection(world, rays, preset=None):
    """Hittable::ClosestIntersection of the flat world on rays (n, 7): (hit int32, t, prim int32, normal), laid out as orc_trace_batch lays them out
    (a miss: t = the rec.distance it started with, prim = -1, normal = 0).  preset: rec.distance before the walk (default: a fresh record's MISS)."""
    prims, quads, _ = world_arrays(world)
    assert not (prims["mat"] & np.uint32(PRIM_MOVING)).any() and world.traversal == 0, "static spheres, stack traversal"
    n = len(rays)
    o, d = np.ascontiguousarray(rays[:, 0:3], F), np.ascontiguousarray(rays[:, 3:6], F)
    rec_t = np.full(n, MISS, F) if preset is None else np.array(preset, F)
    rec_prim, rec_n = np.full(n, -1, np.int64), np.zeros((n, 3), F)
    if world.kind == 1:   # HittableList.cuh:21-34
        bmn, bmx = np.array(list(world.bounds_min), F), np.array(list(world.bounds_max), F)
        inside, _ = _boxes_hit(np.broadcast_to(bmn, (n, 3)), np.broadcast_to(bmx, (n, 3)), o, d, rec_t)
        rows = np.nonzero(inside)[0]
        for i in range(world.n_prims + world.n_quads):
            _leaf(prims, quads, np.full(len(rows), i, np.int64), o, d, rec_t, rec_prim, rec_n, rows)
    else:
        assert world.kind == 0
        nodes = np.frombuffer((C.c_char * (world.n_nodes * O.NODE_DT.itemsize)).from_address(world.nodes), O.NODE_DT)
        stack, head = np.zeros((n, 33), np.int64), np.zeros(n, np.int64)
        root = nodes[world.root]
        inside, _ = _boxes_hit(np.broadcast_to(root["min"], (n, 3)), np.broadcast_to(root["max"], (n, 3)), o, d, rec_t)
        stack[inside, 0], head[inside] = world.root, 1
        while True:
            rows = np.nonzero(head > 0)[0]
            if len(rows) == 0:
                break
            head[rows] -= 1
            node = nodes[stack[rows, head[rows]]]
            leaf = node["left"] == -1
            if leaf.any():
                _leaf(prims, quads, node["right"][leaf].astype(np.int64), o, d, rec_t, rec_prim, rec_n, rows[leaf])
            r = rows[~leaf]
            if len(r):
                li, ri = node["left"][~leaf].astype(np.int64), node["right"][~leaf].astype(np.int64)
                _, ld = _boxes_hit(nodes["min"][li], nodes["max"][li], o[r], d[r], rec_t[r])
                _, rd = _boxes_hit(nodes["min"][ri], nodes["max"][ri], o[r], d[r], rec_t[r])
                swap = ld > rd
                near_i, far_i = np.where(swap, ri, li), np.where(swap, li, ri)
                near_d, far_d = np.where(swap, rd, ld), np.where(swap, ld, rd)
                pf = far_d < rec_t[r]
                stack[r[pf], head[r[pf]]] = far_i[pf]
                head[r[pf]] += 1
                pn = near_d < rec_t[r]
                stack[r[pn], head[r[pn]]] = near_i[pn]
                head[r[pn]] += 1
    hit = rec_prim >= 0
    return hit.astype(np.int32), rec_t, rec_prim.astype(np.int32), rec_n


def radiance(world, cam, width, height, max_depth, seed, gids, samples, mode=0, stats=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 as rt_renderer_light_sampling_enable takes it.
    _nee2_twin.radiance statement by statement, but for the two lines marked below."""
    assert cam.type == 0, "the twin restates the pinhole camera"
    assert mode in (0, 1, 2)
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    l_kind, l_index, l_area = lights_of(prims, quads, mats, mode)   # parallelograms only: a triangle light emits and is in no table
    n_l = len(l_kind)
    if mode:
        assert 1 <= n_l <= MAX_LIGHTS
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)

    if stats is not None:
        for key, zero in T2.new_stats().items():
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


def first_hit_sums(world, cam, width, height, spp, seed, first_sample=0):
    """What the feature pass accumulates of the primary rays' first hits, in sample order: (H, W, 5) float32 = (sum Nx, sum Ny, sum Nz, sum t, hits)"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    tape = _Tape(seed, gids, smp)
    n = len(gids)
    with np.errstate(all="ignore"):
        x, y = (gids % np.uint32(width)).astype(F), (gids // np.uint32(width)).astype(F)
        psx, psy = F(1) / F(width), F(1) / F(height)
        ndcx = ((x + F(0.5)) * psx) * F(2) - F(1)
        ndcy = ((y + F(0.5)) * psy) * F(2) - F(1)
        jx, jy = tape.in_unit2(np.arange(n))
        sx, sy = ndcx + jx * psx, ndcy + jy * psy
        co, cu, cv, cw = (np.array(list(v), F) for v in (cam.o, cam.u, cam.v, cam.w))
        rays = np.zeros((n, 7), F)
        rays[:, 0:3] = co
        rays[:, 3:6] = (cw[None, :] + cu[None, :] * sx[:, None]) + cv[None, :] * sy[:, None]
        hit, t, _, normal = closest_intersection(world, rays)
        per = np.concatenate([normal, t[:, None], hit[:, None].astype(F)], axis=1).reshape(height, width, spp, 5)
        sums = np.zeros((height, width, 5), F)
        for s in range(spp):
            sums = sums + np.where(per[:, :, s, 4:5] > 0, per[:, :, s, :], F(0))
    return sums
