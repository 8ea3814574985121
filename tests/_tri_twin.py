"""A numpy float32 twin of closest intersection and of one whole sample for worlds with TRIANGLES — test infrastructure only.

Nothing here asks the oracle for a closest intersection: the twin is an independent statement of the triangle rule, and the oracle's own (orc_quad::kind) is pinned
to it (tests/test_triangles_cpu.py, pins 3 and 4).  closest_intersection()
walks the flat world itself — RT_WORLD_BVH as BVH::ClosestIntersection does (BVH.cu:54-106: root box, pop, leaf -> primitive, inner -> both child boxes
against rec.distance, near first, push far then near iff dist < rec.distance, no re-check at pop), RT_WORLD_LIST as HittableList.cuh:21-34 (bounds, then every
object in order) — with box decisions from orc_aabb_batch, sphere roots from orc_sphere_batch and the quad test of _nee_twin._quad_hit's arithmetic plus the
caller's rec.distance and the kind rule: kind 1 also rejects alpha + beta > 1 (one fp32 add).  radiance() is the loop of tests/_path_twin.py with that walk in
the place of orc_trace_batch and _nee2_twin's light table over the parallelograms alone; first_hit_sums() is the feature pass's sums under any walk.

It is pinned before anything is compared with it (tests/test_triangles_cpu.py): on worlds without triangles closest_intersection() equals orc_trace_batch in
hit, t, primitive and normal on every ray, and radiance() equals orc_radiance_batch (mode 0) and _nee2_twin (modes 1, 2), bit for bit.  After the pins the
only thing the twin adds is the interior rule.

Scope: stack traversal; spheres static or moving (the centre at the ray's time); a sphere of RT_MAT_ISOTROPIC as a constant medium when the caller hands the walk
the tape, as a plain sphere otherwise.  radiance() here follows _nee_twin's materials under the pinhole camera.
"""
import ctypes as C

import numpy as np

import _nee2_twin as T2
import _nee_twin as T
import _oracle as O
import _path_twin as PT
from _nee2_twin import world_arrays
from _nee_twin import F, MISS, PRIM_MOVING, cross, dot


MAT_ISOTROPIC = 5


def _log(x):
    """the project's deterministic log (orc_math_batch fn 0 = rt_logf)"""
    x = np.ascontiguousarray(x, F)
    out = np.zeros(len(x), F)
    O.lib().orc_math_batch(0, len(x), x, x, out)
    return out


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


def _leaf(prims, quads, idx, o, d, rec_t, rec_prim, rec_n, rows, time=None, media=None):
    """any_prim_closest_intersection of primitive idx[i] on ray rows[i], against the caller's rec.distance; updates the records in place.  time: the rays' times, for
    a moving sphere's centre; media = (material types, material params, tape, the tape's row of every ray, info): a sphere of RT_MAT_ISOTROPIC is then the constant
    medium of prim_closest_intersection (rt_oracle.c:295-322), which draws its uniform from the tape; None: a sphere of any material is a sphere"""
    n_prims = len(prims)
    with np.errstate(all="ignore"):
        sp = idx < n_prims
        if sp.any():
            r, pr, pi = rows[sp], prims[idx[sp]], idx[sp]
            c, rad = pr["c0"].astype(F), pr["radius"].astype(F)
            mov = (pr["mat"] & np.uint32(PRIM_MOVING)) != 0
            if mov.any():   # glm::mix(c0, c1, time) = c0 * (1 - time) + c1 * time
                tm = time[r[mov]][:, None]
                c[mov] = pr["c0"][mov].astype(F) * (F(1) - tm) + pr["c1"][mov].astype(F) * tm
            med = np.zeros(len(r), bool)
            if media is not None:
                m_type, m_param, tape, tape_rows, info = media
                mat = (pr["mat"] & ~np.uint32(PRIM_MOVING)).astype(np.int64)
                med = m_type[mat] == MAT_ISOTROPIC
            if med.any():
                rm, cm, radm = r[med], c[med], rad[med]
                oc = o[rm] - cm
                a = dot(d[rm], d[rm])
                hb = dot(d[rm], oc)
                cc = dot(oc, oc) - radm * radm
                disc = hb * hb - a * cc
                sq = np.sqrt(disc)
                t1, t2 = (-hb - sq) / a, (-hb + sq) / a
                t_in = np.where(t1 < F(0), F(0), t1).astype(F)
                t_out = np.where(t2 > rec_t[rm], rec_t[rm], t2).astype(F)
                draws = np.nonzero(~(disc <= F(0)) & (t_in < t_out))[0]   # a non-empty interval inside the boundary: ONE uniform, whatever becomes of the test
                if len(draws):
                    rd = rm[draws]
                    u = tape.next(tape_rows[rd])
                    ray_length = np.sqrt(a[draws])
                    inside = (t_out[draws] - t_in[draws]) * ray_length
                    hit_distance = (F(-1) / m_param[mat[med][draws]]) * _log(u)
                    tmed = t_in[draws] + hit_distance / ray_length
                    ok = ~(hit_distance > inside) & ~(tmed >= rec_t[rd])
                    rec_t[rd[ok]], rec_prim[rd[ok]] = tmed[ok], pi[med][draws][ok]
                    rec_n[rd[ok]] = np.array([1, 0, 0], F)
                    if info is not None:
                        info["medium_draws"] = info.get("medium_draws", 0) + len(rd)
                        info["medium_hits"] = info.get("medium_hits", 0) + int(ok.sum())
                        if "after_medium" in info:   # a test's hook: (tape, the tape's rows that drew, which of the tests accepted)
                            info["after_medium"](tape, tape_rows[rd], ok)
                r, pi, c, rad = r[~med], pi[~med], c[~med], rad[~med]
            if len(r):
                rays = np.ascontiguousarray(np.concatenate([o[r], d[r]], axis=1), F)
                t = np.zeros(len(r), F)
                O.lib().orc_sphere_batch(len(r), rays, np.ascontiguousarray(np.concatenate([c, rad[:, None]], axis=1), F), t)
                ok = ~(t >= rec_t[r])
                r, t, c, rad = r[ok], t[ok], c[ok], rad[ok]
                rec_t[r], rec_prim[r] = t, pi[ok]
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


def closest_intersection(world, rays, preset=None, tape=None, rows=None, medium_info=None):
    """Hittable::ClosestIntersection of the flat world on rays (n, 7): (hit int32, t, prim int32, normal), laid out as orc_trace_batch lays them out
    (a miss: t = the rec.distance it started with, prim = -1, normal = 0).  preset: rec.distance before the walk (default: a fresh record's MISS).  A moving
    sphere stands where rays[:, 6], the ray's time, puts it.  tape, rows: the tape of the samples' uniforms and the row of it that serves each ray — given
    them, a sphere of RT_MAT_ISOTROPIC is a constant medium and draws from its ray's row, in traversal order; a world without a medium never touches the tape.
    Without them such a sphere is a sphere, as it was before the twin knew media.  medium_info (a dict): 'medium_draws' and 'medium_hits' grow."""
    prims, quads, mats = world_arrays(world)
    assert world.traversal == 0, "stack traversal"
    n = len(rays)
    time = np.ascontiguousarray(rays[:, 6], F)
    media = None
    if tape is not None and (mats["type"] == MAT_ISOTROPIC).any():
        media = (mats["type"].astype(np.int64), mats["param"].astype(F), tape, np.asarray(rows, np.int64), medium_info)
    o, d = np.ascontiguousarray(rays[:, 0:3], F), np.ascontiguousarray(rays[:, 3:6], F)
    rec_t = np.full(n, MISS, F) if preset is None else np.array(preset, F)
    rec_prim, rec_n = np.full(n, -1, np.int64), np.zeros((n, 3), F)
    if world.kind == 1:   # HittableList.cuh:21-34
        bmn, bmx = np.array(list(world.bounds_min), F), np.array(list(world.bounds_max), F)
        inside, _ = _boxes_hit(np.broadcast_to(bmn, (n, 3)), np.broadcast_to(bmx, (n, 3)), o, d, rec_t)
        idx = np.nonzero(inside)[0]
        for i in range(world.n_prims + world.n_quads):
            _leaf(prims, quads, np.full(len(idx), i, np.int64), o, d, rec_t, rec_prim, rec_n, idx, time, media)
    else:
        assert world.kind == 0
        nodes = np.frombuffer((C.c_char * (world.n_nodes * O.NODE_DT.itemsize)).from_address(world.nodes), O.NODE_DT)
        stack, head = np.zeros((n, 33), np.int64), np.zeros(n, np.int64)
        root = nodes[world.root]
        inside, _ = _boxes_hit(np.broadcast_to(root["min"], (n, 3)), np.broadcast_to(root["max"], (n, 3)), o, d, rec_t)
        stack[inside, 0], head[inside] = world.root, 1
        while True:
            live = np.nonzero(head > 0)[0]
            if len(live) == 0:
                break
            head[live] -= 1
            node = nodes[stack[live, head[live]]]
            leaf = node["left"] == -1
            if leaf.any():
                _leaf(prims, quads, node["right"][leaf].astype(np.int64), o, d, rec_t, rec_prim, rec_n, live[leaf], time, media)
            r = live[~leaf]
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
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 as rt_renderer_light_sampling_enable takes it"""
    return T2.table_radiance(world, cam, width, height, max_depth, seed, gids, samples, mode, PT.counters(stats, T2.new_stats()), closest_intersection, lights_of,
                             (0, 1, 2))   # parallelograms only: a triangle light emits and is in no table


def frame_samples(world, cam, width, height, spp, max_depth, seed, mode=0, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, mode, stats), width, height, spp, first_sample)


luminance, in_order_sums, resolve = T.luminance, T.in_order_sums, T.resolve


def first_hit_sums(world, cam, width, height, spp, seed, first_sample=0, trace=closest_intersection):
    """What the feature pass accumulates of the primary rays' first hits by the walk `trace`, in sample order: (H, W, 5) float32 = (sum Nx, sum Ny, sum Nz,
    sum t, hits)"""
    _, ray_o, ray_d = PT.primary_rays(cam, width, height, seed, *PT.keys(width, height, spp, first_sample))
    with np.errstate(all="ignore"):
        rays = np.zeros((len(ray_o), 7), F)
        rays[:, 0:3], rays[:, 3:6] = ray_o, ray_d
        hit, t, _, normal = trace(world, rays)
        per = np.concatenate([normal, t[:, None], hit[:, None].astype(F)], axis=1).reshape(height, width, spp, 5)
        sums = np.zeros((height, width, 5), F)
        for s in range(spp):
            sums = sums + np.where(per[:, :, s, 4:5] > 0, per[:, :, s, :], F(0))
    return sums
