"""A numpy float32 twin of the cutout rule and of the walk that applies it — test infrastructure only.

keeps() restates cutout_keeps (csrc/rt_device_funcs.hpp; include/rt06.h: rt_scene_set_cutout) from the pieces the other twins pin: the hit point and the
coordinates of _uv_twin (planar() on a parallelogram and on a triangle without a table of coordinates, tri_uv() under one), the texel of _tex_twin.lookup(), and
the comparison !(green < cutoff).  keeps64() is the same decision in float64, sharing no float32 code with anything.

closest_intersection() is a walk of its own: _tri_twin.closest_intersection's loops — the list in order, the flat BVH by the stack — calling _tri_twin._leaf one
leaf at a time.  A hit that _leaf has just taken on a parallelogram or triangle whose material's record is on is put to the rule, and taken BACK when the rule
turns it down: the three records of that row (distance, primitive, normal) get the values they had before the leaf, so every later box test and leaf test
sees the distance the kernel's lane sees.  The walk counts what it does.  walk_of() hands it out in the shape _path_twin.radiance takes a walk in;
_interior_twin.solid_walk wraps it like any other.
"""
import ctypes as C

import numpy as np

import _oracle as O
import _tex_twin as XT
import _tri_twin as TT
import _uv_twin as UT
from _nee2_twin import world_arrays
from _nee_twin import F, MISS

CUTOUT_DT = np.dtype([("on", "<u4"), ("image", "<u4"), ("cutoff", "<f4"), ("reserved", "<u4")])
OFF, MASKED = 0, 1
COUNTERS = ("tested", "kept", "rejected", "rejected_quad", "rejected_tri_uv", "rejected_tri_plain", "rejected_deep", "then_farther", "then_miss", "then_nearer")


def new_stats():
    return {name: 0 for name in COUNTERS}


def coords(quads, uv, o, d, t):
    """(u, v) (n, 2) of candidate i at distance t[i] on record quads[i]: the rule of rt_tri_uvs under uv[i] (3, 2), the planar coordinates when uv is None"""
    if uv is not None:
        return UT.tri_uv(quads, uv, o, d, t)
    a, b = UT.planar(quads, o, d, t)
    return np.stack([a, b], axis=1).astype(F)


def keeps(table, quads, uv, o, d, t, records, material):
    """rt_cutout_batch: table = [(image, wrap, filter), ...]; per case its record quads[i], its coordinates uv[i] or uv = None, the ray, the distance and
    material[i], an index into records (CUTOUT_DT) -> (keep uint32, uv (n, 2), value (n,)); zeros and keep = 1 where the record is off"""
    material = np.asarray(material, np.int64).reshape(-1)
    rec = np.asarray(records)[material]
    n = len(material)
    keep, out_uv, value = np.ones(n, np.uint32), np.zeros((n, 2), F), np.zeros(n, F)
    on = np.nonzero(rec["on"] != OFF)[0]
    if len(on):
        o, d, t = (np.ascontiguousarray(a, F) for a in (o, d, t))
        tuv = coords(quads[on], None if uv is None else UT.table(uv)[on], o[on], d[on], t[on])
        with np.errstate(all="ignore"):
            c = XT.lookup(table, rec["image"][on], tuv[:, 0], tuv[:, 1])
            keep[on] = ~(c[:, 1] < rec["cutoff"][on].astype(F))
        out_uv[on], value[on] = tuv, c[:, 1]
    return keep, out_uv, value


def keeps64(image, wrap, Q, u, v, t0, t1, t2, o, d, t, cutoff):
    """the decision in float64 under a bilinear mask: (keep bool, uv (n, 2), value (n,)) — w from u and v, the point from the ray, the formula of value64"""
    hit_p = np.asarray(o, np.float64) + np.asarray(d, np.float64) * np.asarray(t, np.float64)[:, None]
    tuv = UT.tri_uv64(Q, u, v, t0, t1, t2, hit_p)
    value = XT.value64(image, wrap, tuv[:, 0], tuv[:, 1])[:, 1]
    return ~(value < np.asarray(cutoff, np.float64)), tuv, value


LIVE_COUNTERS = ("hole_then_moving", "hole_then_medium_draw", "hole_then_solid", "kept_image_masked", "kept_mapped_masked", "kept_smooth_masked", "mask_uv_is_shade_uv")
NOT_TAKEN_BACK, MASK_AT_PLANAR = "a rejected candidate keeps its distance", "the mask is read at the planar coordinates"   # the deliberately wrong walks (`wrong`)


def closest_intersection(world, uv, cutouts, table, rays, preset=None, stats=None, eye=None, tape=None, rows=None, medium_info=None, marks=None, wrong=None):
    """_tri_twin.closest_intersection under the rule: (hit int32, t, prim int32, normal).  uv: the renderer's table of texture coordinates or None; cutouts: one
    record of CUTOUT_DT per material; table: the texture table [(image, wrap, filter), ...]; stats: new_stats()'s counters grow; eye: the camera's position —
    a rejection on a ray that does not start there counts as deep.  marks (a dict, with stats): what the walk does not know of the world — 'solid' and 'mapped'
    (bool per material: an interior record, a normal-map record), 'smooth' (bool per triangle: vertex normals) — under which LIVE_COUNTERS are counted (DESIGN.md
    §36), and which gets 'masked_image' back: (rows, bool) — the rays of this call whose hit is on a masked image material.  wrong: NOT_TAKEN_BACK or
    MASK_AT_PLANAR — a walk that is WRONG on purpose, for the tests that show a frame would notice."""
    prims, quads, mats = world_arrays(world)
    assert world.traversal == 0, "stack traversal"
    n, n_prims = len(rays), len(prims)
    first_tri = n_prims + int((quads["kind"] == 0).sum())
    tab = UT.table(uv) if uv is not None and len(uv) else None
    on_of_quad = cutouts["on"][quads["mat"].astype(np.int64)] != OFF if len(quads) else np.zeros(0, bool)
    time = np.ascontiguousarray(rays[:, 6], F)
    media = None
    if tape is not None and (mats["type"] == TT.MAT_ISOTROPIC).any():
        media = (mats["type"].astype(np.int64), mats["param"].astype(F), tape, np.asarray(rows, np.int64), medium_info)
    o, d = np.ascontiguousarray(rays[:, 0:3], F), np.ascontiguousarray(rays[:, 3:6], F)
    rec_t = np.full(n, MISS, F) if preset is None else np.array(preset, F)
    rec_prim, rec_n = np.full(n, -1, np.int64), np.zeros((n, 3), F)
    nearest_hole = np.full(n, np.inf, np.float64)   # the smallest distance at which the rule turned a candidate of this ray down
    deep = np.zeros(n, bool) if eye is None else (o != np.asarray(eye, F)[None, :]).any(axis=1)

    def leaf(idx, at):
        before = rec_t[at].copy(), rec_prim[at].copy(), rec_n[at].copy()
        cur0 = tape.cur[media[3][at]].copy() if media is not None and marks is not None else None
        TT._leaf(prims, quads, idx, o, d, rec_t, rec_prim, rec_n, at, time, media)
        if cur0 is not None and stats is not None:   # a medium drew on a ray that had been through a hole
            stats["hole_then_medium_draw"] = stats.get("hole_then_medium_draw", 0) + int(((tape.cur[media[3][at]] > cur0) & np.isfinite(nearest_hole[at])).sum())
        quad = idx >= n_prims
        took = quad & (rec_prim[at] == idx) & (before[1] != idx)
        took[took] = on_of_quad[idx[took] - n_prims]
        c = np.nonzero(took)[0]
        if len(c) == 0:
            return
        r, qi = at[c], idx[c] - n_prims
        under_table = (idx[c] >= first_tri) & (tab is not None) & (wrong != MASK_AT_PLANAR)
        keep = np.ones(len(c), bool)
        for sel, tuv in ((under_table, True), (~under_table, False)):
            if sel.any():
                coords_of = tab[idx[c][sel] - first_tri] if tuv else None
                keep[sel] = keeps(table, quads[qi[sel]], coords_of, o[r[sel]], d[r[sel]], rec_t[r[sel]], cutouts, quads["mat"][qi[sel]])[0] != 0
        rej = ~keep
        if stats is not None:
            plain_tri = idx[c] >= first_tri   # a triangle on the planar coordinates: no table, or the identity record of a mesh that was given none
            if tab is not None:
                plain_tri = plain_tri & (tab[np.where(plain_tri, idx[c] - first_tri, 0)] == UT.IDENTITY).all(axis=(1, 2))
            stats["tested"] += len(c)
            stats["kept"] += int(keep.sum())
            stats["rejected"] += int(rej.sum())
            stats["rejected_quad"] += int((rej & (idx[c] < first_tri)).sum())
            stats["rejected_tri_uv"] += int((rej & (idx[c] >= first_tri) & ~plain_tri).sum())
            stats["rejected_tri_plain"] += int((rej & plain_tri).sum())
            stats["rejected_deep"] += int((rej & deep[r]).sum())
        back = r[rej]
        nearest_hole[back] = np.minimum(nearest_hole[back], rec_t[back].astype(np.float64))
        if wrong != NOT_TAKEN_BACK:
            rec_t[back] = before[0][c][rej]
        rec_prim[back], rec_n[back] = before[1][c][rej], before[2][c][rej]   # the hit is taken back: the lane never took it

    if world.kind == 1:   # HittableList.cuh:21-34
        bmn, bmx = np.array(list(world.bounds_min), F), np.array(list(world.bounds_max), F)
        inside, _ = TT._boxes_hit(np.broadcast_to(bmn, (n, 3)), np.broadcast_to(bmx, (n, 3)), o, d, rec_t)
        idx = np.nonzero(inside)[0]
        for i in range(world.n_prims + world.n_quads):
            leaf(np.full(len(idx), i, np.int64), idx)
    else:
        assert world.kind == 0
        nodes = np.frombuffer((C.c_char * (world.n_nodes * O.NODE_DT.itemsize)).from_address(world.nodes), O.NODE_DT)
        stack, head = np.zeros((n, 33), np.int64), np.zeros(n, np.int64)
        root = nodes[world.root]
        inside, _ = TT._boxes_hit(np.broadcast_to(root["min"], (n, 3)), np.broadcast_to(root["max"], (n, 3)), o, d, rec_t)
        stack[inside, 0], head[inside] = world.root, 1
        while True:
            live = np.nonzero(head > 0)[0]
            if len(live) == 0:
                break
            head[live] -= 1
            node = nodes[stack[live, head[live]]]
            is_leaf = node["left"] == -1
            if is_leaf.any():
                leaf(node["right"][is_leaf].astype(np.int64), live[is_leaf])
            r = live[~is_leaf]
            if len(r):
                li, ri = node["left"][~is_leaf].astype(np.int64), node["right"][~is_leaf].astype(np.int64)
                _, ld = TT._boxes_hit(nodes["min"][li], nodes["max"][li], o[r], d[r], rec_t[r])
                _, rd = TT._boxes_hit(nodes["min"][ri], nodes["max"][ri], o[r], d[r], rec_t[r])
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
    if stats is not None:
        holed = np.isfinite(nearest_hole)
        stats["then_farther"] += int((holed & hit & (rec_t.astype(np.float64) > nearest_hole)).sum())
        stats["then_nearer"] += int((holed & hit & ~(rec_t.astype(np.float64) > nearest_hole)).sum())
        stats["then_miss"] += int((holed & ~hit).sum())
        if marks is not None:
            _live_counters(world, uv, cutouts, table, rays, stats, marks, holed, hit, rec_t, rec_prim, rec_n, rows, (prims, quads, mats, tab, first_tri, on_of_quad))
    return hit.astype(np.int32), rec_t, rec_prim.astype(np.int32), rec_n


def _live_counters(world, uv, cutouts, table, rays, stats, marks, holed, hit, rec_t, rec_prim, rec_n, rows, arrays):
    """LIVE_COUNTERS of one finished walk (hole_then_medium_draw is counted leaf by leaf): what lay behind a hole, and what the kept hits on masked surfaces are"""
    from _nee_twin import PRIM_MOVING
    prims, quads, mats, tab, first_tri, on_of_quad = arrays
    n_prims = len(prims)

    def bump(key, which):
        stats[key] = stats.get(key, 0) + int(np.count_nonzero(which))
    sphere = hit & (rec_prim < n_prims)
    flat = hit & ~sphere
    qi = np.where(flat, rec_prim - n_prims, 0)
    mat = np.where(sphere, prims["mat"][np.where(sphere, rec_prim, 0)] & ~np.uint32(PRIM_MOVING), quads["mat"][qi]).astype(np.int64) if n_prims else quads["mat"][qi].astype(np.int64)
    moving = sphere & ((prims["mat"][np.where(sphere, rec_prim, 0)] & np.uint32(PRIM_MOVING)) != 0) if n_prims else sphere
    bump("hole_then_moving", holed & moving & (rays[:, 6] > F(0.25)))
    bump("hole_then_solid", holed & hit & np.asarray(marks["solid"], bool)[mat])
    masked = flat & on_of_quad[qi]
    image = masked & (mats["type"][mat] == XT.MAT_IMAGE)
    bump("kept_image_masked", image)
    bump("kept_mapped_masked", masked & np.asarray(marks["mapped"], bool)[mat])
    tri = masked & (rec_prim >= first_tri)
    smooth = np.asarray(marks["smooth"], bool)
    bump("kept_smooth_masked", tri & smooth[np.where(tri, rec_prim - first_tri, 0)] if len(smooth) else False)
    marks["masked_image"] = (None if rows is None else np.asarray(rows), image)
    c = np.nonzero(image)[0]
    if len(c):   # the rule's (u, v) of the kept hit, once more, beside the (u, v) the shade lookup reads (_tex_twin.hit_uv): the same bits
        under = (rec_prim[c] >= first_tri) & (tab is not None)
        rule_uv = np.zeros((len(c), 2), F)
        for sel, tuv in ((under, True), (~under, False)):
            if sel.any():
                k = c[sel]
                rule_uv[sel] = keeps(table, quads[qi[k]], tab[rec_prim[k] - first_tri] if tuv else None, rays[k, 0:3], rays[k, 3:6], rec_t[k], cutouts, quads["mat"][qi[k]])[1]
        shade_uv = XT.hit_uv(world, uv, rays[c], hit[c].astype(np.int32), rec_t[c], rec_prim[c].astype(np.int32), rec_n[c])
        bump("mask_uv_is_shade_uv", (rule_uv.view(np.uint32) == np.ascontiguousarray(shade_uv, F).view(np.uint32)).all(axis=1))


def walk_of(uv, cutouts, table, stats=None, eye=None, marks=None, wrong=None):
    """the walk under these tables as _path_twin.radiance takes one: (world, rays[, preset]) -> (hit, t, prim, normal)"""
    return lambda world, rays, preset=None, **draws: closest_intersection(world, uv, cutouts, table, rays, preset, stats, eye, marks=marks, wrong=wrong, **draws)
