"""The numpy float32 twin of one whole sample for light sampling through a light tree, with the light chosen by area (mode 16) — test
infrastructure only.

tests/_mesh_light_twin.py owns §19 (mode 4's table and the triangle rules).  This module owns mode 16 = RT_LIGHT_SAMPLING_TREE: mode 4's lights, permuted into
the leaf order of a median-split tree over their padded boxes.  What mode 16 adds are functions of their own, so that a test can hold each to something no
kernel shares (tests/test_light_tree_cpu.py):

    light_boxes(prims, quads, kind, index, M)   the padded box of every light: its vertices' box widened by PAD * M (a sphere: by that + (PAD_SPHERE * (M * M)) / r)
    build_tree(bmin, bmax)                      the builder: (order, lo, hi, skip, leaf) — preorder nodes, leaves in table order
    tree_of(world)                              the permuted table, the running sum of its areas and the nodes, as rt_world_light_table(.., 16) and
                                                rt_world_light_tree give them
    choose(cdf, x)                              the binary search: the smallest j with c_j > x, or n_l - 1
    tree_walk(tree, hp, dd, visit)              the stackless walk; visit(rows, leaves) is called with the leaves ENTERED, per ray in ascending table position
    leaf_term(tree, prims, quads, j, ...)       mode 4's pl_j without its division by area_j
    tree_density(...), linear_density(...)      the sum over the walk, and over every light of the same table: equal bit for bit when the walk misses nothing

It also owns TableRule, the light rule of every table mode (1, 2, 4 and 16) as tests/_path_twin.py takes it: which half a hit takes and the light half's
point — uniform or by-area choice, then the kind's draws — and the density of the chosen direction, the per-light sum or the tree walk.  radiance() is that
loop under it; tests/test_light_tree_cpu.py pins it before anything is compared with it: in modes 0, 1, 2 and 4 it equals _mesh_light_twin on every world,
bit for bit.

Scope: _tri_twin's.
"""
import numpy as np

import _mesh_light_twin as MT
import _nee2_twin as T2
import _nee_twin as T
import _path_twin as PT
from _mesh_light_twin import MAX_LIGHTS_MESH, TRIANGLE, _tri_hit, _tri_pl, _tri_point, lights_of, triangle_lights  # noqa: F401
from _nee2_twin import QUAD, SPHERE, world_arrays
from _nee_twin import F, MAX_LIGHTS, count, dot
from _tri_twin import closest_intersection, first_hit_sums  # noqa: F401

MAX_LIGHTS_TREE = 4096  # RT_MAX_LIGHTS_TREE
PAD = F(2.0 ** -10)           # RT_LIGHT_TREE_PAD
PAD_SPHERE = F(2.0 ** -18)    # RT_LIGHT_TREE_PAD_SPHERE
TREE_K = F(1.0 + 2.0 ** -16)  # RT_LIGHT_TREE_K
INNER = np.uint32(0xffffffff)
_quad_hit = T._quad_hit


def _gmin(x, y):
    """glm::min: (y < x) ? y : x — a NaN y is dropped, a NaN x is kept"""
    return np.where(y < x, y, x).astype(F)


def _gmax(x, y):
    """glm::max: (x < y) ? y : x"""
    return np.where(x < y, y, x).astype(F)


def light_boxes(prims, quads, kind, index, M):
    """(bmin, bmax) (n, 3) float32 of the lights (kind, index) in a world whose bounds' largest absolute coordinate is M"""
    n = len(kind)
    bmin, bmax = np.zeros((n, 3), F), np.zeros((n, 3), F)
    pad = PAD * F(M)
    for i in range(n):
        p = pad
        if kind[i] == SPHERE:
            pr = prims[index[i]]
            c, r = pr["c0"].astype(F), F(pr["radius"])
            lo, hi = c - r, c + r
            p = pad + (PAD_SPHERE * (F(M) * F(M))) / r
        else:
            q = quads[index[i]]
            Q, u, v = q["Q"].astype(F), q["u"].astype(F), q["v"].astype(F)
            qu, qv = Q + u, Q + v
            lo, hi = _gmin(_gmin(Q, qu), qv), _gmax(_gmax(Q, qu), qv)
            if kind[i] == QUAD:
                quv = qu + v
                lo, hi = _gmin(lo, quv), _gmax(hi, quv)
        bmin[i], bmax[i] = lo - p, hi + p
    return bmin, bmax


def build_tree(bmin, bmax):
    """§20's builder over padded boxes in mode 4's order: (order (n,), lo (2n-1, 3), hi (2n-1, 3), skip (2n-1,) uint32, leaf (2n-1,) uint32)"""
    n = len(bmin)
    cen = ((bmin + bmax) * F(0.5)).astype(F)
    order = np.arange(n)
    lo, hi = np.zeros((2 * n - 1, 3), F), np.zeros((2 * n - 1, 3), F)
    skip, leaf = np.zeros(2 * n - 1, np.uint32), np.full(2 * n - 1, INNER, np.uint32)
    count = [0]

    def build(a, b):
        at = count[0]
        count[0] += 1
        if b - a == 1:
            lo[at], hi[at], leaf[at] = bmin[order[a]], bmax[order[a]], a
        else:
            c = cen[order[a:b]]
            cmin, cmax = c[0], c[0]
            for row in c[1:]:
                cmin, cmax = _gmin(cmin, row), _gmax(cmax, row)
            ext = (cmax - cmin).astype(F)
            axis = 0
            if ext[1] > ext[axis]:
                axis = 1
            if ext[2] > ext[axis]:
                axis = 2
            order[a:b] = order[a:b][np.argsort(c[:, axis], kind="stable")]
            mid = a + (b - a) // 2
            left = build(a, mid)
            right = build(mid, b)
            lo[at], hi[at] = _gmin(lo[left], lo[right]), _gmax(hi[left], hi[right])
        skip[at] = count[0]
        return at

    build(0, n)
    assert count[0] == 2 * n - 1
    return order, lo, hi, skip, leaf


class Tree:
    """the permuted table (kind, index, area), cdf, A and the nodes of a world in mode 16; refused: the message of the refusal, or None"""


def tree_of(world):
    prims, quads, mats = world_arrays(world)
    kind, index, area = MT.lights_of(prims, quads, mats, 4)
    t = Tree()
    t.M = F(max(abs(float(v)) for v in list(world.bounds_min) + list(world.bounds_max)))
    bmin, bmax = light_boxes(prims, quads, kind, index, t.M)
    order, t.lo, t.hi, t.skip, t.leaf = build_tree(bmin, bmax)
    t.order, t.kind, t.index, t.area = order, kind[order], index[order], area[order].astype(F)
    t.cdf = np.zeros(len(order), F)
    c = F(0)
    t.refused = None
    for j in range(len(order)):
        c1 = F(c + t.area[j])
        if c1 == c and t.refused is None:
            t.refused = "lost in the fp32 running sum"
        t.cdf[j] = c = c1
    t.A = t.cdf[-1]
    t.n_l, t.n_nodes = len(order), 2 * len(order) - 1
    return t


def nodes_as_floats(t):
    """(n_nodes, 8) float32 as rt_world_light_tree writes them: min.xyz, skip (bits), max.xyz, leaf (bits)"""
    out = np.zeros((t.n_nodes, 8), F)
    out[:, 0:3], out[:, 4:7] = t.lo, t.hi
    out[:, 3], out[:, 7] = t.skip.view(F), t.leaf.view(F)
    return out


def choose(cdf, x):
    """§20's binary search, step for step: the smallest j with cdf[j] > x, or len(cdf) - 1; x (n,) float32"""
    x = np.asarray(x, F)
    lo, hi = np.zeros(len(x), np.int64), np.full(len(x), len(cdf) - 1, np.int64)
    while (lo < hi).any():
        go = lo < hi
        mid = (lo + hi) >> 1
        above = cdf[mid] > x
        hi = np.where(go & above, mid, hi)
        lo = np.where(go & ~above, mid + 1, lo)
    return lo


def tree_walk(t, hp, dd, visit):
    """§20's walk of rays (hp, dd), all at once: visit(rows, leaves) for the leaves entered in each round — per ray in ascending table position"""
    with np.errstate(all="ignore"):
        rd = (F(1) / dd).astype(F)
        at = np.zeros(len(hp), np.int64)
        rows = np.arange(len(hp))
        while len(rows):
            i = at[rows]
            ta, tb = (t.lo[i] - hp[rows]) * rd[rows], (t.hi[i] - hp[rows]) * rd[rows]
            mn, mx = _gmin(ta, tb), _gmax(ta, tb)
            tmin = _gmax(_gmax(mn[:, 0], mn[:, 1]), mn[:, 2])   # comp_max
            tmax = _gmin(_gmin(mx[:, 0], mx[:, 1]), mx[:, 2])   # comp_min
            entered = (tmin <= tmax * TREE_K) & (tmax > F(0))
            inner = t.leaf[i] == INNER
            at[rows] = np.where(entered & inner, i + 1, t.skip[i].astype(np.int64))
            got = entered & ~inner
            if got.any():
                visit(rows[got], t.leaf[i[got]].astype(np.int64))
            rows = rows[at[rows] < t.n_nodes]


def leaf_term(t, prims, quads, j, hp, dd, len2, ln):
    """mode 4's pl_j of table entry j without its division by area_j (the functions of modes 2 and 4 with an area of 1, which divides nothing):
    (term, met, disc > 0) — met: a hit of a quad or a triangle, a crossing in front for a sphere; the third is None but for a sphere"""
    if t.kind[j] == QUAD:
        q = quads[t.index[j]]
        qhit, qt = _quad_hit(q, hp, dd)
        nj = np.broadcast_to(q["normal"].astype(F), dd.shape)
        pl = ((qt * qt) * len2) / ((np.abs(dot(dd, nj)) / ln) * F(1))
        return np.where(qhit, pl, F(0)).astype(F), qhit, None
    if t.kind[j] == TRIANGLE:
        pl, thit = _tri_pl(quads[t.index[j]], F(1), hp, dd, len2, ln)
        return pl, thit, None
    pr = prims[t.index[j]]
    pl, pos, t1, t2 = T2._sphere_pl(pr["c0"].astype(F), F(pr["radius"]), F(1), hp, dd, len2, ln)
    return pl, pos & (t2 > F(0)), pos


def tree_density(t, prims, quads, hp, dd, len2, ln, on_leaf=None):
    """(sum of the terms in walk order (n,), credited (n, ) lists are on_leaf's business): on_leaf(rows, j, term, met, pos) sees every leaf visit"""
    total = np.zeros(len(hp), F)

    def visit(rows, leaves):
        for j in np.unique(leaves):
            r = rows[leaves == j]
            term, met, pos = leaf_term(t, prims, quads, j, hp[r], dd[r], len2[r], ln[r])
            total[r] = total[r] + term
            if on_leaf is not None:
                on_leaf(r, j, term, met, pos)

    tree_walk(t, hp, dd, visit)
    return total


def linear_density(t, prims, quads, hp, dd, len2, ln):
    """the same sum over EVERY light of the permuted table, in table order: what the walk must equal bit for bit; and how many terms were > 0"""
    total, positive = np.zeros(len(hp), F), np.zeros(len(hp), np.int64)
    for j in range(t.n_l):
        term, _, _ = leaf_term(t, prims, quads, j, hp, dd, len2, ln)
        total = total + term
        positive += term > F(0)
    return total, positive


def new_stats(n=MAX_LIGHTS_MESH):
    """(§20: light_samples over a table of n; tree_leaves: leaf visits of the walks; tree_sphere_uncredited: drawn spheres the walk did not credit)
    _nee2_twin's counters with light_samples[i] over a table of 64, and for triangle lights: tri_light_half: light-half draws sent to a triangle light;
    tri_folded: of those, the draws with a + b > 1; tri_own_missed: light-half draws whose own triangle's test rejects the direction (a point that rounding put
    just outside: pl_j = 0, the direction is still taken); two_tri_crossings: directions that meet two or more triangle lights (both crossings of a closed
    mesh); tri_and_other: directions that meet a triangle light and a light of another kind"""
    st = T2.new_stats()
    st["light_samples"] = np.zeros(n, np.int64)
    st.update({"tree_leaves": 0, "tree_sphere_uncredited": 0})   # §20
    st.update({"tri_light_half": 0, "tri_folded": 0, "tri_own_missed": 0, "two_tri_crossings": 0, "tri_and_other": 0})
    return st


class TableRule:
    """The light rule of the table modes for _path_twin.radiance: table = (kind, index, area) as a lights_of() lists it (modes 1, 2, 4), or, tree = tree_of(world),
    the permuted table with the light chosen by area and the density by the walk (mode 16).  A Lambertian or checker hit is sampled."""
    images = False

    def __init__(self, world, table, tree=None):
        self.prims, self.quads, _ = world_arrays(world)
        self.kind, self.index, self.area = (tree.kind, tree.index, tree.area) if tree is not None else table
        self.tree, self.n_l = tree, len(self.kind)

    def pick(self, tape, r, sampled, mt, hit_p, new_d, stats):
        """The draws, in order: c (below 0.5: the light half); the light — none for one light, next * n_l clamped or, by area, the smallest j with
        c_j > next * A —; the point: a triangle's two draws folded, a parallelogram's two draws, a sphere's on-unit vector, rejection loop and all."""
        prims, quads, l_kind, l_index, n_l = self.prims, self.quads, self.kind, self.index, self.n_l
        to_light = np.zeros(len(r), bool)
        drawn = np.full(len(r), -1, np.int64)   # the light a light-half draw went to
        if sampled.any():
            c = tape.next(r[sampled])
            to_light[np.nonzero(sampled)[0]] = c < F(0.5)
        if to_light.any():
            s = np.nonzero(to_light)[0]
            li = np.zeros(len(s), np.int64)
            if n_l > 1 and self.tree is not None:
                xs = tape.next(r[s]) * self.tree.A
                li = choose(self.tree.cdf, xs)
                clamped = ~(self.tree.A > xs)
            elif n_l > 1:
                scaled = (tape.next(r[s]) * F(n_l)).astype(np.uint32)
                li = np.minimum(scaled, np.uint32(n_l - 1)).astype(np.int64)
                clamped = scaled >= n_l
            drawn[s] = li
            if stats is not None:
                stats["index_clamped"] += int(clamped.sum()) if n_l > 1 else 0
                stats["light_samples"] += np.bincount(li, minlength=len(stats["light_samples"]))
                stats["checker_light_half"] += int((mt[s] == 3).sum())
                count(stats, "sphere_light_half", int((l_kind[li] == SPHERE).sum()))
            sq_, ss_, st_ = s[l_kind[li] == QUAD], s[l_kind[li] == SPHERE], s[l_kind[li] == TRIANGLE]
            if len(st_):   # §19: a, b folded into the triangle: a point uniform over its area; no on-unit draw
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
        return to_light, np.zeros(len(r), bool), (to_light, drawn)

    def density(self, picked, s, hp, dd, len2, ln, pdf_cos, stats):
        """(pl of the directions dd from hp, own_lost: light-half draws whose own sphere gives !(disc > 0) — a failed scatter): the sum of the lights' pl_j
        over n_l or, with the tree, the walk's sum of the terms without their areas over A"""
        prims, quads, l_kind, l_index, l_area, tree = self.prims, self.quads, self.kind, self.index, self.area, self.tree
        to_light, drawn = picked[0][s], picked[1][s]
        pdf_light = np.zeros(len(s), F)
        met = np.zeros(len(s), np.int64)          # lights the direction meets (stats only)
        met_sphere = np.zeros(len(s), np.int64)
        met_tri = np.zeros(len(s), np.int64)
        own_lost = np.zeros(len(s), bool)
        if tree is not None:   # §20
            credited = np.zeros(len(s), bool)   # drawn spheres whose leaf the walk reached with disc > 0

            def on_leaf(rr, j, term, hit, pos):
                met[rr] += hit
                if l_kind[j] == TRIANGLE:
                    met_tri[rr] += hit
                if l_kind[j] == SPHERE:
                    met_sphere[rr] += hit
                    credited[rr] |= to_light[rr] & (drawn[rr] == j) & pos
                if stats is not None:
                    stats["tree_leaves"] += len(rr)

            pdf_light = tree_density(tree, prims, quads, hp, dd, len2, ln, on_leaf)
            own_lost = to_light & (drawn >= 0) & (l_kind[np.maximum(drawn, 0)] == SPHERE) & ~credited
            if stats is not None:
                stats["tree_sphere_uncredited"] += int(own_lost.sum())
        for j in range(self.n_l if tree is None else 0):
            if l_kind[j] == QUAD:
                q = quads[l_index[j]]
                qhit, qt = _quad_hit(q, hp, dd)
                nj = np.broadcast_to(q["normal"].astype(F), dd.shape)
                pl = ((qt * qt) * len2) / ((np.abs(dot(dd, nj)) / ln) * l_area[j])
                pdf_light = pdf_light + np.where(qhit, pl, F(0)).astype(F)
                met += qhit
            elif l_kind[j] == TRIANGLE:   # §19
                pl, thit = _tri_pl(quads[l_index[j]], l_area[j], hp, dd, len2, ln)
                pdf_light = pdf_light + pl
                met += thit
                met_tri += thit
                if stats is not None:
                    stats["tri_own_missed"] += int((to_light & (drawn == j) & ~thit).sum())
            else:   # §17
                pr = prims[l_index[j]]
                pl, pos, t1, t2 = T2._sphere_pl(pr["c0"].astype(F), F(pr["radius"]), l_area[j], hp, dd, len2, ln)
                pdf_light = pdf_light + pl
                front1, front2 = pos & (t1 > F(0)), pos & (t2 > F(0))
                own_lost |= to_light & (drawn == j) & ~pos
                met += front2
                met_sphere += front2
                if stats is not None:
                    mine = to_light & (drawn == j)
                    stats["both_roots"] += int((front1 & front2).sum())
                    stats["one_root"] += int((~front1 & front2).sum())
                    stats["no_root"] += int((pos & ~front2).sum())
                    ocj = pr["c0"].astype(F)[None, :] - hp
                    ccj = dot(ocj, ocj) - F(pr["radius"]) * F(pr["radius"])
                    stats["near_surface"] += int(((ccj >= F(0)) & (ccj < F(0.21) * (F(pr["radius"]) * F(pr["radius"])))).sum())
                    stats["disc_nonpos_light_half"] += int((mine & ~pos).sum())
                    stats["far_side_sample"] += int((mine & front1 & front2 & (np.abs(t2 - F(1)) < np.abs(t1 - F(1)))).sum())
        if stats is not None:
            stats["below_surface"] += int((to_light & (pdf_cos == F(0))).sum())
            stats["light_half_unmet"] += int((to_light & (met == 0)).sum())
            stats["cos_one_light"] += int((~to_light & (met == 1)).sum())
            stats["cos_many_lights"] += int((~to_light & (met >= 2)).sum())
            count(stats, "sphere_and_other", int(((met_sphere >= 1) & (met >= 2)).sum()))
            count(stats, "two_tri_crossings", int((met_tri >= 2).sum()))
            count(stats, "tri_and_other", int(((met_tri >= 1) & (met > met_tri)).sum()))
        return pdf_light / (tree.A if tree is not None else F(self.n_l)), own_lost


def radiance(world, cam, width, height, max_depth, seed, gids, samples, mode=0, stats=None, trace=closest_intersection):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 / 4 / 16 as rt_renderer_light_sampling_enable takes
    it: mode 16 over tree_of(world), the others as _mesh_light_twin lists their tables; trace: the walk"""
    if mode != 16:
        return T2.table_radiance(world, cam, width, height, max_depth, seed, gids, samples, mode, PT.counters(stats, new_stats()), trace, lights_of, (0, 1, 2, 4),
                                 MAX_LIGHTS_MESH if mode == 4 else MAX_LIGHTS)
    tree = tree_of(world)
    assert 1 <= tree.n_l <= MAX_LIGHTS_TREE and tree.refused is None
    return PT.radiance(world, cam, width, height, max_depth, seed, gids, samples, trace, rule=TableRule(world, None, tree),
                       stats=PT.counters(stats, new_stats(max(tree.n_l, MAX_LIGHTS_MESH))))


def frame_samples(world, cam, width, height, spp, max_depth, seed, mode=0, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, mode, stats), width, height, spp, first_sample)


luminance, in_order_sums, resolve = T.luminance, T.in_order_sums, T.resolve
