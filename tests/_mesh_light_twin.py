"""The numpy float32 twin of one whole sample for light sampling over quad, sphere AND triangle lights (mode 4) — test infrastructure only.

tests/_tri_twin.py restates §18 (worlds with triangles; modes 0, 1 and 2, whose tables leave triangles out).  This module owns mode 4 =
RT_LIGHT_SAMPLING_MESH: the table — mode 2's, then every triangle whose material is a diffuse light, in quad-index order, with area = 0.5f * sqrt(dot(n, n)),
n = cross(u, v) —, its counters, and the two rules mode 4 adds, functions of their own, so that a test can hold them to mathematics no kernel shares
(tests/test_mesh_lights_cpu.py: uniformity over the triangle, and the mean of 1 / pl against the solid angle):

    _tri_point(a, b, Q, u, v, hit_p)   the fold `if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }` — one fp32 add, a sum of exactly 1 is not folded — and
                                       d = ((Q + u * a) + v * b) - hit_p, not normalised
    _tri_pl(q, area, hp, dd, len2, ln) the library's quad test with the triangle kind on (hp, dd) over a fresh trace's interval; on a hit
                                       pl = ((t * t) * len2) / ((|dot(dd, n)| / ln) * area), on a miss 0

radiance() is the loop of tests/_path_twin.py over _tri_twin's walk under _light_tree_twin.TableRule, which calls the two.  tests/test_mesh_lights_cpu.py pins
it before anything is compared with it: in modes 0, 1 and 2 it equals _tri_twin on every world, and in mode 4 it equals _tri_twin's mode 2 on worlds without a
triangle light, bit for bit.

Scope: _tri_twin's.
"""
import numpy as np

import _nee2_twin as T2
import _nee_twin as T
import _path_twin as PT
import _tri_twin as TT
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays  # noqa: F401
from _nee_twin import F, MAX_LIGHTS, MISS, cross, dot
from _tri_twin import closest_intersection, first_hit_sums  # noqa: F401

TRIANGLE = 2            # RT_LIGHT_TRIANGLE
MAX_LIGHTS_MESH = 64    # RT_MAX_LIGHTS_MESH


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
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 / 4 as rt_renderer_light_sampling_enable takes it"""
    return T2.table_radiance(world, cam, width, height, max_depth, seed, gids, samples, mode, PT.counters(stats, new_stats()), closest_intersection, lights_of,
                             (0, 1, 2, 4), MAX_LIGHTS_MESH if mode == 4 else MAX_LIGHTS)


def frame_samples(world, cam, width, height, spp, max_depth, seed, mode=0, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, mode, stats), width, height, spp, first_sample)


luminance, in_order_sums, resolve = T.luminance, T.in_order_sums, T.resolve
