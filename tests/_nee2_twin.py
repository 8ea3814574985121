"""Light sampling over quad AND sphere lights (mode 2) for the numpy float32 twin of one whole sample — test infrastructure only.

What this module owns: the sphere lights of a world and their areas, the light table of modes 1 and 2 (the quad lights as §16 lists them, then the static sphere
lights), §17's density of one sphere light (_sphere_pl) and the counters of the sphere rule.  radiance() runs the one loop of tests/_path_twin.py under
_light_tree_twin.TableRule over that table; every closest intersection comes from orc_trace_batch, which hits emitting spheres as it hits any other.
tests/test_light_sampling_spheres_cpu.py pins it — mode 0 to orc_radiance_batch, mode 1 to _nee_twin, bit for bit — before anything is compared with it.

Scope: _nee_twin's (pinhole cameras; spheres and quads with Lambertian, checker, metal and diffuse-light materials).
"""
import ctypes as C

import numpy as np

import _nee_twin as T
import _oracle as O
from _nee_twin import F, MAX_LIGHTS, PRIM_MOVING, dot, oracle_trace

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


def table_radiance(world, cam, width, height, max_depth, seed, gids, samples, mode, stats, trace, lights_of, modes, limit=MAX_LIGHTS):
    """the loop of _path_twin under the table of `mode` (0: the cosine lobe alone) as lights_of(prims, quads, mats, mode) lists it, of 1 to `limit` lights"""
    import _light_tree_twin as LT   # (the rule and the loop stand above this module)
    import _path_twin as PT
    assert mode in modes
    rule = None
    if mode:
        table = lights_of(*world_arrays(world), mode)
        assert 1 <= len(table[0]) <= limit
        rule = LT.TableRule(world, table)
    return PT.radiance(world, cam, width, height, max_depth, seed, gids, samples, trace, rule=rule, stats=stats)


def radiance(world, cam, width, height, max_depth, seed, gids, samples, mode=0, stats=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool); mode 0 / 1 / 2 as rt_renderer_light_sampling_enable takes it"""
    import _path_twin as PT
    return table_radiance(world, cam, width, height, max_depth, seed, gids, samples, mode, PT.counters(stats, new_stats()), oracle_trace, lights_of, (0, 1, 2))


def frame_samples(world, cam, width, height, spp, max_depth, seed, mode=0, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    import _path_twin as PT
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, mode, stats), width, height, spp, first_sample)


luminance, in_order_sums, resolve = T.luminance, T.in_order_sums, T.resolve
