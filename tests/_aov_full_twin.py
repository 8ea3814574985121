"""A numpy float32 twin of the feature sums of mode RT_AOV_FULL — test infrastructure only.

Per sample, in sample order, the feature trace is the colour path's first trace, so this twin is built from what restates that trace already and restates no
walk of its own:
  the ray and the tape: _path_twin.primary_rays with _path_twin.keys — the tape stands behind the camera's draws, where StreamParams::prim_rng stands;
  the walk: _tri_twin.closest_intersection, or _cutout_twin.walk_of(uv, cutouts, table) under a cutout table, handed the tape and the rows it serves
    (trace(world, rays, tape=, rows=)) — the one mechanism by which a medium draws inside a walk in _path_twin.radiance;
  the albedo: _aov_tex_twin.albedo_of_hits for every hit but the isotropic one, which adds the medium's own albedo (and the trace's normal, (1, 0, 0)).
tests/test_path_twin_oracle_cpu.py holds the walk-with-tape to the CPU oracle bit for bit, whole samples long; this twin uses the same rows of the same tape
for the first trace of every sample, so its first hits are the oracle's by that chain.

Counters (new_stats()): the cutout walk's own (_cutout_twin.COUNTERS: rejected, then_farther, then_miss, ...) and, from the medium's draws, fog_hits — first
hits inside the medium — and through_fog — rays that drew in the medium, were let through and hit something behind it.
"""
import numpy as np

import _aov_tex_twin as AT
import _cutout_twin as CT
import _path_twin as PT
import _smooth_twin as ST
import _tri_twin as TT
from _nee2_twin import world_arrays
from _nee_twin import F, _Tape

MAT_ISOTROPIC = PT.MAT_ISOTROPIC


def new_stats():
    return dict(CT.new_stats(), samples=0, fog_hits=0, through_fog=0, medium_draws=0, medium_hits=0)


def first_trace(world, cam, width, height, spp, seed, uv=None, cutouts=None, table=None, first_sample=0, stats=None, fresh_rng=False):
    """(rays (n, 7), hit, t, prim, normal) of the first trace of samples [first_sample, first_sample + spp) of every pixel, pixel-major.  fresh_rng: the walk draws
    from a fresh state of every sample's stream instead of the state the camera's draws left — the wrong place, for the test that shows it would be noticed."""
    gids, smp = PT.keys(width, height, spp, first_sample)
    tape, rays = PT.primary_rays(cam, width, height, seed, gids, smp, timed=True)
    if fresh_rng:
        tape = _Tape(seed, gids, smp)
    walk = TT.closest_intersection if cutouts is None else CT.walk_of(uv, np.asarray(cutouts), table, stats, tuple(cam.o))
    rows = np.arange(len(rays))
    cur0 = tape.cur.copy()
    hit, t, prim, normal = walk(world, rays, tape=tape, rows=rows, medium_info=stats)
    if stats is not None:
        prims, _, mats = world_arrays(world)
        drew, h = tape.cur > cur0, hit != 0
        in_fog = np.zeros(len(rays), bool)
        on_sphere = h & (prim < len(prims))
        in_fog[on_sphere] = mats["type"][prims["mat"][prim[on_sphere]] & ~np.uint32(AT.PRIM_MOVING)] == MAT_ISOTROPIC
        stats["samples"] += len(rays)
        stats["fog_hits"] += int(in_fog.sum())
        stats["through_fog"] += int((drew & h & ~in_fog).sum())
    return rays, hit, t, prim, normal


def sums(world, cam, width, height, spp, seed, uv=None, cutouts=None, table=None, image=None, noise=None, vn=None, first_sample=0, start=None, stats=None,
         fresh_rng=False, nmaps=None):
    """(H, W, 8) float32: (sum Nx, sum Ny, sum Nz, sum t, sum Ar, sum Ag, sum Ab, hits) of samples [first_sample, first_sample + spp), continued from `start` —
    _aov_tex_twin.sums' layout and order of additions.  nmaps (one record of capi.NORMAL_MAP_DT per material): the first-hit normal is the mapped normal —
    _nmap_twin.mapped_walk, the smooth rule and then the map, over the walk first_trace() ran with the tape and its rows (the cutout walk under a cutout table); the
    albedo's (u, v) on a sphere stays the one of the normal the walk found.  With every record off it is the smooth rule alone."""
    rays, hit, t, prim, normal = first_trace(world, cam, width, height, spp, seed, uv, cutouts, table, first_sample, stats, fresh_rng)
    prims, quads, mats = world_arrays(world)
    alb = AT.albedo_of_hits(world, rays, hit, t, prim, normal, True, uv, table, image, noise)
    h = hit != 0
    on_sphere = np.nonzero(h & (prim < len(prims)))[0]
    mat = (prims["mat"][prim[on_sphere]] & ~np.uint32(AT.PRIM_MOVING)).astype(np.int64)
    iso = mats["type"][mat] == MAT_ISOTROPIC
    alb[on_sphere[iso]] = mats["albedo"][mat[iso]]   # the isotropic hit: the medium's albedo
    if nmaps is not None:
        import _nmap_twin as NT
        traced = hit, t, prim, normal
        normal = NT.mapped_walk(world, vn, uv, nmaps, table, rays, base=lambda *a, **k: traced)[3]
    elif vn is not None:   # the smooth rule changes the normal sum only
        first_tri = len(prims) + int((quads["kind"] == 0).sum())
        rows = np.nonzero(h & (prim >= first_tri))[0]
        if len(rows):
            normal = normal.copy()
            normal[rows] = ST.shading_normal(quads[prim[rows] - len(prims)], ST.table(vn)[prim[rows] - first_tri], rays[rows, 0:3], rays[rows, 3:6], t[rows])[0]
    contrib = np.zeros((len(rays), 8), F)
    contrib[h, 0:3], contrib[h, 3], contrib[h, 7] = normal[h], t[h], F(1)
    contrib[:, 4:7] = alb
    contrib = contrib.reshape(width * height, spp, 8)
    acc = np.zeros((width * height, 8), F) if start is None else np.asarray(start, F).reshape(width * height, 8).copy()
    for s in range(spp):   # in sample order; a miss adds zeros to normal, depth and hits
        acc = (acc + contrib[:, s]).astype(F)
    return acc.reshape(height, width, 8)
