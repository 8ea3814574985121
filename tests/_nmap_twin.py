"""A numpy float32 twin of the normal-map rule — test infrastructure only.

tangents() and apply() restate normal_map_sphere_tangents / normal_map_tri_tangents / normal_map_apply of include/rt06.h (rt_scene_set_normal_map) in float32
numpy, every operation rounded on its own; case() is the two together over the texture table's twin (_tex_twin.lookup), as rt_normal_map_batch runs them.
apply64() is the rule in float64 for the mathematics no kernel shares.  The oracle does not know the rule: rt_normal_map_batch — the kernels' own function on
the host — is pinned to this twin bit for bit before anything is compared with either (tests/test_normal_maps_cpu.py).
"""
import numpy as np

import _env_tree_twin as VT
import _smooth_twin as ST
import _tex_twin as XT
import _tri_twin as TT
import _uv_twin as UT
from _nee2_twin import world_arrays
from _nee_twin import PRIM_MOVING, F, cross, dot

SPHERE, PLANAR, TRI_UV, GIVEN = 0, 1, 2, 3
REPLACED, FLAT, NO_TANGENT, NO_LENGTH, FACING, NO_FRAME = 1, 2, 3, 4, 5, 6
PATHS = {REPLACED: "replaced", FLAT: "flat", NO_TANGENT: "no_tangent", NO_LENGTH: "no_length", FACING: "facing", NO_FRAME: "no_frame"}
C0 = F(128.0) * XT.SCALE
K = F(255.0) / F(127.0)


def tangents(surface, a, b, tri_uv=None):
    """(dPdu (n, 3), dPdv (n, 3), frame (n,) bool) of n cases: a sphere's normal in a; a record's u and v in a, b; the same under the coordinates tri_uv (n, 6) =
    t0, t1, t2; or the two as given.  frame is False where a triangle's coordinates span no area."""
    surface = np.asarray(surface).reshape(-1)
    a, b = np.ascontiguousarray(a, F).reshape(-1, 3), np.ascontiguousarray(b, F).reshape(-1, 3)
    dpdu, dpdv, frame = a.copy(), b.copy(), np.ones(len(surface), bool)
    with np.errstate(all="ignore"):
        s = surface == SPHERE
        zero = np.zeros(int(s.sum()), F)
        dpdu[s] = np.stack([a[s, 2], zero, -a[s, 0]], axis=1)
        dpdv[s] = np.array([0, 1, 0], F)
        r = np.nonzero(surface == TRI_UV)[0]
        if len(r):
            t = np.ascontiguousarray(tri_uv, F).reshape(-1, 6)[r]
            du1, dv1 = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
            du2, dv2 = t[:, 4] - t[:, 0], t[:, 5] - t[:, 1]
            det = du1 * dv2 - du2 * dv1
            u, v = a[r], b[r]
            pu = u * dv2[:, None] - v * dv1[:, None]
            pv = v * du1[:, None] - u * du2[:, None]
            neg = (det < F(0))[:, None]
            dpdu[r], dpdv[r] = np.where(neg, -pu, pu), np.where(neg, -pv, pv)
            frame[r] = (det > F(0)) | (det < F(0))
    return dpdu.astype(F), dpdv.astype(F), frame


def apply(c, strength, dpdu, dpdv, ray_d, normal, detail=None):
    """the rule on decoded texels c (n, 3): (normal (n, 3) float32, path (n,) of REPLACED .. FACING).  detail (a dict): gets T, B and N of every case."""
    c, dpdu, dpdv, ray_d, N = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (c, dpdu, dpdv, ray_d, normal))
    strength = np.ascontiguousarray(strength, F).reshape(-1)
    with np.errstate(all="ignore"):
        m = ((c - C0) * K).astype(F)
        mx, my, mz = m[:, 0] * strength, m[:, 1] * strength, m[:, 2]
        flat = (mx == F(0)) & (my == F(0))
        T = dpdu - N * dot(N, dpdu)[:, None]
        tt = dot(T, T)
        no_t = ~(tt > F(0))
        T = T / np.sqrt(tt)[:, None]
        B = cross(N, T)
        B = np.where((dot(B, dpdv) < F(0))[:, None], -B, B)
        g = (T * mx[:, None] + B * my[:, None]) + N * mz[:, None]
        l2 = dot(g, g)
        no_l = ~(l2 > F(0))
        s = g / np.sqrt(l2)[:, None]
        ds, dn = dot(ray_d, s), dot(ray_d, N)
        same = ((ds > F(0)) & (dn > F(0))) | ((ds < F(0)) & (dn < F(0)))
    path = np.where(flat, FLAT, np.where(no_t, NO_TANGENT, np.where(no_l, NO_LENGTH, np.where(~same, FACING, REPLACED)))).astype(np.uint32)
    if detail is not None:
        detail.update(T=T, B=B, N=N)
    return np.where((path == REPLACED)[:, None], s, N).astype(F), path


def case(table, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength):
    """rt_normal_map_batch: table = [(image, wrap, filter), ...] as _tex_twin.lookup takes it"""
    dpdu, dpdv, frame = tangents(surface, a, b, tri_uv)
    c = XT.lookup(table, index, u, v)
    out, path = apply(c, strength, dpdu, dpdv, ray_d, normal)
    N = np.ascontiguousarray(normal, F).reshape(-1, 3)
    return np.where(frame[:, None], out, N).astype(F), np.where(frame, path, NO_FRAME).astype(np.uint32)


def counts(path):
    """{name: how many cases left the rule that way}"""
    return {name: int((np.asarray(path) == code).sum()) for code, name in PATHS.items()}


def encode(vectors):
    """unit vectors (..., 3) as the bytes of a normal map: 128 + round(127 n)"""
    return np.clip(128.0 + np.rint(127.0 * np.asarray(vectors, np.float64)), 0, 255).astype(np.uint8)


def apply64(m, dpdu, dpdv, normal):
    """the frame and the bent normal in float64, m = the tangent-space vector itself: (s, T, B)"""
    m, dpdu, dpdv, N = (np.asarray(x, np.float64).reshape(-1, 3) for x in (m, dpdu, dpdv, normal))
    T = dpdu - N * (N * dpdu).sum(axis=1, keepdims=True)
    T = T / np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(N, T)
    B = np.where(((B * dpdv).sum(axis=1) < 0)[:, None], -B, B)
    g = T * m[:, 0:1] + B * m[:, 1:2] + N * m[:, 2:3]
    return g / np.linalg.norm(g, axis=1, keepdims=True), T, B


# ---- whole samples: the walk every whole-sample twin calls, with the rule behind it --------------------------------------------------------------------------
def mapped_walk(world, vn, uv, nmaps, table, rays, preset=None, info=None, base=None, **draws):
    """_tri_twin.closest_intersection — behind _smooth_twin's rule when vn, a table of vertex normals, is given — then the normal-map rule on every hit whose
    material's record of nmaps (capi.NORMAL_MAP_DT, one per material) says on: (u, v) by _tex_twin.hit_uv from the normal the walk found, the tangents by the
    kind of surface (a triangle takes its coordinates' whenever the world has a table of them, as the kernels do), the entry of `table` = [(image, wrap,
    filter), ...].  info (a dict): its 'mapped' (hits on a mapped material) and one count per way out of the rule grow, and its 'uv' is what this call hands on
    to radiance(): (given (k,) bool, uv (k, 2), on a sphere (k,) bool) over the k rays — the (u, v) of every hit it mapped, taken from the normal BEFORE the map
    replaced it, which the image lookup and the roughness map of that hit share (_tex_twin.prefer_walk_uv) — or None when it mapped no hit.  base: the walk
    both rules post-process (default: _tri_twin's), as _smooth_twin.closest_intersection_smooth takes it."""
    if info is not None:
        info["uv"] = None
    if vn is not None and len(vn):
        hit, t, prim, normal = ST.closest_intersection_smooth(world, vn, rays, preset, base=base, **draws)   # draws: the tape and its rows, for a constant medium (_tri_twin)
    else:
        hit, t, prim, normal = (ST._flat_walk if base is None else base)(world, rays, preset, **draws)
    prims, quads, mats = world_arrays(world)
    first_tri = len(prims) + int((quads["kind"] == 0).sum())
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    mi = mat_of_prim[np.where(hit != 0, prim, 0)]
    rows = np.nonzero((hit != 0) & (nmaps["on"][mi] != 0))[0]
    if len(rows) == 0:
        return hit, t, prim, normal
    tuv = XT.hit_uv(world, uv, rays[rows], hit[rows], t[rows], prim[rows], normal[rows])
    k = len(rows)
    surface = np.full(k, PLANAR, np.uint32)
    a, b, tri = np.zeros((k, 3), F), np.zeros((k, 3), F), np.zeros((k, 6), F)
    sph = prim[rows] < len(prims)
    surface[sph] = SPHERE
    a[sph] = normal[rows][sph]
    q = quads[np.where(sph, 0, prim[rows] - len(prims))] if len(quads) else None
    if q is not None:
        a[~sph], b[~sph] = q["u"][~sph], q["v"][~sph]
        if uv is not None and len(uv):
            tr = ~sph & (prim[rows] >= first_tri)
            surface[tr] = TRI_UV
            tri[tr] = UT.table(uv)[prim[rows][tr] - first_tri].reshape(-1, 6)
    rec = nmaps[mi[rows]]
    out, path = case(table, surface, a, b, tri, normal[rows], rays[rows, 3:6], tuv[:, 0], tuv[:, 1], rec["image"], rec["strength"])
    normal = normal.copy()
    normal[rows] = out
    if info is not None:
        given, full, on_sphere = np.zeros(len(rays), bool), np.zeros((len(rays), 2), F), np.zeros(len(rays), bool)
        given[rows], full[rows], on_sphere[rows] = True, tuv, sph
        info["uv"] = (given, full, on_sphere)
        info["mapped"] = info.get("mapped", 0) + k
        for name, count in counts(path).items():
            info[name] = info.get(name, 0) + count
    return hit, t, prim, normal


def walk_of(vn, uv, nmaps, table, info=None, base=None):
    """(trace, walk) as _path_twin.radiance takes them, for a world with these tables: mapped_walk and the dict its (u, v) travel to radiance() in where there is a
    normal-map table (nmaps None = none), the smooth walk under a table of vertex normals, _tri_twin's flat walk otherwise; base: the walk they post-process
    in its place — _cutout_twin.walk_of(...), the rule in the leaf phase and then smooth normal and map at the hit the walk kept"""
    if nmaps is not None:
        info = {} if info is None else info
        return (lambda w, rays, preset=None, **draws: mapped_walk(w, vn, uv, nmaps, table, rays, preset, info, base, **draws)), info
    if vn is not None and len(vn):
        return ST.smooth_walk(vn, base=base), None
    return (TT.closest_intersection if base is None else base), None


def tex_of(uv, table):
    """tex as _path_twin.radiance takes it: (the table of texture coordinates or None, the texture table), or None without a texture table"""
    return (uv if uv is not None and len(uv) else None, table) if table is not None else None


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, vn, uv, nmaps, table, light=None, tree=None, first_sample=0, stats=None, info=None):
    """_env_tree_twin.frame_samples — plain (light None) or mode 48 — over the walk walk_of() chooses"""
    trace, walk = walk_of(vn, uv, nmaps, table, info)
    return VT.frame_samples(world, cam, width, height, spp, max_depth, seed, sky, light=light, tree=tree, tex=tex_of(uv, table), first_sample=first_sample,
                            stats=stats, walk=walk, trace=trace)
