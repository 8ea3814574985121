"""Pins against the REFERENCE itself.

tests/golden/glm_*   : the reference's vendored GLM 0.9.9.7 + utilities/glm_utils.h   (oracle/ref_glm_probe.cpp)
tests/golden/ref_*   : the reference's own rt_engine headers — ray_data.cuh, geometry/aabb.cuh, HittableList.cuh,
                       bvh_node.cuh, BVH.cuh (layout), shaders/cu_Textures.cuh — compiled by plain g++ against NVIDIA's
                       real <cuda_runtime.h> from the image's triton wheel      (oracle/ref_path_probe.cpp)
tests/golden/ref_core_*: the reference's SphereHittable.cuh/.cu, BVH.cuh/.cu (traversal + BVH_Handle::Factory), cu_materials.cuh,
                       cu_Cameras.cuh, cuRandom.cuh + glm_utils.h's cuRandomInUnit/OnUnit, with three stand-ins that do no
                       pinned arithmetic (oracle/ref_shim/: curand_uniform served from a tape of k, u = k * 2^-24; a prelude for
                       cuError.h / cuda_utils.cuh; host cudaMalloc/cudaMemcpy/cudaFree)    (oracle/ref_core_probe.cpp)
All sets are produced by `python oracle/gen_golden.py` in the dev container and committed as data.

CPU tests (`not gpu`): the oracle (and the product's host-side aabb helpers) reproduce the reference's outputs bit for bit.
GPU tests: the HIP device functions reproduce the same outputs bit for bit, called through the C ABI probes — the direct
reference -> HIP check; the tape probes (rt_probe_scatter_tape / rt_probe_camera_tape) reach the edges of measure zero under the
product's 2^-24 stream (a zero or unit-length draw vector, u == reflect_prob, u = 1).  What stays unpinned: sample_world and
render_kernel (Renderer.cu launches kernels in its own text), and the shade-phase copies inlined in rt_stream_kernel.hpp /
rt_xchg_kernel.hpp at tape-only edges (they are reached only through the oracle-vs-framebuffer chain, on natural streams).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _oracle as O
from _common import bits_equal, mismatch_report, pkg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISS = np.float32(3.402823466e+38)


def gold(name, cols, dtype="<f4"):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype).reshape(-1, cols)


def olib():
    L = O.lib()
    L.orc_aabb_misc_batch.argtypes = [C.c_size_t, O.f32p, O.f32p]
    L.orc_checker_batch.argtypes = [C.c_size_t, O.f32p, O.f32p]
    L.orc_ray_batch.argtypes = [C.c_size_t, O.f32p, O.f32p]
    L.orc_trace_counts.argtypes = [C.POINTER(O.World), C.c_size_t, O.f32p, O.u32p, O.u32p]
    L.orc_trace_order.argtypes = [C.POINTER(O.World), C.c_size_t, O.f32p, C.c_uint32, O.i32p]
    return L


# ---------------------------------------------------------------------------------------------------------------------
# the aggregate fixtures as flat worlds (64 scenarios x 8 spheres x 64 rays)
# ---------------------------------------------------------------------------------------------------------------------
class AggScenario:
    """One scenario of tests/golden/ref_agg_*: arrays kept alive + a world struct of the requested binding class."""

    def __init__(self, s, kind, world_cls, node_dt, prim_dt, mat_dt):
        spheres = gold("ref_agg_spheres.f32", 4).reshape(64, 8, 4)[s]
        self.prims = np.zeros(8, dtype=prim_dt)
        self.prims["c0"], self.prims["radius"], self.prims["c1"], self.prims["mat"] = spheres[:, :3], spheres[:, 3], spheres[:, :3], 0
        self.mats = np.zeros(1, dtype=mat_dt)
        self.mats["albedo"] = 0.5
        boxes = gold("ref_agg_nodeboxes.f32", 6).reshape(64, 7, 6)[s]
        refs = gold("ref_agg_refs.i32", 15, "<i4")[s]
        self.nodes = np.zeros(7, dtype=node_dt)
        self.nodes["min"], self.nodes["max"] = boxes[:, :3], boxes[:, 3:]
        self.nodes["left"], self.nodes["right"] = refs[0:14:2], refs[1:14:2]
        lb = gold("ref_agg_listbounds.f32", 6)[s]
        w = world_cls()
        w.kind = 1 if kind == "list" else 2   # RT_WORLD_LIST / RT_WORLD_NODE_TREE
        w.root = int(refs[14]) if kind == "tree" else 0
        w.n_nodes = 7 if kind == "tree" else 0
        w.n_prims, w.n_materials, w.max_stack = 8, 1, 8
        # a HittableList carries its own bounds (HittableList.cuh:19); a bvh_node tree's root box is node data
        for k in range(3):
            w.bounds_min[k], w.bounds_max[k] = (float(lb[k]), float(lb[3 + k])) if kind == "list" else (float(boxes[int(refs[14])][k]), float(boxes[int(refs[14])][3 + k]))
        w.nodes = self.nodes.ctypes.data if kind == "tree" else None
        w.prims, w.materials = self.prims.ctypes.data, self.mats.ctypes.data
        self.world = w
        self.rays = np.ascontiguousarray(gold("ref_agg_rays.f32", 7).reshape(64, 64, 7)[s])
        self.expect = gold(f"ref_agg_{kind}_out.f32", 12).reshape(64, 64, 12)[s]   # hit, t, prim, n_visits, order[8]


def check_agg(kind, trace_fn, world_cls, node_dt, prim_dt, mat_dt, counts_fn=None, order_fn=None):
    n_hits = 0
    for s in range(64):
        sc = AggScenario(s, kind, world_cls, node_dt, prim_dt, mat_dt)
        hit, t, prim = trace_fn(sc.world, sc.rays)
        e = sc.expect
        assert np.array_equal(hit, e[:, 0].astype(np.int32)), f"{kind} scenario {s}: hit flags differ at rays {np.nonzero(hit != e[:, 0])[0][:5]}"
        assert bits_equal(t, e[:, 1]), f"{kind} scenario {s}: " + mismatch_report(t, e[:, 1])
        assert np.array_equal(prim, e[:, 2].astype(np.int32)), f"{kind} scenario {s}: closest primitive differs (visiting order / tie rule)"
        if counts_fn is not None:
            leaf = counts_fn(sc.world, sc.rays)
            assert np.array_equal(leaf, e[:, 3].astype(np.uint32)), f"{kind} scenario {s}: number of leaves reached differs"
        if order_fn is not None:
            order = order_fn(sc.world, sc.rays)
            assert np.array_equal(order, e[:, 4:12].astype(np.int32)), f"{kind} scenario {s}: leaf visiting order differs"
        n_hits += int(hit.sum())
    assert n_hits > 1000


# ---------------------------------------------------------------------------------------------------------------------
# CPU: oracle (and the product's host helpers) against the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_record_layouts():
    """sizeof / offsetof of the reference's PODs, as compiled from its headers, against the flat records of include/rt06.h."""
    lay = json.load(open(os.path.join(GOLD, "ref_layout.json")))
    assert lay["sizeof_Ray"] == 28 and lay["offsetof_Ray_d"] == 12 and lay["offsetof_Ray_time"] == 24
    assert lay["sizeof_RayPayload"] == 40 and lay["sizeof_aabb"] == 24
    p = pkg()
    assert lay["sizeof_BVH_Node"] == p.capi.NODE_DT.itemsize == O.NODE_DT.itemsize == 32
    assert lay["offsetof_BVH_Node_left_child_idx"] == p.capi.NODE_DT.fields["left"][1] == 24
    assert lay["offsetof_BVH_Node_right_child_hittable_idx"] == p.capi.NODE_DT.fields["right"][1] == 28
    assert lay["IS_LEAF_CODE"] == -1
    assert np.array([lay["MISS_DIST_bits"]], np.uint32).view(np.float32)[0] == MISS


def test_oracle_aabb_intersects_matches_reference():
    """G1: aabb::intersects (aabb.cuh:30-44) incl. 0 / +-inf / NaN / origin-inside / inverted / empty boxes."""
    i, e = gold("ref_aabb_in.f32", 13), gold("ref_aabb_out.f32", 2)
    n = len(i)
    hit, dist = np.zeros(n, np.int32), np.zeros(n, np.float32)
    O.lib().orc_aabb_batch(n, np.ascontiguousarray(i[:, 0:6]), np.ascontiguousarray(i[:, 6:12]), np.ascontiguousarray(i[:, 12]), hit, dist)
    assert np.array_equal(hit, e[:, 0].astype(np.int32)), f"{(hit != e[:, 0]).sum()} hit flags differ"
    assert bits_equal(dist, e[:, 1]), mismatch_report(dist, e[:, 1])
    assert 0.2 < e[:, 0].mean() < 0.7


def test_oracle_aabb_helpers_match_reference():
    i, e = gold("ref_aabbmisc_in.f32", 12), gold("ref_aabbmisc_out.f32", 20)
    out = np.zeros_like(e)
    olib().orc_aabb_misc_batch(len(i), i, out)
    assert bits_equal(out, e), mismatch_report(out, e)


def test_product_host_aabb_helpers_match_reference():
    """the builders' helpers inside librt06.so (csrc/rt_host.cpp), through the C ABI — runs without a GPU"""
    i, e = gold("ref_aabbmisc_in.f32", 12), gold("ref_aabbmisc_out.f32", 20)
    out = pkg().api.probe_aabb_misc(i)
    assert bits_equal(out, e), mismatch_report(out, e)


def test_oracle_checker_texture_matches_reference():
    """checker_texture::value (cu_Textures.cuh:31-39): truncation toward zero, negative coordinates, cell boundaries"""
    i, e = gold("ref_checker_in.f32", 10), gold("ref_checker_out.f32", 3)
    out = np.zeros_like(e)
    olib().orc_checker_batch(len(i), i, out)
    assert bits_equal(out, e), mismatch_report(out, e)
    assert 0.3 < np.all(e == i[:, 0:3], axis=1).mean() < 0.7   # both colours occur


def test_oracle_ray_at_and_backfacing_match_reference():
    i, e = gold("ref_ray_in.f32", 10), gold("ref_ray_out.f32", 4)
    out = np.zeros_like(e)
    olib().orc_ray_batch(len(i), i, out)
    assert bits_equal(out, e), mismatch_report(out, e)


def _oracle_trace(world, rays):
    n = len(rays)
    hit, t, prim, nrm = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
    assert O.lib().orc_trace_batch(C.byref(world), n, rays, hit, t, prim, nrm) == 0
    return hit, t, prim


def _oracle_order(world, rays):
    order = np.zeros((len(rays), 8), np.int32)
    assert olib().orc_trace_order(C.byref(world), len(rays), rays, 8, order) == 0
    return order


def _oracle_counts(world, rays):
    leaf, box = np.zeros(len(rays), np.uint32), np.zeros(len(rays), np.uint32)
    assert olib().orc_trace_counts(C.byref(world), len(rays), rays, leaf, box) == 0
    return leaf


@pytest.mark.parametrize("kind", ["list", "tree"])
def test_oracle_aggregates_match_reference(kind):
    """HittableList::ClosestIntersection (HittableList.cuh:21-34) / bvh_node::ClosestIntersection (bvh_node.cuh:19-24):
    closest hit, its primitive (identical spheres expose the visiting order) and the number of leaves reached."""
    check_agg(kind, _oracle_trace, O.World, O.NODE_DT, O.PRIM_DT, O.MAT_DT, _oracle_counts, _oracle_order)


def test_reference_fixture_visit_orders_are_consistent():
    """the recorded leaf order of the list is 0..7 whenever the bounds pre-test passes; of the tree, a pre-order walk"""
    e = gold("ref_agg_list_out.f32", 12)
    visited = e[:, 3] > 0
    assert np.all(e[visited, 3] == 8) and np.all(e[visited, 4:12] == np.arange(8, dtype=np.float32))
    assert 0.05 < (~visited).mean() < 0.6


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the HIP device functions against the reference
# ---------------------------------------------------------------------------------------------------------------------
GLM_SHAPES = {"dot": (6, 1), "cross": (6, 3), "normalize": (3, 3), "reflect": (6, 3), "refract": (7, 3), "mix3": (7, 3), "mix1": (3, 1),
              "min3": (6, 3), "max3": (6, 3), "compmax": (3, 1), "compmin": (3, 1), "clamp01_sqrt": (3, 3), "near_zero": (3, 1),
              "length2": (3, 1), "lerp": (7, 3), "radians": (1, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GLM_SHAPES))
def test_device_math_matches_reference_glm(name):
    """csrc/rt_math.hpp on gfx950 == the reference's GLM / glm_utils.h on the committed vectors (NaN / inf / denormals included)"""
    nin, nout = GLM_SHAPES[name]
    i, e = gold(f"glm_{name}_in.f32", nin), gold(f"glm_{name}_out.f32", nout)
    assert len(i) == len(e) == 1024
    out = pkg().api.probe_glm(name, i)
    assert bits_equal(out, e), f"{name}: " + mismatch_report(out, e)


@pytest.mark.gpu
def test_device_ray_at_and_backfacing_match_reference():
    i, e = gold("ref_ray_in.f32", 10), gold("ref_ray_out.f32", 4)
    out = pkg().api.probe_glm("ray", i)
    assert bits_equal(out, e), mismatch_report(out, e)


@pytest.mark.gpu
def test_device_aabb_intersects_matches_reference():
    i, e = gold("ref_aabb_in.f32", 13), gold("ref_aabb_out.f32", 2)
    hit, dist = pkg().api.probe_aabb(i[:, 0:6], i[:, 6:12], i[:, 12])
    assert np.array_equal(hit, e[:, 0].astype(np.int32)), f"{(hit != e[:, 0]).sum()} hit flags differ"
    assert bits_equal(dist, e[:, 1]), mismatch_report(dist, e[:, 1])


@pytest.mark.gpu
def test_device_checker_texture_matches_reference():
    """LambertianTexture's attenuation = checker_texture::value at the hit point (cu_materials.cuh:27-40): the scatter probe with
    the hit point placed at `pos` (origin = pos, distance 0)"""
    p = pkg()
    i, e = gold("ref_checker_in.f32", 10), gold("ref_checker_out.f32", 3)
    n = len(i)
    mats = np.zeros(n, dtype=p.capi.MAT_DT)
    mats["albedo"], mats["albedo2"], mats["type"] = i[:, 0:3], i[:, 3:6], p.capi.MAT_LAMBERTIAN_CHECKER
    mats["param"] = np.float32(1.0) / i[:, 6]                # inv_scale(1.0f / scale), cu_Textures.cuh:27
    rays = np.zeros((n, 7), np.float32)
    rays[:, 0:3], rays[:, 3:6] = i[:, 7:10], (0.0, -1.0, 0.0)
    normals = np.tile(np.float32([0, 1, 0]), (n, 1))
    keys = np.stack([np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)], axis=1)
    sc, _, att, _ = p.api.probe_scatter(7, mats, rays, np.zeros(n, np.float32), normals, keys)
    ok = sc == 1                                           # a degenerate direction absorbs (cu_materials.cuh:34): no colour then
    assert ok.mean() > 0.99
    assert bits_equal(att[ok], e[ok]), mismatch_report(att[ok], e[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["list", "tree"])
def test_device_aggregates_match_reference(kind):
    p = pkg()

    def trace(world, rays):
        hit, t, prim, _ = p.api.probe_trace(world, rays)
        return hit, t, prim
    check_agg(kind, trace, p.capi.WorldFlat, p.capi.NODE_DT, p.capi.PRIM_DT, p.capi.MAT_DT)


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/ref_core_*: spheres, the flat BVH and its builders, Scatter, the cameras — from the reference's own code
# (oracle/ref_core_probe.cpp).  Uniforms come from tapes of k, u = k * 2^-24: natural cases take the product's own stream for
# (seed 1984, pixel, sample) and are replayed by the key-driven probes; adversarial prefixes reach edges of measure zero under that
# stream and are replayed by the tape probes.  `draws` = uniforms consumed.
# ---------------------------------------------------------------------------------------------------------------------
SEED = 1984


def core(name, cols, dtype="<f4"):
    return gold(f"ref_core_{name}", cols, dtype)


def olib_core():
    L = olib()
    L.orc_scatter_tape.argtypes = [C.c_size_t, C.c_void_p, O.f32p, O.f32p, O.f32p, O.u32p, O.u32p, O.i32p, O.f32p, O.f32p, O.u32p]
    L.orc_camera_tape.argtypes = [C.POINTER(O.Camera), C.c_size_t, O.f32p, O.u32p, O.u32p, O.f32p, O.u32p]
    L.orc_sphere_hit_batch.argtypes = [C.c_size_t, C.c_void_p, O.f32p, O.f32p, O.i32p, O.f32p, O.f32p]
    return L


class Tapes:
    """ref_core_<kind>_idx.u32 rows [offset, length, pixel, sample, natural] + ref_core_<kind>_tape.u32"""

    def __init__(self, kind):
        self.idx = core(f"{kind}_idx.u32", 5, "<u4")
        self.tape = np.fromfile(os.path.join(GOLD, f"ref_core_{kind}_tape.u32"), dtype="<u4")
        self.offsets = np.ascontiguousarray(self.idx[:, 0:2])
        self.keys = np.ascontiguousarray(self.idx[:, 2:4])
        self.natural = self.idx[:, 4] == 1
        self.draws = self.idx[:, 1]


def _prims(rows, mat=0):
    """[c0 3, c1 3, radius, moving] -> PRIM_DT records (RT_PRIM_MOVING = bit 31 of mat)"""
    p = np.zeros(len(rows), dtype=O.PRIM_DT)
    p["c0"], p["c1"], p["radius"] = rows[:, 0:3], rows[:, 3:6], rows[:, 6]
    p["mat"] = np.where(rows[:, 7] > 0, np.uint32(0x80000000) | np.uint32(mat), np.uint32(mat))
    return p


def _scatter_inputs(i, dt):
    """ref_core_scatter_in rows -> (materials, rays)"""
    mats = np.zeros(len(i), dtype=dt)
    mats["type"], mats["albedo"], mats["param"], mats["albedo2"] = i[:, 8].astype(np.uint32), i[:, 9:12], i[:, 12], i[:, 13:16]
    return mats, np.ascontiguousarray(i[:, 16:23])


def _check_scatter(name, sc, rays, att, draws, e, expect_draws, rows=slice(None)):
    e = e[rows]
    assert np.array_equal(draws, expect_draws), f"{name}: draws differ at cases {np.nonzero(draws != expect_draws)[0][:5]}"
    assert np.array_equal(sc, e[:, 4].astype(np.int32)), f"{name}: scatter flags differ at cases {np.nonzero(sc != e[:, 4])[0][:5]}"
    assert bits_equal(rays, e[:, 5:12]), f"{name}: out rays: " + mismatch_report(rays, e[:, 5:12])
    assert bits_equal(att, e[:, 12:15]), f"{name}: attenuation: " + mismatch_report(att, e[:, 12:15])


def make_cameras(ctors):
    """ref_core_camera_cams rows -> cameras built by (pinhole, defocus, motion) constructors"""
    cams = []
    for row in core("camera_cams.f32", 16):
        f, at, up, vfov, aspect = [float(x) for x in row[1:4]], [float(x) for x in row[4:7]], [float(x) for x in row[7:10]], float(row[10]), float(row[11])
        t = int(row[0])
        cams.append(ctors[0](f, at, up, vfov, aspect) if t == 0 else ctors[1](f, at, up, vfov, aspect, float(row[12]), float(row[13]))
                    if t == 1 else ctors[2](f, at, up, vfov, aspect, float(row[14]), float(row[15])))
    return cams


def _cam_state(c):
    return np.array(list(c.o) + list(c.u) + list(c.v) + list(c.w) + [c.viewport_width, c.viewport_height, c.lens_radius, c.focus_dist, c.t0, c.t1], np.float32)


# which of the 18 state columns each reference class has (cu_Cameras.cuh: Pinhole o,u,v,w; DefocusBlur + viewport, lens, focus; MotionBlur + t0, t1)
CAM_STATE_COLS = {0: list(range(12)), 1: list(range(16)), 2: list(range(12)) + [16, 17]}


def check_camera_ctors(cams):
    state, types = core("camera_state.f32", 18), core("camera_cams.f32", 16)[:, 0].astype(int)
    for i, c in enumerate(cams):
        cols = CAM_STATE_COLS[types[i]]
        got = _cam_state(c)[cols]
        assert int(c.type) == types[i]
        assert bits_equal(got, state[i, cols]), f"camera {i}: " + mismatch_report(got, state[i, cols])


def run_cameras(cams, keyed, taped):
    """keyed(cam, st, keys) / taped(cam, st, tape, offsets) -> (rays, draws); checks both against ref_core_camera_out"""
    i, e, T = core("camera_in.f32", 3), core("camera_out.f32", 8), Tapes("camera")
    ci = i[:, 0].astype(int)
    n_checked = 0
    for c in range(len(cams)):
        rows = ci == c
        st = np.ascontiguousarray(i[rows, 1:3])
        exp_rays, exp_draws = e[rows, 0:7], e[rows, 7].astype(np.uint32)
        assert np.array_equal(exp_draws, T.draws[rows])
        if taped is not None:
            rays, draws = taped(cams[c], st, T.tape, np.ascontiguousarray(T.offsets[rows]))
            assert np.array_equal(draws, exp_draws), f"camera {c} (tape): draws differ at {np.nonzero(draws != exp_draws)[0][:5]}"
            assert bits_equal(rays, exp_rays), f"camera {c} (tape): " + mismatch_report(rays, exp_rays)
        nat = T.natural[rows]
        if keyed is not None and nat.any():
            rays, draws = keyed(cams[c], np.ascontiguousarray(st[nat]), np.ascontiguousarray(T.keys[rows][nat]))
            assert np.array_equal(draws, exp_draws[nat]), f"camera {c} (stream): draws differ"
            assert bits_equal(rays, exp_rays[nat]), f"camera {c} (stream): " + mismatch_report(rays, exp_rays[nat])
        n_checked += int(rows.sum())
    assert n_checked == len(i)


class BvhCase:
    """one (sphere set, builder) of ref_core_bvh_* or one given tree of ref_core_bvhgiven_*, as a flat BVH world"""

    def __init__(self, prefix, row, order=None, world_cls=O.World, node_dt=O.NODE_DT, prim_dt=O.PRIM_DT, mat_dt=O.MAT_DT):
        if prefix == "bvh":
            s_off, n, self.builder, n_off, nn, self.root, r_off, nr = [int(x) for x in row]
        else:
            s_off, n, n_off, nn, self.root, r_off, nr = [int(x) for x in row]
        self.spheres = SPH[prefix][s_off:s_off + n]
        self.nodes = NODES[prefix][n_off:n_off + nn].copy().view(node_dt)[:, 0] if node_dt is not None else None
        hitt = self.spheres if order is None else self.spheres[order]      # hittables[] order
        self.prims = _prims(hitt).astype(prim_dt)
        self.mats = np.zeros(1, dtype=mat_dt)
        self.mats["albedo"] = 0.5
        w = world_cls()
        w.kind, w.root, w.n_nodes, w.n_prims, w.n_materials, w.max_stack = 0, self.root, nn, n, 1, 32
        for k in range(3):
            w.bounds_min[k], w.bounds_max[k] = float(self.nodes["min"][self.root][k]), float(self.nodes["max"][self.root][k])
        w.nodes, w.prims, w.materials = self.nodes.ctypes.data, self.prims.ctypes.data, self.mats.ctypes.data
        self.world = w
        self.rays = np.ascontiguousarray(RAYS[prefix][r_off:r_off + nr])
        self.expect = OUTS[prefix][r_off:r_off + nr]


SPH = {p: gold(f"ref_core_{p}_spheres.f32", 8) for p in ("bvh", "bvhgiven")}
NODES = {p: gold(f"ref_core_{p}_nodes.f32", 8) for p in ("bvh", "bvhgiven")}
RAYS = {p: gold(f"ref_core_{p}_rays.f32", 7) for p in ("bvh", "bvhgiven")}
OUTS = {p: gold(f"ref_core_{p}_out.f32", 12) for p in ("bvh", "bvhgiven")}


def bvh_cases(prefix, **kw):
    if prefix == "bvh":
        idx, order = core("bvh_idx.i32", 8, "<i4"), np.fromfile(os.path.join(GOLD, "ref_core_bvh_order.i32"), dtype="<i4")
        o_off = np.concatenate([[0], np.cumsum(idx[:, 1])])
        return [BvhCase(prefix, r, order[o_off[j]:o_off[j] + r[1]], **kw) for j, r in enumerate(idx)]
    return [BvhCase(prefix, r, None, **kw) for r in core("bvhgiven_idx.i32", 7, "<i4")]


def check_bvh_trace(cases, trace_fn, counts_fn=None, order_fn=None):
    n_hits = 0
    for j, c in enumerate(cases):
        hit, t, prim = trace_fn(c.world, c.rays)
        e = c.expect
        assert np.array_equal(hit, e[:, 0].astype(np.int32)), f"case {j}: hit flags differ at rays {np.nonzero(hit != e[:, 0])[0][:5]}"
        assert bits_equal(t, e[:, 1]), f"case {j}: " + mismatch_report(t, e[:, 1])
        assert np.array_equal(prim, e[:, 2].astype(np.int32)), f"case {j}: closest hittable differs at rays {np.nonzero(prim != e[:, 2])[0][:5]}"
        if counts_fn is not None:
            leaf = counts_fn(c.world, c.rays)
            assert np.array_equal(leaf, e[:, 3].astype(np.uint32)), f"case {j}: leaves reached differ at rays {np.nonzero(leaf != e[:, 3])[0][:5]}"
        if order_fn is not None:
            order = order_fn(c.world, c.rays)
            assert np.array_equal(order, e[:, 4:12].astype(np.int32)), f"case {j}: leaf visiting order differs at rays {np.nonzero(np.any(order != e[:, 4:12], axis=1))[0][:5]}"
        n_hits += int(hit.sum())
    assert n_hits > 0.2 * sum(len(c.rays) for c in cases)


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_oracle_sphere_hittables_match_reference():
    """G5: _sphere_closest_intersection, (Moving)SphereHittable::ClosestIntersection with a preset rec.distance (`t >= rec.distance`
    rejects, equality included), getNormal: tangent rays with d == 0 exactly, origins inside / on / behind, negative radii,
    unnormalised directions, times 0 / 1 / mid, specials"""
    i, e = core("sphere_in.f32", 16), core("sphere_out.f32", 12)
    L = olib_core()
    n = len(i)
    static = i[:, 7] == 0
    t = np.zeros(int(static.sum()), np.float32)
    L.orc_sphere_batch(len(t), np.ascontiguousarray(i[static, 8:14]), np.ascontiguousarray(np.c_[i[static, 0:3], i[static, 6]]), t)
    assert bits_equal(t, e[static, 0]), "sphere t: " + mismatch_report(t, e[static, 0])
    prims, rays = _prims(i[:, 0:8]), np.ascontiguousarray(i[:, 8:15])
    hit, dist, nrm = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    L.orc_sphere_hit_batch(n, prims.ctypes.data, rays, np.ascontiguousarray(i[:, 15]), hit, dist, nrm)
    assert np.array_equal(hit, e[:, 1].astype(np.int32)), f"hit flags differ at {np.nonzero(hit != e[:, 1])[0][:5]}"
    assert bits_equal(dist, e[:, 2]), "rec.distance: " + mismatch_report(dist, e[:, 2])
    assert bits_equal(nrm, e[:, 3:6]), "normal: " + mismatch_report(nrm, e[:, 3:6])
    fresh = i[:, 15] == MISS   # with a fresh payload the hit distance IS _sphere_closest_intersection's t (or stays _MISS_DIST)
    assert bits_equal(dist[fresh], np.where(e[fresh, 0] >= MISS, MISS, e[fresh, 0]))
    tangent = (np.arange(n) % 16) == 1
    assert tangent.sum() == 256 and not e[tangent, 1].any()   # d == 0 exactly: `d <= 0` misses
    assert 0.3 < e[:, 1].mean() < 0.8 and (e[i[:, 15] < MISS, 1] == 0).any()


def test_product_sphere_bounds_match_reference():
    """getSphereBounds / getMovingSphereBounds (SphereHittable.cu:52-54, :85-89) in the product's host scene code"""
    i, e = core("sphere_in.f32", 16), core("sphere_out.f32", 12)
    fin = np.all(np.isfinite(i[:, 0:7]), axis=1)
    s = pkg().api.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    for k in np.nonzero(fin)[0][::3]:
        c0, c1, r = [float(x) for x in i[k, 0:3]], [float(x) for x in i[k, 3:6]], float(i[k, 6])
        p = s.MakeMovingSphere(c0, c1, r, m) if i[k, 7] > 0 else s.MakeSphere(c0, r, m)
        mn, mx = s.prim_bounds(p)
        assert bits_equal(np.r_[mn, mx], e[k, 6:12]), f"case {k}: " + mismatch_report(np.r_[mn, mx], e[k, 6:12])


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_product_bvh_builders_match_reference_factory(builder):
    """G6: the product's host builders (rt_scene_build_bvh_topdown / _sah / _bottomup) == BVH_Handle::Factory's rec1 / rec2 /
    bottom-up merge (BVH.cu:156-384): node array node for node, root, and the hittables[] order of the primitives"""
    api = pkg().api
    cases = [c for c in bvh_cases("bvh") if c.builder == builder]
    assert len(cases) >= 40
    for j, c in enumerate(cases):
        s = api.Scene()
        m = s.Lambertian((0.5, 0.5, 0.5))
        for sp in c.spheres:
            if sp[7] > 0:
                s.MakeMovingSphere([float(x) for x in sp[0:3]], [float(x) for x in sp[3:6]], float(sp[6]), m)
            else:
                s.MakeSphere([float(x) for x in sp[0:3]], float(sp[6]), m)
        (s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp)[builder]()
        nodes, prims, _ = s.arrays()
        assert s.getWorldPtr().root == c.root, f"set {j}: root"
        assert nodes.tobytes() == c.nodes.tobytes(), f"set {j}: node arrays differ"
        assert prims.tobytes() == c.prims.astype(prims.dtype).tobytes(), f"set {j}: hittables[] order differs"


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_oracle_bvh_builders_match_reference_factory(builder):
    for j, c in enumerate([c for c in bvh_cases("bvh") if c.builder == builder]):
        sc = O.Scene.from_arrays(_prims(c.spheres), c.mats, builder)
        assert sc.world.root == c.root, f"set {j}: root"
        assert sc.nodes.tobytes() == c.nodes.tobytes(), f"set {j}: node arrays differ"
        assert sc.prims.tobytes() == c.prims.tobytes(), f"set {j}: hittables[] order differs"


@pytest.mark.parametrize("prefix", ["bvh", "bvhgiven"])
def test_oracle_flat_bvh_matches_reference(prefix):
    """G6: BVH::ClosestIntersection (BVH.cu:54-106) over real SphereHittable leaves: closest hit, its hittable, leaves reached and
    the first 8 in visiting order —
    on the reference's own built trees and on given trees with duplicate spheres, coincident boxes, rays on box planes"""
    check_bvh_trace(bvh_cases(prefix), _oracle_trace, _oracle_counts, _oracle_order)


def test_oracle_scatter_matches_reference():
    """G7: a ray hits a real Sphere / MovingSphere, then Lambertian, Metal (fuzz 0 / 0.3 / 1), Dielectric (ior 1.5, 1/1.5, 1.333,
    2.4: front, back, TIR, hollow) and LambertianTexture (scale 0.32) scatter: flag, out ray, attenuation, draws"""
    i, e, T = core("scatter_in.f32", 23), core("scatter_out.f32", 16), Tapes("scatter")
    L = olib_core()
    n = len(i)
    assert np.array_equal(e[:, 15].astype(np.uint32), T.draws)
    mats, rays = _scatter_inputs(i, O.MAT_DT)
    # the hit that feeds Scatter
    hit, dist, nrm = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    prims = _prims(i[:, 0:8])
    L.orc_sphere_hit_batch(n, prims.ctypes.data, rays, np.full(n, MISS, np.float32), hit, dist, nrm)
    assert hit.all() and bits_equal(dist, e[:, 0]) and bits_equal(nrm, e[:, 1:4]), mismatch_report(np.c_[dist, nrm], e[:, 0:4])
    dist, nrm = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1:4])
    # every case on its tape
    sc, orays, att, draws = np.zeros(n, np.int32), np.zeros((n, 7), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    L.orc_scatter_tape(n, mats.ctypes.data, rays, dist, nrm, T.tape, T.offsets, sc, orays, att, draws)
    _check_scatter("tape", sc, orays, att, draws, e, T.draws)
    # natural cases on the generator's own stream
    nat = T.natural
    k = int(nat.sum())
    sc, orays, att, draws = np.zeros(k, np.int32), np.zeros((k, 7), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.uint32)
    nat_mats = np.ascontiguousarray(mats[nat])
    L.orc_scatter_batch(SEED, k, nat_mats.ctypes.data, np.ascontiguousarray(rays[nat]), np.ascontiguousarray(dist[nat]),
                        np.ascontiguousarray(nrm[nat]), np.ascontiguousarray(T.keys[nat]), sc, orays, att, draws)
    _check_scatter("stream", sc, orays, att, draws, e, T.draws[nat], nat)
    assert 2000 < k < n and 0.05 < (e[:, 4] == 0).mean() < 0.5


def test_scatter_fixture_reaches_the_tape_only_edges():
    """the adversarial tapes do reach what they are for: zero / unit-length / corner rejections, absorption by near_zero, u equal
    to reflect_prob, TIR without a draw"""
    i, e, T = core("scatter_in.f32", 23), core("scatter_out.f32", 16), Tapes("scatter")
    adv = ~T.natural
    first = T.tape[T.offsets[:, 0]]
    assert adv.sum() > 300
    assert ((first == 1 << 23) & adv).sum() >= 20 and ((first == 1 << 24) & adv).sum() >= 20 and ((first == 1) & adv).sum() >= 20
    lam_absorbed = adv & (i[:, 8] != 2) & (e[:, 4] == 0) & (i[:, 8] != 1)
    assert lam_absorbed.sum() >= 4                                         # normal + on-unit == 0 -> near_zero
    assert (adv & (i[:, 8] == 1) & (i[:, 12] == 1.0) & (e[:, 4] == 0)).sum() >= 2
    die = (i[:, 8] == 2) & adv
    assert die.sum() >= 288 and np.all(T.draws[die] == 1)
    assert ((i[:, 8] == 2) & (T.draws == 0)).sum() >= 16                  # TIR: `ior_ratio * sin_theta > 1` short-circuits the draw
    assert (T.draws >= 30).sum() >= 10                                     # runs of >= 10 rejections


def test_oracle_cameras_match_reference():
    """G8: the three cameras' constructors (the Book-1 final camera and several vfov / aspect / aperture) and sample_ray on the
    stream and on tapes (lens draws at the disc's edges, u = 1 for MotionBlur's mix)"""
    L = olib_core()
    cams = make_cameras((O.camera_pinhole, O.camera_defocus, O.camera_motion))
    check_camera_ctors(cams)

    def keyed(cam, st, keys):
        rays, draws = np.zeros((len(st), 7), np.float32), np.zeros(len(st), np.uint32)
        L.orc_camera_batch(SEED, C.byref(cam), len(st), st, keys, rays, draws)
        return rays, draws

    def taped(cam, st, tape, offsets):
        rays, draws = np.zeros((len(st), 7), np.float32), np.zeros(len(st), np.uint32)
        L.orc_camera_tape(C.byref(cam), len(st), st, tape, offsets, rays, draws)
        return rays, draws
    run_cameras(cams, keyed, taped)


def test_product_camera_ctors_match_reference():
    api = pkg().api
    check_camera_ctors(make_cameras((api.PinholeCamera, api.DefocusBlurCamera, api.MotionBlurCamera)))


def test_core_fixture_natural_tapes_are_the_product_stream():
    """a natural tape is the prefix of the generator's uniforms for (seed 1984, pixel, sample): what the key-driven probes draw"""
    for kind in ("scatter", "camera"):
        T = Tapes(kind)
        for r in np.nonzero(T.natural & (T.draws > 0))[0][::97]:
            u = np.zeros(int(T.draws[r]), np.float32)
            O.lib().orc_rng_uniforms(SEED, int(T.keys[r, 0]), int(T.keys[r, 1]), 0, len(u), u)
            k = T.tape[T.offsets[r, 0]:T.offsets[r, 0] + T.offsets[r, 1]]
            assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, k.astype(np.float64)), f"{kind} case {r}"


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_sphere_hittables_match_reference():
    p = pkg()
    i, e = core("sphere_in.f32", 16), core("sphere_out.f32", 12)
    static = i[:, 7] == 0
    t = p.api.probe_sphere(np.ascontiguousarray(i[static, 8:14]), np.ascontiguousarray(np.c_[i[static, 0:3], i[static, 6]]))
    assert bits_equal(t, e[static, 0]), "sphere t: " + mismatch_report(t, e[static, 0])
    # the leaf test itself, with rec.distance preset (`t >= rec.distance` rejects, equality included) or fresh
    hit, dist, nrm = p.api.probe_sphere_hit(_prims(i[:, 0:8]), i[:, 8:15], i[:, 15])
    assert np.array_equal(hit, e[:, 1].astype(np.int32)), f"hit flags differ at {np.nonzero(hit != e[:, 1])[0][:5]}"
    assert bits_equal(dist, e[:, 2]), "rec.distance: " + mismatch_report(dist, e[:, 2])
    assert bits_equal(nrm, e[:, 3:6]), "normal: " + mismatch_report(nrm, e[:, 3:6])
    assert (i[:, 15] < MISS).sum() > 400


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", ["bvh", "bvhgiven"])
def test_device_flat_bvh_matches_reference(prefix):
    p = pkg()

    def trace(world, rays):
        hit, t, prim, _ = p.api.probe_trace(world, rays)
        return hit, t, prim
    check_bvh_trace(bvh_cases(prefix, world_cls=p.capi.WorldFlat, node_dt=p.capi.NODE_DT, prim_dt=p.capi.PRIM_DT, mat_dt=p.capi.MAT_DT), trace)


@pytest.mark.gpu
def test_device_scatter_matches_reference():
    p = pkg()
    i, e, T = core("scatter_in.f32", 23), core("scatter_out.f32", 16), Tapes("scatter")
    mats, rays = _scatter_inputs(i, p.capi.MAT_DT)
    dist, nrm = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1:4])
    nat = T.natural
    sc, orays, att, draws = p.api.probe_scatter(SEED, np.ascontiguousarray(mats[nat]), rays[nat], dist[nat], nrm[nat], T.keys[nat])
    _check_scatter("stream", sc, orays, att, draws, e, T.draws[nat], nat)
    sc, orays, att, draws = p.api.probe_scatter_tape(mats, rays, dist, nrm, T.tape, T.offsets)
    _check_scatter("tape", sc, orays, att, draws, e, T.draws)


@pytest.mark.gpu
def test_device_cameras_match_reference():
    api = pkg().api
    cams = make_cameras((api.PinholeCamera, api.DefocusBlurCamera, api.MotionBlurCamera))
    run_cameras(cams, lambda cam, st, keys: api.probe_camera(SEED, cam, st, keys),
                lambda cam, st, tape, offsets: api.probe_camera_tape(cam, st, tape, offsets))
