"""Triangle worlds beyond the numpy twin's scope, on the GPU against the CPU oracle, bit for bit on every pixel and every ray.

The oracle reads a quad's kind and is pinned to the twin on it without a GPU (tests/test_triangles_cpu.py, pins 3 and 4), so here it judges what the twin cannot
follow: dielectrics on triangles, moving spheres, the defocus and motion-blur cameras, media, noise and image textures, the lane walks, worlds around the
`quad index >= n_plain_quads` boundary, a mesh too big for the LDS, random worlds.  Every world comes from tests/_tri_worlds.py, where test_triangles_cpu.py
asserts what it holds.  Every test names the kernel it ran through kernel_form() and kernel_triangles()."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
import _tri_twin as TT
import _tri_worlds as TW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg
from test_light_sampling_cpu import plain_samples

pytestmark = pytest.mark.gpu
F = np.float32
QUEUE_WORLD = 3   # RT_WORLD_BVH_QUEUE: the key of both lane walks


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


class Expected:
    """the oracle's frame of a world and, on request, the in-order sums of its per-sample radiance; computed once, never modified"""

    def __init__(self, scene, cam, w, h, spp, depth):
        self.scene, self.cam, self.args = scene, cam, (w, h, spp, depth)
        self.world, self.ocam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam)
        self.frame, _ = O.render(self.world, self.ocam, w, h, spp, depth, TW.SEED)
        self.frame.setflags(write=False)

    @functools.cached_property
    def sums(self):
        w, h, spp, depth = self.args
        sums = TT.in_order_sums(plain_samples(self.world, self.ocam, w, h, spp, depth))
        assert bits_equal(TT.resolve(sums, spp), self.frame)   # the oracle's two entry points agree with one another
        sums.setflags(write=False)
        return sums


@functools.lru_cache(maxsize=None)
def wide_room_expected(ext, as_list, cam_kind, medium=True):
    p = pkg()
    return Expected(TW.wide_room(p, ext=ext, as_list=as_list, medium=medium), TW.camera(p, kind=cam_kind), TW.W, TW.H, TW.SPP, TW.DEPTH)


def check_frame(img, exp):
    assert np.array_equal(np.isnan(img), np.isnan(exp)) and bits_equal(img, exp), mismatch_report(img, exp)


# ---- a, b: the wide room and the EXT 2 room, every stack-walk and list form, three cameras -----------------------------------------------------------
@pytest.mark.parametrize("cam_kind", TW.CAMERAS)
@pytest.mark.parametrize("form", list(TW.FORMS), ids=[TW.form_id(f) for f in TW.FORMS])
def test_every_triangle_instantiation_renders_the_wide_room_as_the_oracle_does(p, monkeypatch, form, cam_kind):
    """The sixteen RT_KERNEL_TRI keys on what the twin cannot follow: a glass icosphere, a fuzzy-metal tetrahedron, a moving sphere and a background behind an
    opening; the EXT 2 keys plus an image-textured and a noise-textured triangle and a sphere of medium.  Frame and refinement sums, every pixel, two passes
    and uneven refine steps."""
    world, exact, ext, big, wide = form
    variant, env = TW.FORMS[form]
    as_list = world == TW.LIST
    exp = wide_room_expected(ext, as_list, cam_kind)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RT06_PASS_SPP", "3")
    scene = TW.wide_room(p, ext=ext, as_list=as_list)
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, scene.getWorldPtr(), seed=TW.SEED, variant=variant)
    assert r.kernel_form() == TW.kernel_form_of(form) and r.kernel_triangles()
    r.Render()
    img = r.DownloadRenderbuffer()
    check_frame(img, exp.frame)
    r.refine(1)
    r.refine(3)
    check_frame(r.refine_sums(), exp.sums)
    assert bits_equal(r.DownloadRenderbuffer(), img)
    r.close()
    assert not bits_equal(exp.frame, wide_room_expected(ext, as_list, "pinhole" if cam_kind != "pinhole" else "defocus").frame)   # the camera is in the frame


def test_a_medium_beside_triangles_is_accepted(p):
    """the host takes a constant medium together with triangles (nothing refuses it), so the EXT 2 room above keeps its medium; it is in view: without it the frame differs"""
    with_medium, without = wide_room_expected(2, False, "pinhole"), wide_room_expected(2, False, "pinhole", medium=False)
    assert not bits_equal(with_medium.frame, without.frame)
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, with_medium.cam, with_medium.scene.getWorldPtr(), seed=TW.SEED)
    assert r.kernel_form()["ext"] == 2 and r.kernel_triangles()
    r.close()


# ---- c: the group boundary -----------------------------------------------------------------------------------------------------------------------------
WALKS = {   # name: (as a list, kernel variant, traversal)
    "stack-exact": (False, 2, 0), "stack-fast": (False, 3, 0), "queue": (False, 0, 1), "wide4": (False, 0, 2), "list": (True, 0, 0),
}
BOUNDARY = ("triangles_only", "one_quad", "one_triangle", "siblings")


@functools.lru_cache(maxsize=None)
def boundary_expected(which, as_list, traversal):
    p = pkg()
    builder = "MakeHittableList" if as_list else ("BuildBVH_SAH" if which == "siblings" else "BuildBVH_TopDown")
    return Expected(TW.boundary_world(p, which, builder, traversal), TW.boundary_camera(p), TW.W, TW.H, TW.SPP, TW.DEPTH)


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("which", BOUNDARY)
def test_worlds_around_the_group_boundary_render_as_the_oracle_does(p, which, walk):
    """`(code - first_quad) >= n_plain_quads` with no parallelogram at all (and no sphere: n_prims == 0), with exactly one, with one triangle behind many, and
    with the last parallelogram and the first triangle under one inner node: the stack walk exact and fast, the list and both lane walks (the baseline kernel: below)."""
    as_list, variant, traversal = WALKS[walk]
    exp = boundary_expected(which, as_list, traversal)
    w = exp.scene.getWorldPtr()
    assert w.traversal == traversal and w.kind == int(as_list)
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, w, seed=TW.SEED, variant=variant)
    form = r.kernel_form()
    if traversal:
        assert form == TW.kernel_form_of((TW.BVH, 1, 1, 1, 1)) | {"world": QUEUE_WORLD} and not r.kernel_triangles()   # a lane walk reads the kind from the flat record
    else:
        assert form == TW.kernel_form_of((TW.LIST if as_list else TW.BVH, int(variant != 3), 1, 0, 0)) and r.kernel_triangles()
    r.Render()
    check_frame(r.DownloadRenderbuffer(), exp.frame)
    r.refine(TW.SPP)
    check_frame(r.refine_sums(), exp.sums)
    r.close()
    assert exp.frame[..., :3].std() > 0.05   # something is in view


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
@pytest.mark.parametrize("which", BOUNDARY)
def test_the_baseline_kernel_renders_the_boundary_worlds_as_the_oracle_does(p, which, as_list):
    """The baseline kernel (variant 1) reads the kind from the flat record.  Held to the oracle's frame bit for bit, as every comparison of this file is.

    The regression test of a finding: these worlds' sky leaves no sample black, and while the kernel added a pixel's samples pairwise across its
    lanes, 16 to 83 of a frame's 4096 words were one unit in the last place (5.96e-8) off the oracle's in-order sum, in all eight cases.  It adds them in sample order now."""
    exp = boundary_expected(which, as_list, 0)
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, exp.scene.getWorldPtr(), seed=TW.SEED, variant=1)
    assert r.kernel_form()["kernel"] == "baseline" and not r.kernel_triangles()
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    differ = img.view(np.uint32) != exp.frame.view(np.uint32)
    print(f"baseline {which} {'list' if as_list else 'bvh'}: {int(differ.sum())} of {differ.size} words differ, max |delta| {float(np.nanmax(np.abs(img - exp.frame))):.3e}")
    check_frame(img, exp.frame)


# ---- d: a mesh that does not fit the LDS by itself -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_room_expected(level):
    p = pkg()
    return Expected(TW.mesh_room(p, level), TW.camera(p), TW.W, TW.H, 2, TW.DEPTH)


@pytest.mark.parametrize("variant", [2, 3])
def test_a_mesh_too_big_for_the_lds_takes_the_global_memory_form_by_itself(p, variant):
    """icosphere(4), 5120 triangles of glass, in the room, nothing forced: accepted, and sent to the global-memory form; icosphere(2) in the same room stays in
    the LDS, so the pair brackets the switch.  Both against the oracle."""
    assert "RT06_FORCE_BIG" not in os.environ and "RT06_FORCE_WIDE" not in os.environ
    for level, big in ((2, 0), (4, 1)):
        exp = mesh_room_expected(level)
        r = p.Renderer.MakeRenderer(TW.W, TW.H, 2, TW.DEPTH, exp.cam, exp.scene.getWorldPtr(), seed=TW.SEED, variant=variant)
        form = r.kernel_form()
        assert form == TW.kernel_form_of((TW.BVH, int(variant == 2), 1, big, form["wide"])) and form["wide"] <= big and r.kernel_triangles()
        assert r.kernel_info()["lds_resident"] == (not big)
        r.Render()
        check_frame(r.DownloadRenderbuffer(), exp.frame)
        r.refine(2)
        check_frame(r.refine_sums(), exp.sums)
        r.close()
    assert not bits_equal(mesh_room_expected(2).frame, mesh_room_expected(4).frame)


# ---- e: random triangle worlds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(12)))
def test_random_triangle_worlds_render_bit_exact(p, seed):
    """Modelled on test_gpu_parity.test_random_scenes_cameras_and_builders_render_bit_exact, and like it on the default variant, which that test holds to the
    oracle's bits with no allowance; the baseline kernel (variant 1) gets none there and is not run here (the boundary worlds above run it)."""
    scene, cam, W, H, spp, depth, recipe = TW.random_tri_world(p, seed)
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, seed=TW.SEED)
    form = r.kernel_form()
    recipe["kernel"] = form
    assert form["kernel"] == "stream" and form["ext"] == recipe["ext"] and form["world"] == w.kind and r.kernel_triangles(), recipe
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    ref, _ = O.render(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, depth, TW.SEED)
    assert np.array_equal(np.isnan(img), np.isnan(ref)), recipe
    assert bits_equal(img, ref), f"{recipe}: " + mismatch_report(img, ref)


# ---- f: probes -----------------------------------------------------------------------------------------------------------------------------------------------
def orc_trace(w, rays):
    n = len(rays)
    hit, t, prim, normal = np.zeros(n, np.int32), np.zeros(n, F), np.zeros(n, np.int32), np.zeros((n, 3), F)
    assert O.lib().orc_trace_batch(C.byref(w), n, np.ascontiguousarray(rays, F), hit, t, prim, normal) == 0
    return hit, t, prim, normal


def check_probe(p, scene, rays):
    got = p.api.probe_trace(scene.getWorldPtr(), rays)
    exp = orc_trace(as_oracle_world(scene.getWorldPtr()), rays)
    for name, g, e in zip(("hit", "t", "primitive", "normal"), got, exp):
        assert bits_equal(np.asarray(g, F), np.asarray(e, F)), name + ": " + mismatch_report(np.asarray(g, F), np.asarray(e, F))
    return exp


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_probe_trace_on_the_wide_room_is_the_oracles(p, as_list):
    scene = TW.wide_room(p, as_list=as_list)
    hit, _, prim, _ = check_probe(p, scene, TW.room_rays(4096, timed=True))
    n_prims = scene.getWorldPtr().n_prims
    assert (prim >= n_prims + 6).sum() > 400 and (prim == 0).any() and (hit == 0).any()   # triangles, the moving sphere, the opening


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_probe_trace_at_every_vertex_edge_and_face_of_a_closed_mesh_is_the_oracles(p, as_list):
    """rays from outside a closed icosphere(2) at its 162 vertices, 480 edge midpoints and 320 centroids.  Only agreement with the oracle is asserted, whatever
    the answer at a shared edge is: how many rays pass through is printed, a measurement (watertightness)."""
    scene, rays, (nv, ne, nf) = TW.closed_mesh_world(p, as_list)
    hit = check_probe(p, scene, rays)[0]
    print(f"closed icosphere(2), {'list' if as_list else 'bvh'}: {int((hit == 0).sum())} of {len(rays)} rays pass through")


# ---- g: feature buffers --------------------------------------------------------------------------------------------------------------------------------------
def test_feature_buffers_of_the_wide_room_under_the_defocus_camera_are_the_oracles(p):
    import test_gpu_aov as A
    exp = wide_room_expected(1, False, "defocus")
    w = exp.scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, w, seed=TW.SEED)
    assert r.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 1, 0, 0)) and r.kernel_triangles()
    r.enable_aov()
    r.refine(1)
    r.refine(TW.SPP - 1)
    got = r.aov_sums()
    sums, hit_rate = A.expected_sums(w, exp.cam, TW.W, TW.H, TW.SPP)
    assert 0.5 < hit_rate < 1.0   # the opening is in view
    assert bits_equal(got, sums), mismatch_report(got, sums)
    r.close()


# ---- h: two and three ranks ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 3])
def test_ranks_render_the_ext_2_room_through_the_memcpy_transport(p, monkeypatch, ranks):
    exp = wide_room_expected(2, False, "motion")
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    one = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, exp.scene.getWorldPtr(), seed=TW.SEED)
    assert one.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 2, 0, 0)) and one.kernel_triangles()   # what every rank runs on its share
    one.close()
    m = p.MultiRenderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, exp.scene.getWorldPtr(), ranks, seed=TW.SEED)
    m.Render()
    check_frame(m.DownloadRenderbuffer(), exp.frame)
    m.close()


# ---- the fuzzer ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fuzz_campaign_runs_twenty_worlds_with_triangles(p):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_campaign.py"), "--seeds", "20"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    done = [line for line in res.stdout.splitlines() if line.startswith("DONE: 20 worlds, 0 failures")]
    assert done and "'triangle_worlds':" in done[0] and "'tri_kernels':" in done[0], res.stdout[-2000:]
