"""First-hit feature buffers (rt_renderer_aov_*) on the GPU, against the CPU oracle only.

Expected sums: orc_rng_uniforms gives the draws of stream (pixel, s); the pixel-jitter rule (Renderer.cu:199, glm::cuRandomInUnit<2>) is restated
in numpy; orc_camera_tape is fed the remaining draws; orc_trace_batch traces the resulting rays; orc_checker_batch gives checker albedo; the
results are summed in numpy float32 in sample order.  Every comparison is exact equality of bits."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from _common import as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, pkg

pytestmark = pytest.mark.gpu
f32 = np.float32
N_DRAWS = 64   # per (pixel, sample): two rejection loops of acceptance pi/4 never come near it (checked below)
MOVING = 0x80000000


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def _arr(ptr, n, dt):
    return np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(ptr), dtype=dt).copy() if n and ptr else np.zeros(0, dt)


def primary_rays(cam, W, H, s_first, s_count, seed=1984):
    """rays (H*W, s_count, 7) of samples [s_first, s_first + s_count) of every pixel, from the oracle's RNG and camera"""
    L = O.lib()
    L.orc_camera_tape.argtypes = [C.POINTER(O.Camera), C.c_size_t, O.f32p, O.u32p, O.u32p, O.f32p, O.u32p]
    n = W * H * s_count
    u = np.zeros((n, N_DRAWS), f32)
    row = np.zeros(N_DRAWS, f32)
    i = 0
    for gid in range(W * H):
        for s in range(s_first, s_first + s_count):
            L.orc_rng_uniforms(seed, gid, s, 0, N_DRAWS, row)
            u[i] = row
            i += 1
    # pixel jitter: pairs (x, y) = (u * 2 - 1) until length2 = (0 + x*x) + y*y < 1
    sgn = u * f32(2.0) - f32(1.0)
    x, y = sgn[:, 0::2], sgn[:, 1::2]
    ok = (f32(0.0) + x * x) + y * y < f32(1.0)
    first = ok.argmax(axis=1)
    assert ok.any(axis=1).all()
    rows = np.arange(n)
    jx, jy = x[rows, first], y[rows, first]
    gid = np.repeat(np.arange(W * H), s_count)
    px, py = (gid % W).astype(f32), (gid // W).astype(f32)
    psx, psy = f32(1.0) / f32(W), f32(1.0) / f32(H)
    ndcx = (px + f32(0.5)) * psx * f32(2.0) - f32(1.0)
    ndcy = (py + f32(0.5)) * psy * f32(2.0) - f32(1.0)
    st = np.ascontiguousarray(np.stack([ndcx + jx * psx, ndcy + jy * psy], axis=1), f32)
    used = (2 * (first + 1)).astype(np.uint32)
    tape = np.ascontiguousarray((u * f32(16777216.0)).astype(np.uint32).reshape(-1))
    offsets = np.ascontiguousarray(np.stack([rows.astype(np.uint32) * N_DRAWS + used, N_DRAWS - used], axis=1).reshape(-1), np.uint32)
    rays = np.zeros((n, 7), f32)
    draws = np.zeros(n, np.uint32)
    L.orc_camera_tape(C.byref(as_oracle_camera(cam)), n, st, tape, offsets, rays, draws)
    assert (draws <= N_DRAWS - used).all(), "a camera ran past its tape"
    return rays.reshape(W * H, s_count, 7)


def checker_albedo(mats, pos):
    """orc_checker_batch takes the texture's scale and inverts it: find the scale whose reciprocal IS the stored inv_scale"""
    L = O.lib()
    L.orc_checker_batch.argtypes = [C.c_size_t, O.f32p, O.f32p]
    inp = np.zeros((len(pos), 10), f32)
    inp[:, 0:3], inp[:, 3:6], inp[:, 7:10] = mats["albedo"], mats["albedo2"], pos
    for k, inv in enumerate(mats["param"]):
        up = down = f32(1.0) / f32(inv)
        cand = [up]
        for _ in range(4):
            up, down = np.nextafter(up, f32(np.inf)), np.nextafter(down, f32(-np.inf))
            cand += [up, down]
        good = [s for s in cand if f32(1.0) / f32(s) == f32(inv)]
        assert good, f"no scale inverts to {inv}"
        inp[k, 6] = good[0]
    out = np.zeros((len(pos), 3), f32)
    L.orc_checker_batch(len(pos), np.ascontiguousarray(inp), out)
    return out


def expected_sums(w, cam, W, H, n_samples, s_first=0, start=None):
    """(H, W, 8) float32: the feature sums of samples [s_first, s_first + n_samples), continued from `start`"""
    ow = as_oracle_world(w)
    rays = primary_rays(cam, W, H, s_first, n_samples)
    n = W * H * n_samples
    flat = np.ascontiguousarray(rays.reshape(n, 7))
    hit, t, prim, nrm = np.zeros(n, np.int32), np.zeros(n, f32), np.zeros(n, np.int32), np.zeros((n, 3), f32)
    assert O.lib().orc_trace_batch(C.byref(ow), n, flat, hit, t, prim, nrm) == 0
    prims, quads, mats = _arr(ow.prims, ow.n_prims, O.PRIM_DT), _arr(ow.quads, ow.n_quads, O.QUAD_DT), _arr(ow.materials, ow.n_materials, O.MAT_DT)
    alb = np.ones((n, 3), f32)
    h = hit != 0
    mat_of = np.zeros(n, np.int64)
    is_quad = h & (prim >= ow.n_prims)
    is_sph = h & ~is_quad
    mat_of[is_sph] = prims["mat"][prim[is_sph]] & ~np.uint32(MOVING)
    if ow.n_quads:
        mat_of[is_quad] = quads["mat"][prim[is_quad] - ow.n_prims]
    mtype = mats["type"][mat_of]
    plain = h & ((mtype == 0) | (mtype == 1))
    alb[plain] = mats["albedo"][mat_of[plain]]
    chk = h & (mtype == 3)
    if chk.any():
        pos = flat[chk, 0:3] + flat[chk, 3:6] * t[chk, None]   # Ray::at, each operation rounded on its own
        alb[chk] = checker_albedo(mats[mat_of[chk]], pos)
    assert not (h & (mtype >= 5)).any()
    contrib = np.zeros((n, 8), f32)
    contrib[h, 0:3], contrib[h, 3], contrib[h, 7] = nrm[h], t[h], f32(1.0)
    contrib[:, 4:7] = alb
    contrib = contrib.reshape(W * H, n_samples, 8)
    sums = np.zeros((W * H, 8), f32) if start is None else start.reshape(W * H, 8).copy()
    for s in range(n_samples):   # in sample order; a miss adds nothing to normal / depth / hits (x + 0 keeps x's bits: no sum is -0)
        sums = (sums + contrib[:, s]).astype(f32)
    return sums.reshape(H, W, 8), float(h.mean())


def node_tree_scene(p, n=48, seed=7):
    rng = np.random.default_rng(seed)
    s = p.Scene()
    refs = []
    for i in range(n):
        m = [s.Lambertian, lambda a: s.Metal(a, 0.3), lambda a: s.Dielectric((1, 1, 1), 1.5)][i % 3](rng.random(3, dtype=f32))
        c = (rng.random(3, dtype=f32) * 2 - 1) * 4
        c[2] -= 8
        refs.append(s.prim_ref(s.MakeSphere(c, float(rng.random() * 0.8 + 0.2), m)))
    while len(refs) > 1:
        nxt = [s.bvh_node(refs[i], refs[i + 1]) for i in range(0, len(refs) - 1, 2)]
        if len(refs) % 2:
            nxt.append(refs[-1])
        refs = nxt
    s.set_world_node_tree(refs[0])
    return s


CASES = {"three_spheres": (64, 48), "book1_final": (203, 117), "book2_moving": (96, 64), "cornell_box": (64, 64), "node_tree": (64, 48),
         # the world's own traversal rule is the feature pass's too: the distance-sorted queue (two LDS stacks) and the 4-wide walk
         "book2_moving@queue": (96, 64), "book1_final@wide4": (90, 60), "cornell_box@queue": (48, 48)}


def make_case(p, which):
    W, H = CASES[which]
    if which == "node_tree":
        return node_tree_scene(p), p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 70.0, W / H), W, H
    base, _, walk = which.partition("@")
    scene = config_scene(p, base)
    if walk:
        scene.set_traversal({"queue": 1, "wide4": 2}[walk])
    return scene, config_cameras(p, base, W, H), W, H


@pytest.mark.parametrize("which", list(CASES))
def test_feature_sums_are_the_oracles_bits(p, which):
    scene, cam, W, H = make_case(p, which)
    w = scene.getWorldPtr()
    assert w.kind == {"three_spheres": 1, "node_tree": 2}.get(which, 0)
    assert w.traversal == {"queue": 1, "wide4": 2}.get(which.partition("@")[2], 0)
    r = p.Renderer.MakeRenderer(W, H, 16, 12, cam, w)
    r.enable_aov()
    assert r.aov_info() == {"enabled": True, "samples": 0, "bytes": ((W + 7) // 8) * ((H + 7) // 8) * 64 * 32}
    r.refine(16)
    assert r.aov_info()["samples"] == 16
    got = r.aov_sums()
    exp, hit_rate = expected_sums(w, cam, W, H, 16)
    assert 0.05 < hit_rate <= 1.0
    assert bits_equal(got, exp), mismatch_report(got, exp)
    f = r.aov()
    assert bits_equal(f["albedo"], exp[..., 4:7] * (f32(1.0) / f32(16))) and bits_equal(f["coverage"], exp[..., 7] * (f32(1.0) / f32(16)))
    r.close()


def test_steps_equal_one_step_and_a_render_between_disturbs_nothing(p, monkeypatch):
    monkeypatch.setenv("RT06_PASS_SPP", "2")   # read at creation: every step spans several internal passes
    scene, cam, W, H = make_case(p, "book1_final")
    w = scene.getWorldPtr()
    a = p.Renderer.MakeRenderer(W, H, 4, 12, cam, w)
    a.enable_aov()
    a.refine(3)
    a.Render()
    a.refine(5)
    a.set_camera(cam)   # the same bytes: kept
    a.refine(8)
    monkeypatch.delenv("RT06_PASS_SPP")
    b = p.Renderer.MakeRenderer(W, H, 16, 12, cam, w)
    b.enable_aov()
    b.refine(16)
    off = p.Renderer.MakeRenderer(W, H, 16, 12, cam, w)
    off.refine(16)
    assert off.aov_info() == {"enabled": False, "samples": 0, "bytes": 0}
    assert a.aov_info()["samples"] == 16
    assert bits_equal(a.aov_sums(), b.aov_sums()), mismatch_report(a.aov_sums(), b.aov_sums())
    # the colour path does not know the feature pass: frame and sums have the bits of a renderer without it
    for r in (a, b):
        assert bits_equal(r.DownloadRenderbuffer(), off.DownloadRenderbuffer())
        assert bits_equal(r.refine_sums(), off.refine_sums())
    for r in (a, b, off):
        r.close()


def test_max_samples_is_honoured_and_reported(p, monkeypatch):
    monkeypatch.setenv("RT06_PASS_SPP", "4")   # 6 ends inside the second pass
    scene, cam, W, H = make_case(p, "book2_moving")
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 4, 12, cam, w)
    r.enable_aov(6)
    r.refine(5)
    assert r.aov_info()["samples"] == 5
    r.refine(7)
    assert r.aov_info()["samples"] == 6 and r.refine_info()["samples"] == 12
    exp, _ = expected_sums(w, cam, W, H, 6)
    assert bits_equal(r.aov_sums(), exp), mismatch_report(r.aov_sums(), exp)
    r.refine(4)   # past the limit: the feature pass is skipped, the buffers stay
    assert r.aov_info()["samples"] == 6 and bits_equal(r.aov_sums(), exp)
    r.close()


def test_camera_change_and_reset_discard_the_buffers(p):
    scene, cam, W, H = make_case(p, "three_spheres")
    cam2 = p.PinholeCamera((0.5, 0.3, 0.4), (0, 0, -1), (0, 1, 0), 70.0, W / H)
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, 8, 12, cam, w)
    r.enable_aov()
    r.refine(8)
    r.set_camera(cam2)
    assert r.aov_info()["samples"] == 0
    with pytest.raises(p.capi.RtError):
        r.aov_sums()
    r.refine(4)
    exp, _ = expected_sums(w, cam2, W, H, 4)
    assert r.aov_info()["samples"] == 4 and bits_equal(r.aov_sums(), exp), mismatch_report(r.aov_sums(), exp)
    r.refine_reset()
    assert r.aov_info()["samples"] == 0
    r.set_camera(cam)
    r.refine(4)
    exp, _ = expected_sums(w, cam, W, H, 4)
    assert bits_equal(r.aov_sums(), exp)
    r.close()


def test_refusals(p):
    W, H = 32, 32
    scene, cam = config_scene(p, "book1_final"), config_cameras(p, "book1_final", W, H)
    base = p.Renderer.MakeRenderer(W, H, 4, 8, cam, scene.getWorldPtr(), variant=1)
    with pytest.raises(p.capi.RtError, match="variant 1"):
        base.enable_aov()
    base.close()
    shard = p.Renderer.MakeRenderer(W, H, 4, 8, cam, scene.getWorldPtr(), rank=1, world_size=2)
    shard.enable_aov()
    shard.refine(4)   # a shard accumulates its own pixels
    assert shard.aov_info()["samples"] == 4
    with pytest.raises(p.capi.RtError, match="shard"):
        shard.aov_sums()
    with pytest.raises(p.capi.RtError, match="shard"):
        shard.denoise()
    shard.close()
    for mtype, word in ((p.capi.MAT_ISOTROPIC, "medium"), (p.capi.MAT_LAMBERTIAN_NOISE, "noise"), (p.capi.MAT_LAMBERTIAN_IMAGE, "image")):
        s = p.Scene()
        if mtype == p.capi.MAT_LAMBERTIAN_NOISE:
            s.set_perlin(1984)
        if mtype == p.capi.MAT_LAMBERTIAN_IMAGE:
            s.set_image(np.full((4, 8, 3), 128, np.uint8))
        m = s.add_material(mtype, (0.5, 0.5, 0.5), 0.5)
        s.MakeSphere((0, 0, -2), 0.5, m)
        s.MakeSphere((0, -100.5, -2), 100.0, s.Lambertian((0.5, 0.5, 0.5)))
        s.BuildBVH_TopDown()
        r = p.Renderer.MakeRenderer(W, H, 4, 8, p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, 1.0), s.getWorldPtr())
        with pytest.raises(p.capi.RtError, match=word):
            r.enable_aov()
        r.refine(2)   # refinement itself goes on without the feature pass
        r.close()
