"""The default hot loop's far planes as one fma each (csrc/rt_fastdiv.hpp: CERTIFIED FAR PLANES, ONE FMA EACH) on the GPU.

The probe runs the box pair as the kernel takes it — slab_far_fma and far_pair_uncertain_fma, the helpers the hot loop calls, with the per-ray offset and margin
of begin-trace and the exact redo — next to aabb::intersects verbatim: the two hit flags and the order must be equal on every regular case, with the redo well
exercised.  The frames — Book-1 final and Book-2 moving, whole, cut into passes, and as 1/8 shards — must be the CPU oracle's bits, and so must a frame whose
primary rays are outside the regular class (they take the verbatim loop, which this form does not touch).  The arithmetic itself is restated in numpy by
tests/test_far_plane_fma_bound.py."""
import numpy as np
import pytest

import _oracle as O
from _common import as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, pkg, random_rays
from test_gpu_baseline_configs import _sharded

pytestmark = pytest.mark.gpu

DEPTH = 8
SIZES = [(240, 160, 24), (61, 37, 4)]
WORLDS = ["book1_final", "book2_moving"]
F32_MAX = np.float32(3.402823466e38)


@pytest.fixture(scope="module")
def p():
    m = pkg()
    assert m.api.device_count() >= 1, "no HIP device: the gpu tests need an MI355X"
    return m


_refs = {}


def _world(p, which, W, H):
    return config_scene(p, which), config_cameras(p, which, W, H)


def _reference(key, w, cam, W, H, spp):
    """the oracle's frame: computed once per world and size, shared, never written to"""
    key = (key, W, H, spp)
    if key not in _refs:
        ref, _ = O.render(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, DEPTH)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _probe_cases(n, seed):
    """Box pairs and rays of the families the certificate exists for: sibling boxes that share faces, flat boxes, rays aimed exactly at corners and edge points
    (far within a few ulp of tmin), origins on a face plane (a plane equal to the origin component: q = 0), near-axis-parallel rays that start far from the
    boxes (|o / d| up to 2^20 |t|), rec_t on the entry distance; directions of both signs throughout."""
    rng = np.random.default_rng(seed)
    lo = ((rng.random((n, 3), dtype=np.float32) * 2 - 1) * 12).astype(np.float32)
    ext = (rng.random((n, 3), dtype=np.float32) * 3 + 0.01).astype(np.float32)
    ext[rng.random((n, 3)) < 0.03] = 0.0
    left = np.concatenate([lo, lo + ext], axis=1)
    shift = np.where(rng.random((n, 3)) < 0.5, 0.0, rng.random((n, 3)) * 2 - 1).astype(np.float32)
    rlo = (lo + shift * ext).astype(np.float32)
    rext = np.where(rng.random((n, 3)) < 0.5, ext, (rng.random((n, 3), dtype=np.float32) * 3 + 0.01)).astype(np.float32)
    right = np.concatenate([rlo, rlo + rext], axis=1)
    boxes = np.ascontiguousarray(np.concatenate([left, right], axis=1), dtype=np.float32)
    rays = random_rays(rng, n, with_time=False)
    e = n // 8
    # [0, 2e): aimed exactly at a corner of the left box; [2e, 4e): at a point of an edge of the right box
    corner = np.where(rng.random((2 * e, 3)) < 0.5, left[:2 * e, 0:3], left[:2 * e, 3:6]).astype(np.float32)
    rays[:2 * e, 3:6] = (corner - rays[:2 * e, 0:3]) * (rng.random((2 * e, 1), dtype=np.float32) + 0.5)
    k = np.arange(2 * e, 4 * e)
    edge = np.where(rng.random((2 * e, 3)) < 0.5, right[k, 0:3], right[k, 3:6]).astype(np.float32)
    free = rng.integers(0, 3, 2 * e)
    t = rng.random(2 * e, dtype=np.float32)
    edge[np.arange(2 * e), free] = (right[k, 0:3][np.arange(2 * e), free] * (1 - t) + right[k, 3:6][np.arange(2 * e), free] * t).astype(np.float32)
    rays[k, 3:6] = (edge - rays[k, 0:3]) * (rng.random((2 * e, 1), dtype=np.float32) * 3 + 0.25)
    # [4e, 5e): the origin ON one, two or three face planes of the left box
    k = np.arange(4 * e, 5 * e)
    on = rng.random((e, 3)) < 0.4
    on[np.arange(e), rng.integers(0, 3, e)] = True
    face = np.where(rng.random((e, 3)) < 0.5, left[k, 0:3], left[k, 3:6])
    rays[k, 0:3] = np.where(on, face, rays[k, 0:3])
    # [5e, 6e): near-axis-parallel rays from far away, half of them still aimed at a corner: one or two direction components scaled down by up to 2^20
    k = np.arange(5 * e, 6 * e)
    rays[k, 0:3] *= np.exp2(rng.integers(0, 6, (e, 1))).astype(np.float32)
    aim = k[: e // 2]
    corner = np.where(rng.random((len(aim), 3)) < 0.5, right[aim, 0:3], right[aim, 3:6]).astype(np.float32)
    rays[aim, 3:6] = corner - rays[aim, 0:3]
    small = rng.random((e, 3)) < 0.5
    small[np.arange(e), rng.integers(0, 3, e)] = False
    rays[k, 3:6] = np.where(small, rays[k, 3:6] * np.exp2(-rng.integers(1, 21, (e, 3))).astype(np.float32), rays[k, 3:6])
    # [6e, 8e): the random tail
    maxd = np.where(rng.random(n) < 0.5, F32_MAX, rng.random(n, dtype=np.float32) * 30).astype(np.float32)
    return boxes, np.ascontiguousarray(rays, np.float32), maxd, e


def test_probe_takes_the_verbatim_decisions_and_exercises_the_redo(p):
    n = 1 << 20
    boxes, rays, maxd, e = _probe_cases(n, 53)
    hit, dist = p.api.probe_aabb(np.ascontiguousarray(boxes[:, 0:6]), rays, np.full(n, F32_MAX, np.float32))
    kk = np.where(hit[:e] == 1)[0]
    maxd[kk] = dist[kk]                                # rec_t exactly on the left box's entry distance
    out = p.api.probe_boxpair_certified_fma(boxes, rays, maxd)
    reg = out[:, 0] == 1
    redo = out[reg, 1].mean()
    tail = np.zeros(n, bool)
    tail[6 * e:] = True
    tail &= reg & (boxes[:, 3:6] > boxes[:, 0:3]).all(axis=1) & (boxes[:, 9:12] > boxes[:, 6:9]).all(axis=1)
    plain = out[tail, 1].mean()
    print(f"one-fma far planes: exact redo on {redo:.3f} of {reg.sum()} adversarial visits, {plain:.2e} of the random ones; "
          f"hit_left {out[reg, 5].mean():.3f}, swap {out[reg, 7].mean():.3f}")
    assert reg.mean() > 0.9
    assert np.array_equal(out[reg, 2], out[reg, 5]), f"hit_left differs in {(out[reg, 2] != out[reg, 5]).sum()} cases"
    assert np.array_equal(out[reg, 3], out[reg, 6]), f"hit_right differs in {(out[reg, 3] != out[reg, 6]).sum()} cases"
    assert np.array_equal(out[reg, 4], out[reg, 7]), f"near/far order differs in {(out[reg, 4] != out[reg, 7]).sum()} cases"
    assert redo >= 0.1          # the redo path is really exercised
    assert plain < 1e-3         # and random visits of boxes with thickness almost never take it
    assert out[reg, 5].mean() > 0.02 and out[reg, 7].mean() > 0.005


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("W,H,spp", SIZES)
@pytest.mark.parametrize("which", WORLDS)
def test_frames_are_the_oracles(p, which, W, H, spp, variant):
    s, cam = _world(p, which, W, H)
    w = s.getWorldPtr()
    ref = _reference(which, w, cam, W, H, spp)
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w, variant=variant)
    info = r.kernel_info()
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    assert info["variant"] == 3 and info["lds_resident"], info      # the instantiation that takes the fma form
    assert bits_equal(img, ref), f"{which} {W}x{H}x{spp} variant {variant}: " + mismatch_report(img, ref)


def test_forced_pass_cut_is_the_oracles(p, monkeypatch):
    """24 spp in passes of 7, 7, 7 and 3"""
    W, H, spp = SIZES[0]
    s, cam = _world(p, "book2_moving", W, H)
    w = s.getWorldPtr()
    ref = _reference("book2_moving", w, cam, W, H, spp)
    monkeypatch.setenv("RT06_PASS_SPP", "7")
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w)
    assert r.pass_info()["n_passes"] == 4
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(img, ref), mismatch_report(img, ref)


def test_one_eighth_shards_are_the_oracles(p):
    W, H, spp = SIZES[0]
    s, cam = _world(p, "book1_final", W, H)
    w = s.getWorldPtr()
    ref = _reference("book1_final", w, cam, W, H, spp)
    got = _sharded(p, W, H, spp, DEPTH, cam, w, 8)
    assert bits_equal(got, ref), mismatch_report(got, ref)


def test_rays_outside_the_regular_class_still_match(p):
    """An axis-parallel view (primary rays with exactly zero direction components) and a camera origin component of 1e-30 (every primary ray outside the
    class, the scattered ones inside): the former are stepped by the verbatim loop, the latter by the fma form, in the same waves."""
    s = config_scene(p, "book1_final")
    w = s.getWorldPtr()
    W, H, spp = 96, 64, 4
    for name, cam in (("axis", p.PinholeCamera((0, 1, 12), (0, 1, 0), (0, 1, 0), 40.0, W / H)),
                      ("tiny", p.DefocusBlurCamera((1e-30, 2.0, 9.0), (0, 0.5, 0), (0, 1, 0), 35.0, W / H, 0.0, 9.0))):
        ref = _reference(name, w, cam, W, H, spp)
        r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w)
        r.Render()
        img = r.DownloadRenderbuffer()
        r.close()
        assert bits_equal(img, ref), f"{name}: " + mismatch_report(img, ref)
