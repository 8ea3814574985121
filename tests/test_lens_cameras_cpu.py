"""Lens cameras without a GPU: rt_camera_rays_batch against the numpy twin bit for bit over all sixteen forms; a type-16 copy of each reference
camera against the original and the oracle's orc_camera_tape; the projections and the lens against float64 formulas, inside a tolerance derived from rt_sinf's
stated error; a full panorama against the environment map texel for texel; every refusal; the C and C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _lens_twin as LT
import _oracle as O
from _common import ROOT, as_oracle_camera, bits_equal, mismatch_report, pkg

F = np.float32
W, H = 20, 12                      # the frame of tests/test_gpu_lens_cameras.py: `just past the edge` is |s| = 1 + 1/W
EPS = 2.0 ** -24                   # fp32 unit roundoff
SIN_ERR = 3e-7                     # rt_sinf's worst absolute error as the project states it: tests/test_oracle_golden.py::test_extension_math_is_accurate, |x| < 2000
# One component of a direction along the basis is a sine of an argument that carries at most four roundings of a value <= pi (x = a s, y = b t, their squares' sum,
# the square root — or the + pi/2 of the cosine), times factors that add six more roundings (k = sin / th, x k, the three products with the basis and two sums):
DIR_ERR = SIN_ERR + (4 * np.pi + 6) * EPS
ANGLE_TOL = 2 * DIR_ERR            # an angle read off a direction of length 1 - 2 DIR_ERR or more moves by at most sqrt(2) DIR_ERR / |d|


@pytest.fixture(scope="module")
def p():
    return pkg()


def forms(p, lens_shutter=((False, False), (False, True), (True, False), (True, True))):
    """(name, camera) of the four projections x lens x shutter"""
    frm, at, up = (3.0, 2.0, -4.0), (0.5, 0.25, 1.0), (0.1, 1.0, 0.05)
    out = []
    for lens, shutter in lens_shutter:
        rest = (0.3 if lens else 0.0, 4.5, 0.25, 0.75 if shutter else 0.25)
        out += [(f"perspective lens={lens} shutter={shutter}", p.api.PerspectiveCamera(frm, at, up, 35.0, W / H, *rest)),
                (f"orthographic lens={lens} shutter={shutter}", p.api.OrthographicCamera(frm, at, up, 3.0, W / H, *rest)),
                (f"fisheye lens={lens} shutter={shutter}", p.api.FisheyeCamera(frm, at, up, 180.0, W / H, *rest)),
                (f"panorama lens={lens} shutter={shutter}", p.api.PanoramaCamera(frm, at, up, 360.0, 180.0, *rest))]
    return out


def cases(n_random=300, seed=7):
    """(st (n, 2), tape, offsets (n, 2)): the centre, the four corners, points just past each edge, a seeded random set; eight uniforms a case, the last cases fewer"""
    rng = np.random.default_rng(seed)
    e = 1.0 + 1.0 / W
    fixed = [(0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (e, 0.3), (-e, -0.3), (0.2, 1 + 1 / H), (-0.2, -(1 + 1 / H)), (e, 1 + 1 / H)]
    st = np.concatenate([np.array(fixed, F), (rng.random((n_random, 2)) * 2 - 1).astype(F)])
    n = len(st)
    tape = rng.integers(1, (1 << 24) + 1, 8 * n).astype(np.uint32)
    offsets = np.stack([np.arange(n) * 8, np.full(n, 8)], axis=1).astype(np.uint32)
    offsets[-3:, 1] = (0, 1, 2)    # tapes that may run out: the count goes on past them
    return st, tape, offsets


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_batch_is_the_twin_bit_for_bit(p):
    st, tape, offsets = cases()
    seen = set()
    for name, cam in forms(p):
        rays, draws = p.api.camera_rays_batch(cam, st, tape, offsets)
        want, want_draws = LT.batch(cam, st, tape, offsets)
        assert bits_equal(rays, want), (name, mismatch_report(rays, want))
        assert (draws == want_draws).all(), (name, np.nonzero(draws != want_draws)[0][:5])
        lens, shutter = cam.lens_radius > 0, cam.t0 != cam.t1
        full = offsets[:, 1] == 8
        assert (draws[full] >= 2 * lens + shutter).all() and ((draws[full] - shutter) % 2 == 0).all() and (lens or (draws == shutter).all())
        assert (lens and (draws[full] > 3).any()) or not lens   # some lens point was rejected at least once
        assert np.isfinite(rays).all()
        assert (rays[:, 6] == cam.t0).all() if not shutter else (np.unique(rays[:, 6]).size > 100)
        seen.add((cam.type, lens, shutter))
    assert len(seen) == 16


def test_a_type_16_copy_of_a_reference_camera_is_that_camera(p):
    """rays and draws, bit for bit, and the originals are the oracle's orc_camera_tape"""
    st, tape, offsets = cases()
    L = O.lib()
    L.orc_camera_tape.argtypes = [C.POINTER(O.Camera), C.c_size_t, O.f32p, O.u32p, O.u32p, O.f32p, O.u32p]
    frm, at, up = (13, 2, 3), (0, 0, 0), (0, 1, 0)
    originals = [p.PinholeCamera(frm, at, up, 20.0, W / H), p.DefocusBlurCamera(frm, at, up, 20.0, W / H, 0.1, 10.0), p.MotionBlurCamera(frm, at, up, 20.0, W / H, 0.0, 1.0)]
    for cam in originals:
        rays, draws = p.api.camera_rays_batch(cam, st, tape, offsets)
        orc_rays, orc_draws = np.zeros_like(rays), np.zeros_like(draws)
        L.orc_camera_tape(C.byref(as_oracle_camera(cam)), len(st), np.ascontiguousarray(st.reshape(-1)), tape, np.ascontiguousarray(offsets.reshape(-1)), orc_rays, orc_draws)
        assert bits_equal(rays, orc_rays) and (draws == orc_draws).all(), (cam.type, mismatch_report(rays, orc_rays))
        copy = lens_copy(p, cam)
        got, got_draws = p.api.camera_rays_batch(copy, st, tape, offsets)
        assert bits_equal(got, rays), (cam.type, mismatch_report(got, rays))
        assert (got_draws == draws).all(), cam.type
    defocus = originals[1]
    built = p.api.PerspectiveCamera(frm, at, up, 20.0, W / H, 0.1, 10.0)   # the constructor's record is that copy, byte for byte
    assert bytes(built) == bytes(lens_copy(p, defocus))


def lens_copy(p, cam):
    """the type-16 record that is the reference camera `cam` (rt06.h)"""
    c = type(cam).from_buffer_copy(bytes(cam))
    c.type = 16
    if cam.type == 1:
        c.t0 = c.t1 = 0.0
    else:
        c.viewport_width = c.viewport_height = 1.0
        c.lens_radius = 0.0
        if cam.type == 0:
            c.t0 = c.t1 = 0.0
    return c


# ---- 3. geometry against float64 -------------------------------------------------------------------------------------------------------------------------------------
def basis64(cam):
    return tuple(np.array(list(v), np.float64) for v in (cam.o, cam.u, cam.v, cam.w))


def directions64(cam, st):
    """(o0, d0) of the projection in float64 from the record's fp32 fields"""
    o, u, v, w = basis64(cam)
    a, b = float(cam.viewport_width), float(cam.viewport_height)
    s, t = st[:, 0].astype(np.float64)[:, None], st[:, 1].astype(np.float64)[:, None]
    o0, d0 = np.broadcast_to(o, (len(st), 3)), np.broadcast_to(w, (len(st), 3))
    if cam.type == 16:
        d0 = w + u * a * s + v * b * t
    elif cam.type == 17:
        o0 = o + u * a * s + v * b * t
    elif cam.type == 18:
        x, y = a * s, b * t
        th = np.sqrt(x * x + y * y)
        k = np.where(th > 0, np.sin(th) / np.where(th > 0, th, 1), 1.0)
        d0 = w * np.cos(th) + u * x * k + v * y * k
    else:
        ph, lm = a * s, b * t
        d0 = w * np.cos(lm) * np.cos(ph) + u * np.cos(lm) * np.sin(ph) + v * np.sin(lm)
    return o0, d0


def test_projections_and_lens_against_float64(p):
    st, tape, offsets = cases()
    inside = (np.abs(st) <= 1).all(axis=1)
    for name, cam in forms(p):
        rays, _ = p.api.camera_rays_batch(cam, st, tape, offsets)
        ro, rd = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
        o, u, v, w = basis64(cam)
        a, b, f = float(cam.viewport_width), float(cam.viewport_height), float(cam.focus_dist)
        lens = cam.lens_radius > 0
        o0, d0 = directions64(cam, st)
        if lens:   # ray.o + ray.d lies on the focus surface o0 + d0 f: the direction's error times f, and the roundings of sums of terms this large
            scale = np.abs(o).max() + a + b + 2 * cam.lens_radius + f * (1 + a + b if cam.type == 16 else 1)
            tol = f * DIR_ERR + 12 * EPS * scale
            miss = np.abs((ro + rd) - (o0 + d0 * f)).max()
            assert miss <= tol, (name, miss, tol)
            continue
        if cam.type == 17:
            assert (rays[:, 3:6] == np.array(list(cam.w), F)[None, :]).all(), name          # every direction IS w
            off_plane = np.abs((ro - o) @ w).max()
            assert off_plane <= 12 * EPS * (np.abs(o).max() + a + b), (name, off_plane)     # the origins lie in the plane through o
            assert np.abs((ro - o) @ u - a * st[:, 0]).max() <= 12 * EPS * (np.abs(o).max() + a + b), name
        elif cam.type == 18:
            th = np.sqrt((a * st[:, 0].astype(np.float64)) ** 2 + (b * st[:, 1].astype(np.float64)) ** 2)
            angle = np.arctan2(np.linalg.norm(np.cross(rd, w), axis=1), rd @ w)
            short = th <= np.pi    # a point past two edges at once lies beyond the back pole, where the angle folds: no sample of a frame reaches it
            assert short.sum() == len(th) - 1 and not inside[~short].any()
            assert np.abs(angle - th)[short].max() <= ANGLE_TOL, (name, np.abs(angle - th)[short].max(), ANGLE_TOL)
            assert th[short].max() > 3.0 and angle[0] == 0.0                                       # the corner nears the back pole; the centre is w itself
            assert (rays[0, 3:6] == np.array(list(cam.w), F)).all()
        elif cam.type == 19:
            lat = np.arctan2(rd @ v, np.hypot(rd @ w, rd @ u))
            assert np.abs(lat - b * st[:, 1])[inside].max() <= ANGLE_TOL, (name, np.abs(lat - b * st[:, 1])[inside].max())
            cl = np.cos(b * st[:, 1].astype(np.float64))
            away = inside & (cl > 1e-3) & (np.abs(st[:, 0]) < 1)                            # a longitude is read off a vector of length cos(latitude)
            lon = np.arctan2(rd @ u, rd @ w)
            err = np.abs(lon - a * st[:, 0])[away] * cl[away]
            assert err.max() <= ANGLE_TOL, (name, err.max())
        assert np.abs(rd - d0).max() <= (DIR_ERR if cam.type >= 18 else 8 * EPS * (1 + a + b)), (name, np.abs(rd - d0).max())


# ---- 4. a full panorama sees an unrotated map texel for texel ------------------------------------------------------------------------------------------------------------
def test_a_full_panorama_meets_the_environment_map_texel_for_texel(p):
    MW, MH = 64, 32
    rng = np.random.default_rng(11)
    image = rng.random((MH, MW, 3)).astype(F)
    cam = p.api.PanoramaCamera((0, 0, 0), (1, 0, 0), (0, 1, 0))
    assert tuple(cam.u) == (0.0, 0.0, -1.0) and tuple(cam.w) == (1.0, 0.0, 0.0)
    ys, xs = np.divmod(np.arange(MW * MH), MW)
    fraction = 0.99
    ang = np.arange(8) * (np.pi / 4) + 0.1
    jitters = [(0.0, 0.0)] + [(fraction * np.cos(q), fraction * np.sin(q)) for q in ang]
    psx, psy = F(1) / F(MW), F(1) / F(MH)
    for jx, jy in jitters:
        sx = (((xs.astype(F) + F(0.5)) * psx) * F(2) - F(1)) + F(jx) * psx
        sy = (((ys.astype(F) + F(0.5)) * psy) * F(2) - F(1)) + F(jy) * psy
        st = np.stack([sx, sy], axis=1).astype(F)
        own = ((MH - 1 - ys) * MW + xs).astype(np.uint32)
        ph, lm = np.pi * sx.astype(np.float64), (np.pi / 2) * sy.astype(np.float64)   # the inputs first: the float64 direction, rounded, lands in the pixel's own texel
        d64 = np.stack([np.cos(lm) * np.cos(ph), np.sin(lm), -np.cos(lm) * np.sin(ph)], axis=1).astype(F)
        _, texel = p.api.environment_batch(image, 0.0, d64)
        assert (texel == own).all(), ("float64 directions", jx, jy, np.nonzero(texel != own)[0][:5])
        rays, _ = p.api.camera_rays_batch(cam, st, np.zeros(0, np.uint32), np.zeros((len(st), 2), np.uint32))
        rgb, texel = p.api.environment_batch(image, 0.0, rays[:, 3:6])
        assert (texel == own).all(), ("the rule's directions", jx, jy, np.nonzero(texel != own)[0][:5])
        assert bits_equal(rgb, image.reshape(-1, 3)[own])


# ---- 5. validation -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_records_are_refused_and_the_field_is_named(p):
    st, tape, offsets = cases(n_random=4)
    frm, at, up = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    good = p.api.FisheyeCamera(frm, at, up, 120.0, 1.5, 0.2, 3.0, 0.0, 1.0)

    def refused(cam, word):
        with pytest.raises(p.capi.RtError) as e:
            p.api.camera_rays_batch(cam, st, tape, offsets)
        assert word in str(e.value), (word, str(e.value))

    for field in ("viewport_width", "viewport_height", "lens_radius", "focus_dist", "t0", "t1"):
        for bad in (float("nan"), float("inf")):
            c = type(good).from_buffer_copy(bytes(good))
            setattr(c, field, bad)
            refused(c, field)
    for field in ("o", "u", "v", "w"):
        c = type(good).from_buffer_copy(bytes(good))
        getattr(c, field)[1] = float("nan")
        refused(c, f"field {field} ")
    for field, bad in (("viewport_width", 0.0), ("viewport_height", -1.0), ("lens_radius", -0.1), ("focus_dist", 0.0)):
        c = type(good).from_buffer_copy(bytes(good))
        setattr(c, field, bad)
        refused(c, field)
    c = type(good).from_buffer_copy(bytes(good))
    c.lens_radius, c.focus_dist = 0.0, 0.0       # no lens: the focus distance is not read
    p.api.camera_rays_batch(c, st, tape, offsets)
    for t in (3, 15, 20):
        c = type(good).from_buffer_copy(bytes(good))
        c.type = t
        refused(c, "unknown camera type")
    out = p.capi.Camera()
    out.type = 77
    lib = p.capi.lib()
    v3 = p.capi.v3
    assert lib.rt_camera_fisheye(v3(frm), v3(at), v3(up), 300.0, 1.6, 0.0, 1.0, 0.0, 0.0, C.byref(out)) != 0 and out.type == 77   # corner >= pi; nothing written
    assert b"pi" in lib.rt_last_error() and b"rt_camera_fisheye" in lib.rt_last_error()
    p.api.FisheyeCamera(frm, at, up, 180.0, W / H)                                   # the GPU tests' fisheye: corner 3.05 < pi
    with pytest.raises(p.capi.RtError, match="viewport_width"):
        p.api.PanoramaCamera(frm, at, up, 361.0, 180.0)
    with pytest.raises(p.capi.RtError, match="viewport_height"):
        p.api.PanoramaCamera(frm, at, up, 360.0, 181.0)
    with pytest.raises(p.capi.RtError, match="viewport_width"):   # a window of no height has no width either: the first of the two is named
        p.api.OrthographicCamera(frm, at, up, 0.0, 1.0)
    with pytest.raises(p.capi.RtError, match="focus_dist"):
        p.api.PerspectiveCamera(frm, at, up, 40.0, 1.0, 0.5, -1.0)
    with pytest.raises(p.capi.RtError, match="lens_radius"):
        p.api.PerspectiveCamera(frm, at, up, 40.0, 1.0, -0.5, 1.0)
    full = p.api.PanoramaCamera(frm, at, up, 360.0, 180.0)
    assert full.viewport_width == F(np.pi) and full.viewport_height == F(np.pi / 2)
    ortho = p.api.OrthographicCamera(frm, at, up, 3.0, 2.0)
    assert (ortho.viewport_width, ortho.viewport_height) == (3.0, 1.5) and ortho.type == 17


# ---- 6. the C and C++ surface --------------------------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_and_cpp_mirror_build():
    d = os.path.join(ROOT, "tests", "cpp_lens_cameras")
    subprocess.check_call(["make", "-s", "-C", d])
    out = subprocess.run([os.path.join(d, "lens_cameras_abi_check")], capture_output=True, text=True)
    assert out.returncode == 0 and "lens cameras ABI ok" in out.stdout, out.stdout + out.stderr
    assert os.path.exists(os.path.join(d, "lens_cameras_app"))   # the mirror compiles and links; tests/test_gpu_lens_cameras.py runs it
