"""A numpy float32 twin of the lens cameras (rt06.h: RT_CAM_PERSPECTIVE .. RT_CAM_PANORAMA) — test infrastructure only.

rule() restates lens_camera_draw / lens_camera_ray (csrc/rt_device_funcs.hpp) as rt06.h states them: the lens point iff lens_radius > 0, one uniform for the
time iff t0 != t1, then the projection and the lens, every operation a float32 operation rounded on its own, the sine from the oracle's orc_math_batch (fn 1 =
rt_sinf, pinned to the device's by tests/test_gpu_cornell.py) and cos x = sin(x + pi/2).  primary_rays() is _path_twin.primary_rays for these cameras — the
pixel centre, the jitter in a disc of half a pixel, then rule() — and delegates to it for types 0 to 2; use(monkeypatch) hands it to the whole-sample loop and
the first-hit twins, which look the name up in _path_twin at call time.  KTape serves rule() the uniforms of a caller's tape of k in [1, 2^24], as
rt_camera_rays_batch reads them.
"""
import numpy as np

import _path_twin as PT
from _nee_twin import F, _Tape
from _noise_twin import _sin

PERSPECTIVE, ORTHOGRAPHIC, FISHEYE, PANORAMA = 16, 17, 18, 19
HALF_PI = F(float.fromhex("0x1.921fb6p+0"))
_path_primary_rays = PT.primary_rays   # the loop's own, before use() replaces the module attribute


class KTape:
    """Per case a slice of a tape of k: u = k * 2^-24; past its end k = 2^23 + 1, and the count goes on (TapeRng, csrc/rt_probes.hip)"""

    def __init__(self, tape, offsets):
        self.k = np.ascontiguousarray(tape, np.uint32)
        off = np.ascontiguousarray(offsets, np.uint32).reshape(-1, 2).astype(np.int64)
        self.first, self.n = off[:, 0], off[:, 1]
        self.cur = np.zeros(len(off), np.int64)

    def next(self, rows):
        at = self.cur[rows]
        inside = at < self.n[rows]
        k = np.full(len(rows), 0x800001, np.uint32)
        k[inside] = self.k[(self.first[rows] + at)[inside]]
        self.cur[rows] += 1
        return k.astype(F) * F(2.0 ** -24)

    in_unit2 = _Tape.in_unit2


def _vec(v):
    return np.array(list(v), F)


def rule(cam, sx, sy, tape, rows):
    """The camera's draws from `tape` for the cases `rows` and its rays through (sx, sy): (origin (n, 3), direction (n, 3), time (n,))"""
    n = len(rows)
    sx, sy = np.ascontiguousarray(sx, F), np.ascontiguousarray(sy, F)
    o, u, v, w = _vec(cam.o), _vec(cam.u), _vec(cam.v), _vec(cam.w)
    a, b = F(cam.viewport_width), F(cam.viewport_height)
    lens, shutter = cam.lens_radius > 0, cam.t0 != cam.t1
    focus = F(cam.focus_dist)
    col = lambda x: x[:, None]
    with np.errstate(all="ignore"):
        if lens:
            la, lb = tape.in_unit2(rows)
            off = (u[None, :] * col(la) + v[None, :] * col(lb)) * F(cam.lens_radius)
        if shutter:
            x = tape.next(rows)
            time = F(cam.t0) * (F(1) - x) + F(cam.t1) * x
        else:
            time = np.full(n, F(cam.t0), F)
        ua, vb = u * a, v * b
        if cam.type == PERSPECTIVE:
            if lens:   # DefocusBlurCamera::sample_ray's own order
                forward, hori, vert = w * focus, ua * focus, vb * focus
                return o[None, :] + off, ((forward[None, :] + hori[None, :] * col(sx)) + vert[None, :] * col(sy)) - off, time
            return np.broadcast_to(o, (n, 3)).copy(), (w[None, :] + ua[None, :] * col(sx)) + vb[None, :] * col(sy), time
        o0, d0 = np.broadcast_to(o, (n, 3)).copy(), np.broadcast_to(w, (n, 3)).copy()
        if cam.type == ORTHOGRAPHIC:
            o0 = (o[None, :] + ua[None, :] * col(sx)) + vb[None, :] * col(sy)
        elif cam.type == FISHEYE:
            x, y = a * sx, b * sy
            th = np.sqrt(x * x + y * y)
            k = _sin(th) / th
            d = (w[None, :] * col(_sin(th + HALF_PI)) + u[None, :] * col(x * k)) + v[None, :] * col(y * k)
            off_axis = th != F(0)
            d0[off_axis] = d[off_axis]
        else:
            assert cam.type == PANORAMA, cam.type
            ph, lm = a * sx, b * sy
            cl = _sin(lm + HALF_PI)
            d0 = (w[None, :] * col(cl * _sin(ph + HALF_PI)) + u[None, :] * col(cl * _sin(ph))) + v[None, :] * col(_sin(lm))
        if lens:
            return o0 + off, d0 * focus - off, time
        return o0, d0, time


def batch(cam, st, tape, offsets):
    """rt_camera_rays_batch of a lens camera, restated: (rays (n, 7), draws (n,))"""
    st = np.ascontiguousarray(st, F).reshape(-1, 2)
    kt = KTape(tape, offsets)
    ray_o, ray_d, time = rule(cam, st[:, 0], st[:, 1], kt, np.arange(len(st)))
    rays = np.zeros((len(st), 7), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = ray_o, ray_d, time
    return rays, kt.cur.astype(np.uint32)


def primary_rays(cam, width, height, seed, gids, samples, timed=False):
    """_path_twin.primary_rays for every camera: types 0 to 2 are its own; a lens camera's are the pixel jitter, then rule().  Without `timed` the caller
    drops the rays' times, so the world must hold nothing that moves."""
    if cam.type < PERSPECTIVE:
        return _path_primary_rays(cam, width, height, seed, gids, samples, timed=timed)
    n = len(gids)
    tape = _Tape(seed, gids, samples)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        x, y = (gids % np.uint32(width)).astype(F), (gids // np.uint32(width)).astype(F)
        psx, psy = F(1) / F(width), F(1) / F(height)
        ndcx = ((x + F(0.5)) * psx) * F(2) - F(1)
        ndcy = ((y + F(0.5)) * psy) * F(2) - F(1)
        jx, jy = tape.in_unit2(rows)
        sx, sy = ndcx + jx * psx, ndcy + jy * psy
    ray_o, ray_d, time = rule(cam, sx, sy, tape, rows)
    if timed:
        rays = np.zeros((n, 7), F)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = ray_o, ray_d, time
        return tape, rays
    return tape, ray_o, ray_d


def use(monkeypatch):
    """From here to the end of the test, the whole-sample loop and the first-hit twins take their primary rays from this module"""
    monkeypatch.setattr(PT, "primary_rays", primary_rays)
