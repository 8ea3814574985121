"""The ground floor of the numpy float32 twins of one whole sample, and the twin with and without light sampling over quad lights — test
infrastructure only.

What this module owns: the float32 vector helpers, the tape of a sample's uniforms with the two rejection loops (_Tape), the quad lights of a world, quad::hit
restated (_quad_hit), the oracle's walk as the twins take one (oracle_trace), the resolve, and the counters of §16.  The sample's path itself — the pixel jitter,
the pinhole ray, the shade step of sample_world and the light-sampling estimator as rt06.h states it, every operation a float32 operation rounded on its own —
is tests/_path_twin.py's one loop; radiance() runs it over orc_trace_batch under _light_tree_twin.TableRule on the quad lights.
What it takes from the oracle: the uniforms of a sample (orc_rng_uniforms, on the stream id one_sample uses) and every closest
intersection (orc_trace_batch, through _oracle.py).  The per-light quad test of the density step is quad::hit restated here:
orc_trace_batch tests a world's bounds before its primitives, which the bare test the kernel calls does not.

Scope: pinhole cameras; worlds of spheres and quads with Lambertian, checker, metal and diffuse-light materials.  A sample that meets
anything else (a dielectric, a medium, a textured material) is not followed: its radiance is NaN and `followed` is False.

What a run exercised: radiance() and frame_samples() fill an optional `stats` dict (new_stats() names its counters), so that a test world can
be shown to reach the estimator's edges before a kernel is compared with it.  Counting reads the values the arithmetic produced; it changes none.
"""
import ctypes as C

import numpy as np

import _oracle as O

F = np.float32
MISS = F(3.402823466e+38)
STREAM_RENDER = 0          # the stream id of one_sample (rt_oracle.c) / RT_STREAM_RENDER
MAX_LIGHTS = 16
INV_PI = F(0.318309886)
PRIM_MOVING = 0x80000000


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0], x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], axis=1)


def near_zero(a):
    return ~(np.abs(a[:, 0]) > F(1e-9)) & ~(np.abs(a[:, 1]) > F(1e-9)) & ~(np.abs(a[:, 2]) > F(1e-9))


def quad_lights(quads, mats):
    """(quad indices, areas): the quads whose material is a diffuse light, in index order; area = sqrt(dot(n, n)), n = cross(u, v)."""
    idx = np.array([i for i in range(len(quads)) if mats["type"][quads["mat"][i]] == 4], dtype=np.uint32)
    if len(idx) == 0:
        return idx, np.zeros(0, F)
    n = cross(quads["u"][idx].astype(F), quads["v"][idx].astype(F))
    return idx, np.sqrt(dot(n, n))


class _Tape:
    """The uniforms of each sample, in draw order; grown from the start of the stream when a sample comes near the end of what it has."""

    def __init__(self, seed, gids, samples):
        self.seed, self.gids, self.samples = int(seed), gids, samples
        self.cur = np.zeros(len(gids), np.int64)
        self.len = 0
        self.u = np.zeros((len(gids), 0), F)
        self._grow(np.arange(len(gids)), 48)

    def _grow(self, rows, n):
        if n > self.len:
            wider = np.zeros((len(self.gids), n), F)
            wider[:, : self.len] = self.u
            self.u, self.len = wider, n
        fill, buf = O.lib().orc_rng_uniforms, np.zeros(n, F)
        for r in rows:
            fill(self.seed, int(self.gids[r]), int(self.samples[r]), STREAM_RENDER, n, buf)
            self.u[r, :n] = buf
        self.have = getattr(self, "have", np.zeros(len(self.gids), np.int64))
        self.have[rows] = n

    def next(self, rows):
        short = rows[self.cur[rows] >= self.have[rows]]
        if len(short):
            self._grow(short, max(self.len, 2 * int(self.have[short].max())))
        u = self.u[rows, self.cur[rows]]
        self.cur[rows] += 1
        return u

    def in_unit2(self, rows):
        """glm::cuRandomInUnit<2>: pairs of u * 2 - 1 until x*x + y*y < 1"""
        ox, oy = np.zeros(len(rows), F), np.zeros(len(rows), F)
        todo = np.arange(len(rows))
        while len(todo):
            x = self.next(rows[todo]) * F(2) - F(1)
            y = self.next(rows[todo]) * F(2) - F(1)
            ok = (x * x + y * y) < F(1)
            ox[todo[ok]], oy[todo[ok]] = x[ok], y[ok]
            todo = todo[~ok]
        return ox, oy

    def on_unit3(self, rows):
        """glm::cuRandomOnUnit<3>: triples of u * 2 - 1 until not near zero and inside the unit ball; then normalised"""
        out = np.zeros((len(rows), 3), F)
        todo = np.arange(len(rows))
        while len(todo):
            v = np.stack([self.next(rows[todo]) * F(2) - F(1) for _ in range(3)], axis=1)
            ok = ~near_zero(v) & (((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) < F(1))
            out[todo[ok]] = v[ok]
            todo = todo[~ok]
        inv = F(1) / np.sqrt(dot(out, out))
        return out * inv[:, None]


def new_stats():
    """light_samples[i]: light-half draws sent to light i; below_surface: light-half directions failed for pdf_cos == 0; cos_one_light /
    cos_many_lights: cosine-half directions that met one light / two or more; checker_light_half: checker hits that took the light half;
    light_half_unmet: light-half directions that no light's quad test accepts (the sampled point lies in a plane through the hit point: |denom| < 1e-8);
    index_clamped: light-index draws whose uniform is 1 (one in 2^24), so that only the min(..., n_l - 1) keeps the index inside the table;
    not_followed: samples that met something outside the twin's scope"""
    return {"light_samples": np.zeros(MAX_LIGHTS, np.int64), "below_surface": 0, "cos_one_light": 0, "cos_many_lights": 0, "checker_light_half": 0, "light_half_unmet": 0,
            "index_clamped": 0, "not_followed": 0}


def _quad_hit(q, o, d):
    """quad::hit (quad_closest_intersection) of one quad on rays (o, d) over a fresh trace's interval [0, MISS): (hit, t)"""
    n = np.broadcast_to(q["normal"].astype(F), d.shape)
    denom = dot(n, d)
    t = (F(q["D"]) - dot(n, o)) / denom
    hit = ~(np.abs(denom) < F(1e-8)) & ~(t < F(0)) & ~(t >= MISS)
    planar = (o + d * t[:, None]) - q["Q"].astype(F)[None, :]
    w = np.broadcast_to(q["w"].astype(F), d.shape)
    alpha = dot(w, cross(planar, np.broadcast_to(q["v"].astype(F), d.shape)))
    beta = dot(w, cross(np.broadcast_to(q["u"].astype(F), d.shape), planar))
    hit &= (alpha >= F(0)) & (alpha <= F(1)) & (beta >= F(0)) & (beta <= F(1))
    return hit, t


def oracle_trace(world, rays):
    """every closest intersection of rays (k, 7) by the oracle's orc_trace_batch: (hit, t, prim, normal)"""
    k = len(rays)
    hit, t, prim, normal = np.zeros(k, np.int32), np.zeros(k, F), np.zeros(k, np.int32), np.zeros((k, 3), F)
    assert O.lib().orc_trace_batch(C.byref(world), k, rays, hit, t, prim, normal) == 0
    return hit, t, prim, normal


def count(stats, key, n):
    """stats[key] += n where the caller's dict keeps that counter"""
    if key in stats:
        stats[key] += n


def radiance(world, cam, width, height, max_depth, seed, gids, samples, light_sampling=False, stats=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool).  world: _oracle.World, cam: _oracle.Camera (pinhole).
    stats: a dict of new_stats()'s shape (or an empty one, which is given it) that the run adds its counts to."""
    import _nee2_twin as T2   # (the table, the rule and the loop stand above this module)
    import _path_twin as PT
    return T2.table_radiance(world, cam, width, height, max_depth, seed, gids, samples, 1 if light_sampling else 0, PT.counters(stats, new_stats()), oracle_trace,
                             T2.lights_of, (0, 1))   # mode 1's table: quad_lights() above


def frame_samples(world, cam, width, height, spp, max_depth, seed, light_sampling=False, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    import _path_twin as PT
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, light_sampling, stats), width, height, spp, first_sample)


def luminance(rgb):
    return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def in_order_sums(samples):
    """(H, W, 4) float32 = (sum R, sum G, sum B, sum Y^2) of (H, W, spp, 3) samples, added in sample order as the resolve kernels add them"""
    h, w, spp, _ = samples.shape
    sums = np.zeros((h, w, 4), F)
    with np.errstate(all="ignore"):
        for s in range(spp):
            c = samples[:, :, s, :]
            sums[..., 0:3] = sums[..., 0:3] + c
            yy = luminance(c)
            sums[..., 3] = sums[..., 3] + yy * yy
    return sums


def resolve(sums, spp):
    """the framebuffer of `spp` accumulated samples: mean, clamp to [0, 1] with GLM's NaN rules, sqrt, alpha 1"""
    with np.errstate(all="ignore"):
        mean = sums[..., 0:3] * (F(1) / F(spp))
        lo = np.where(mean < F(0), F(0), mean)           # glm::max(x, 0) = (x < 0) ? 0 : x
        c = np.where(F(1) < lo, F(1), lo)                # glm::min(x, 1) = (1 < x) ? 1 : x
        out = np.ones(sums.shape[:2] + (4,), F)
        out[..., 0:3] = np.sqrt(c)
    return out
