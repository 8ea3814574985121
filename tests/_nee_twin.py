"""A numpy float32 restatement of one whole sample, with and without light sampling — test infrastructure only.

What it takes from the oracle: the uniforms of a sample (orc_rng_uniforms, on the stream id one_sample uses) and every closest
intersection (orc_trace_batch, through _oracle.py).  What it restates: the pixel jitter's rejection loop, the pinhole ray, the shade
step of sample_world — Lambertian, checker, metal, diffuse light, the sky — and the light-sampling estimator as rt06.h states it,
every operation a float32 operation rounded on its own.  The per-light quad test of the density step is quad::hit restated here:
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


def radiance(world, cam, width, height, max_depth, seed, gids, samples, light_sampling=False, stats=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool).  world: _oracle.World, cam: _oracle.Camera (pinhole).
    stats: a dict of new_stats()'s shape (or an empty one, which is given it) that the run adds its counts to."""
    assert cam.type == 0, "the twin restates the pinhole camera"
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims = np.frombuffer((C.c_char * (world.n_prims * O.PRIM_DT.itemsize)).from_address(world.prims), O.PRIM_DT) if world.n_prims else np.zeros(0, O.PRIM_DT)
    quads = np.frombuffer((C.c_char * (world.n_quads * O.QUAD_DT.itemsize)).from_address(world.quads), O.QUAD_DT) if world.n_quads else np.zeros(0, O.QUAD_DT)
    mats = np.frombuffer((C.c_char * (world.n_materials * O.MAT_DT.itemsize)).from_address(world.materials), O.MAT_DT)
    light_idx, light_area = quad_lights(quads, mats)
    n_l = len(light_idx)
    if light_sampling:
        assert 1 <= n_l <= MAX_LIGHTS
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)

    if stats is not None:
        for key, zero in new_stats().items():
            stats.setdefault(key, zero)
    tape = _Tape(seed, gids, samples)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        # one_sample: pixel centre in NDC, jitter in a disc of half a pixel, PinholeCamera::sample_ray
        x, y = (gids % np.uint32(width)).astype(F), (gids // np.uint32(width)).astype(F)
        psx, psy = F(1) / F(width), F(1) / F(height)
        ndcx = ((x + F(0.5)) * psx) * F(2) - F(1)
        ndcy = ((y + F(0.5)) * psy) * F(2) - F(1)
        jx, jy = tape.in_unit2(rows)
        sx, sy = ndcx + jx * psx, ndcy + jy * psy
        co, cu, cv, cw = (np.array(list(v), F) for v in (cam.o, cam.u, cam.v, cam.w))
        ray_o = np.broadcast_to(co, (n, 3)).copy()
        ray_d = (cw[None, :] + cu[None, :] * sx[:, None]) + cv[None, :] * sy[:, None]

        atten = np.ones((n, 3), F)
        accum = np.zeros((n, 3), F)
        out = np.zeros((n, 3), F)
        followed = np.ones(n, bool)
        live = rows.copy()   # samples whose path goes on
        for bounce in range(max_depth):
            if len(live) == 0:
                break
            k = len(live)
            rays = np.zeros((k, 7), F)
            rays[:, 0:3], rays[:, 3:6] = ray_o[live], ray_d[live]
            hit, t, prim, normal = np.zeros(k, np.int32), np.zeros(k, F), np.zeros(k, np.int32), np.zeros((k, 3), F)
            assert O.lib().orc_trace_batch(C.byref(world), k, rays, hit, t, prim, normal) == 0
            o, d = rays[:, 0:3], rays[:, 3:6]
            # miss: the sky (Renderer.cu:150-151) or the constant background
            miss = hit == 0
            if miss.any():
                dm = d[miss]
                if world.background == 1:
                    sky = np.broadcast_to(np.array(list(world.background_color), F), dm.shape)
                else:
                    inv = F(1) / np.sqrt(dot(dm, dm))
                    tt = (dm[:, 1] * inv) * F(0.5) + F(0.5)
                    a, b = np.array([0.1, 0.2, 0.4], F), np.array([0.9, 0.9, 0.99], F)
                    sky = a[None, :] + (b - a)[None, :] * tt[:, None]
                out[live[miss]] = atten[live[miss]] * sky + accum[live[miss]]
            mi = mat_of_prim[np.where(miss, 0, prim)]
            mt = np.where(miss, -1, m_type[mi])
            # a light: emits, never scatters
            lit = mt == 4
            accum[live[lit]] = accum[live[lit]] + atten[live[lit]] * m_albedo[mi[lit]]
            out[live[lit]] = accum[live[lit]]
            other = ~miss & ~lit & ~np.isin(mt, (0, 1, 3))
            followed[live[other]] = False
            out[live[other]] = np.nan
            go = np.isin(mt, (0, 1, 3))
            if bounce + 1 >= max_depth:   # the last allowed bounce: whatever it scatters into is never traced
                out[live[go]] = accum[live[go]]
                break
            sel = np.nonzero(go)[0]
            r = live[sel]
            o, d, t, normal, mi, mt = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel]
            hit_p = o + d * t[:, None]
            k = len(r)
            lamb = mt != 1
            ok = np.ones(k, bool)
            new_d = np.zeros((k, 3), F)
            weight = np.ones(k, F)
            weighted = np.zeros(k, bool)
            to_light = np.zeros(k, bool)
            if light_sampling and lamb.any():
                c = tape.next(r[lamb])
                to_light[np.nonzero(lamb)[0]] = c < F(0.5)
            if to_light.any():
                s = np.nonzero(to_light)[0]
                li = np.zeros(len(s), np.int64)
                if n_l > 1:
                    scaled = (tape.next(r[s]) * F(n_l)).astype(np.uint32)
                    li = np.minimum(scaled, np.uint32(n_l - 1)).astype(np.int64)
                    if stats is not None:
                        stats["index_clamped"] += int((scaled >= n_l).sum())
                la = tape.next(r[s])
                lb = tape.next(r[s])
                if stats is not None:
                    stats["light_samples"] += np.bincount(li, minlength=MAX_LIGHTS)
                    stats["checker_light_half"] += int((mt[s] == 3).sum())
                q = quads[light_idx[li]]
                new_d[s] = ((q["Q"].astype(F) + q["u"].astype(F) * la[:, None]) + q["v"].astype(F) * lb[:, None]) - hit_p[s]
            s = np.nonzero(~to_light)[0]
            if len(s):
                on_unit = tape.on_unit3(r[s])
                sl, sm = s[lamb[s]], s[~lamb[s]]
                new_d[sl] = normal[sl] + on_unit[lamb[s]]
                ok[sl] = ~near_zero(new_d[sl])
                dn = dot(normal[sm], d[sm])
                refl = d[sm] - (normal[sm] * dn[:, None]) * F(2)
                new_d[sm] = refl + on_unit[~lamb[s]] * m_param[mi[sm]][:, None]
                ok[sm] = ~((dot(new_d[sm], normal[sm]) < F(0)) | near_zero(new_d[sm]))
            albedo = m_albedo[mi].copy()
            chk = np.nonzero(mt == 3)[0]
            if len(chk):   # checker_texture::value: ivec3 truncation of pos * scale, parity of the sum
                sp = hit_p[chk] * m_param[mi[chk]][:, None]
                ssum = np.trunc(sp).astype(np.int64).sum(axis=1)
                albedo[chk] = np.where((ssum % 2 == 0)[:, None], m_albedo[mi[chk]], m_albedo2[mi[chk]])
            if light_sampling:
                s = np.nonzero(lamb & ok)[0]
                if len(s):
                    dd, nn, hp = new_d[s], normal[s], hit_p[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    pdf_light = np.zeros(len(s), F)
                    met = np.zeros(len(s), np.int64)   # lights the direction meets (stats only)
                    for j in range(n_l):
                        q = quads[light_idx[j]]
                        qhit, qt = _quad_hit(q, hp, dd)
                        nj = np.broadcast_to(q["normal"].astype(F), dd.shape)
                        pl = ((qt * qt) * len2) / ((np.abs(dot(dd, nj)) / ln) * light_area[j])
                        pdf_light = pdf_light + np.where(qhit, pl, F(0)).astype(F)
                        met += qhit
                    pdf_light = pdf_light / F(n_l)
                    pdf = F(0.5) * pdf_cos + F(0.5) * pdf_light
                    good = ~(pdf_cos == F(0)) & (pdf > F(0))
                    if stats is not None:
                        stats["below_surface"] += int((to_light[s] & (pdf_cos == F(0))).sum())
                        stats["light_half_unmet"] += int((to_light[s] & (met == 0)).sum())
                        stats["cos_one_light"] += int((~to_light[s] & (met == 1)).sum())
                        stats["cos_many_lights"] += int((~to_light[s] & (met >= 2)).sum())
                    ok[s[~good]] = False
                    weight[s[good]] = pdf_cos[good] / pdf[good]
                    weighted[s[good]] = True
            albedo = np.where(weighted[:, None], albedo * weight[:, None], albedo)
            out[r[~ok]] = accum[r[~ok]]   # a failed scatter keeps what the path has collected
            r, new_d, hit_p, albedo = r[ok], new_d[ok], hit_p[ok], albedo[ok]
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = r
    if stats is not None:
        stats["not_followed"] += int((~followed).sum())
    return out, followed


def frame_samples(world, cam, width, height, spp, max_depth, seed, light_sampling=False, first_sample=0, stats=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    rad, ok = radiance(world, cam, width, height, max_depth, seed, gids, smp, light_sampling, stats)
    return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)


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
