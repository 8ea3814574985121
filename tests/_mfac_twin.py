"""A numpy float32 twin of the microfacet rule and of whole samples under it — test infrastructure only.

scatter() restates microfacet_scatter of include/rt06.h (rt_scene_set_microfacet) in float32 numpy, every operation rounded on its own, over any tape that
serves next(rows) and in_unit2(rows): CaseTape (the words of rt_microfacet_batch's cases), RandomTape (fresh uniforms, for the mathematics no kernel shares) or
_nee_twin's tape of a sample.  radiance() is the loop of tests/_path_twin.py under _env_tree_twin's rule with the records given to it — the loop runs scatter()
before the scatter branches — and with the dielectric of material_scatter followed, so that a room with a glass ball is followed on every sample.  With no
records and no glass it is _env_tree_twin.radiance; tests/test_microfacets_cpu.py holds that bit for bit.  The oracle does not know the rule:
rt_microfacet_batch — the kernels' own function on the host — is pinned to scatter() bit for bit before anything is compared with either.
"""
import numpy as np

import _env_tree_twin as VT
import _nmap_twin as NT
import _path_twin as PT
import _tex_twin as XT
import _tri_twin as TT
from _nee_twin import F, cross, dot

SPECULAR, BASE, ABSORBED, BACKSIDE = 1, 2, 3, 4
WAYS = {SPECULAR: "specular", BASE: "base", ABSORBED: "absorbed", BACKSIDE: "backside"}
OFF, CONSTANT, MAPPED = 0, 1, 2
GLASS, GLASS_MAPPED = 4, 6   # §30's records, which _rglass_twin follows
MAT_METAL, MAT_DIELECTRIC, MAT_IMAGE = 1, 2, XT.MAT_IMAGE
A_MIN = F(2.0 ** -10)
PAST_END = 0x800001   # what a tape serves past its end: every rejection loop accepts it


def fmax(x, c):
    """x > c ? x : c, so a NaN takes c"""
    return np.where(x > c, x, c).astype(F)


def fmin(x, c):
    return np.where(x < c, x, c).astype(F)


def normalize(a):
    inv = F(1) / np.sqrt(dot(a, a))
    return (a * inv[:, None]).astype(F)


class CaseTape:
    """tapes[i] = the words k in [1, 2^24] of case i: u = k 2^-24, and k = 2^23 + 1 past the end; draws[i] counts"""

    def __init__(self, tapes):
        self.tapes = [np.asarray(t, np.uint32) for t in tapes]
        width = max([len(t) for t in self.tapes] + [1])
        self.k = np.full((len(self.tapes), width), PAST_END, np.uint32)
        for i, t in enumerate(self.tapes):
            self.k[i, : len(t)] = t
        self.draws = np.zeros(len(self.tapes), np.int64)

    def next(self, rows):
        at = self.draws[rows]
        k = np.where(at < self.k.shape[1], self.k[rows, np.minimum(at, self.k.shape[1] - 1)], PAST_END)
        self.draws[rows] += 1
        return (k.astype(F) * F(2.0 ** -24)).astype(F)

    def in_unit2(self, rows):
        ox, oy = np.zeros(len(rows), F), np.zeros(len(rows), F)
        todo = np.arange(len(rows))
        while len(todo):
            x = self.next(rows[todo]) * F(2) - F(1)
            y = self.next(rows[todo]) * F(2) - F(1)
            ok = (x * x + y * y) < F(1)
            ox[todo[ok]], oy[todo[ok]] = x[ok], y[ok]
            todo = todo[~ok]
        return ox, oy


class RandomTape(CaseTape):
    """fresh uniforms k 2^-24, k uniform in [1, 2^24], from numpy's generator: the generator's own stream is not what the mathematics is about"""

    def __init__(self, n, seed):
        self.rng = np.random.default_rng(seed)
        self.draws = np.zeros(n, np.int64)

    def next(self, rows):
        self.draws[rows] += 1
        return (self.rng.integers(1, 2 ** 24 + 1, len(rows)).astype(F) * F(2.0 ** -24)).astype(F)


def scatter(normal, ray_d, roughness, f0, coat, tape, rows=None, detail=None):
    """the rule on n cases, numbered as rt06.h numbers it: (direction (n, 3), weight (n, 3), way out (n,)); f0 (n, 3), of which a coat reads the first component;
    rows: the tape's rows of the cases (default 0 .. n - 1).  detail (a dict): gets m (the microfacet normal in the frame of N), G and F of every case."""
    N, d, F0 = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (normal, ray_d, f0))
    r = np.ascontiguousarray(roughness, F).reshape(-1)
    coat = np.asarray(coat).reshape(-1) != 0
    n = len(r)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    F0 = np.where(coat[:, None], F0[:, 0:1], F0).astype(F)
    one = F(1)
    with np.errstate(all="ignore"):
        v = (-d) / np.sqrt(dot(d, d))[:, None]                                   # 1
        co = dot(N, v)
        back = ~(co > F(0))
        a = fmax(r * r, A_MIN)                                                   # 2
        s = np.where(N[:, 2] >= F(0), one, -one).astype(F)                       # 3
        k = -one / (s + N[:, 2])
        b = (N[:, 0] * N[:, 1]) * k
        sx = s * N[:, 0]
        T = np.stack([one + (sx * N[:, 0]) * k, s * b, -sx], axis=1)
        B = np.stack([b, s + (N[:, 1] * N[:, 1]) * k, -N[:, 1]], axis=1)
        h = normalize(np.stack([a * dot(T, v), a * dot(B, v), co], axis=1))      # 4
        l2 = h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]                               # 5
        sq = np.sqrt(l2)
        T1 = np.where((l2 > F(0))[:, None], np.stack([-h[:, 1] / sq, h[:, 0] / sq, np.zeros(n, F)], axis=1), np.array([1, 0, 0], F)).astype(F)
        T2 = cross(h, T1)
        t1, t2 = np.zeros(n, F), np.zeros(n, F)                                  # 6
        live = np.nonzero(~back)[0]
        if len(live):
            t1[live], t2[live] = tape.in_unit2(rows[live])
        q = F(0.5) * (one + h[:, 2])
        t11 = t1 * t1
        t2 = (one - q) * np.sqrt(fmax(one - t11, F(0))) + q * t2
        nh = (T1 * t1[:, None] + T2 * t2[:, None]) + h * np.sqrt(fmax((one - t11) - t2 * t2, F(0)))[:, None]
        m = normalize(np.stack([a * nh[:, 0], a * nh[:, 1], fmax(nh[:, 2], F(0))], axis=1))   # 7
        M = (T * m[:, 0:1] + B * m[:, 1:2]) + N * m[:, 2:3]
        ch = dot(v, M)
        x = one - fmin(fmax(ch, F(0)), one)
        k5 = ((x * x) * (x * x)) * x
        Fr = F0 + (one - F0) * k5[:, None]                                       # 8
        base = np.zeros(n, bool)
        toss = np.nonzero(~back & coat)[0]
        if len(toss):
            base[toss] = ~(tape.next(rows[toss]) < Fr[toss, 0])
        w = M * (F(2) * ch)[:, None] - v                                         # 9
        ci = dot(N, w)
        absorbed = ~back & ~base & ~(ci > F(0))
        ci2 = ci * ci
        G = F(2) / (one + np.sqrt(one + ((a * a) * fmax(one - ci2, F(0))) / ci2))
        weight = np.where(coat[:, None], G[:, None], Fr * G[:, None]).astype(F)
    way = np.where(back, BACKSIDE, np.where(base, BASE, np.where(absorbed, ABSORBED, SPECULAR))).astype(np.uint32)
    spec = (way == SPECULAR)[:, None]
    if detail is not None:
        detail.update(m=m, G=G, F=Fr, a=a)
    return np.where(spec, w, F(0)).astype(F), np.where(spec, weight, F(0)).astype(F), way


def counts(way):
    """{name: how many cases left the rule that way}"""
    return {name: int((np.asarray(way) == code).sum()) for code, name in WAYS.items()}


def case(normal, ray_d, roughness, f0, coat, tapes):
    """rt_microfacet_batch: (directions, weights, ways out, uniforms consumed)"""
    tape = CaseTape(tapes)
    out = scatter(normal, ray_d, roughness, f0, coat, tape)
    return out + (tape.draws.astype(np.uint32),)


# ---- the mathematics no kernel shares: GGX in float64, N = +z ---------------------------------------------------------------------------------------------------
def ggx_d(mz, a):
    return a * a / (np.pi * (mz * mz * (a * a - 1.0) + 1.0) ** 2)


def ggx_g1(z, a):
    """Smith's masking of a direction with cosine z > 0"""
    z = np.clip(z, 1e-300, 1.0)
    return 2.0 / (1.0 + np.sqrt(1.0 + a * a * (1.0 - z * z) / (z * z)))


def quadrature(r, co, n_theta=2000, n_phi=4000, chunk=250):
    """(furnace, mean cosine) of roughness r seen at cosine co, by the midpoint rule on an n_theta x n_phi grid of the upper hemisphere:
    furnace = the integral of D G1(o) G1(i) / (4 co) over the directions i, mean cosine = the integral of D_vis (m.N) over the normals m,
    D_vis = G1(o) max(0, v.m) D / co."""
    a = max(r * r, 2.0 ** -10)
    v = np.array([np.sqrt(max(0.0, 1.0 - co * co)), 0.0, co])
    g1o = float(ggx_g1(np.array(co), a))
    dt, dp = 0.5 * np.pi / n_theta, 2.0 * np.pi / n_phi
    phi = (np.arange(n_phi) + 0.5) * dp
    cp, sp = np.cos(phi)[None, :], np.sin(phi)[None, :]
    furnace = cosine = 0.0
    for lo in range(0, n_theta, chunk):
        theta = ((np.arange(lo, min(lo + chunk, n_theta)) + 0.5) * dt)[:, None]
        st, ct = np.sin(theta), np.cos(theta)
        x, y, z = st * cp, st * sp, ct + 0.0 * cp
        dw = st * dt * dp
        # the grid as directions i: the half vector, its D, both maskings
        hx, hy, hz = x + v[0], y + v[1], z + v[2]
        hz = hz / np.sqrt(hx * hx + hy * hy + hz * hz)
        furnace += float((ggx_d(hz, a) * g1o * ggx_g1(z, a) / (4.0 * co) * dw).sum())
        # the grid as normals m
        vm = np.maximum(0.0, x * v[0] + y * v[1] + z * v[2])
        cosine += float((g1o * vm * ggx_d(z, a) / co * z * dw).sum())
    return furnace, cosine


# ---- whole samples ----------------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    st = VT.new_stats()
    st.update({name: 0 for name in WAYS.values()})
    st.update({"recorded": 0, "conductor": 0, "coat": 0, "mapped": 0, "glass": 0, "glass_reflected": 0})
    return st


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, tree=None, tex=None, mfacs=None, stats=None, walk=None,
             trace=TT.closest_intersection):
    """_env_tree_twin.radiance with §29's records — mfacs = one record of capi.MICROFACET_DT per material, or None — and with every dielectric hit followed, so
    that a room with a glass ball is followed on every sample.  This twin knows no rough glass: a table with such records is _rglass_twin's.
    ((n, 3) float32, followed (n,) bool)"""
    assert mfacs is None or not np.isin(mfacs["on"], (GLASS, GLASS_MAPPED)).any(), "rough-glass records: _rglass_twin.radiance"
    stats = PT.counters(stats, {"misses_by_bounce": np.zeros(max_depth, np.int64), **new_stats()})
    return VT.map_radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light, tree, tex, mfacs, stats, walk, trace, True)


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, vn, uv, nmaps, mfacs, table, light=None, tree=None, first_sample=0, stats=None, info=None):
    """(height, width, spp, 3) float32 and followed (height, width, spp): every sample of every pixel, plain (light None) or in mode 48, over the walk
    _nmap_twin.walk_of chooses (nmaps None = no normal-map table) and with the records of mfacs (None = no microfacet table)"""
    trace, walk = NT.walk_of(vn, uv, nmaps, table, info)
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, sky, light, tree, NT.tex_of(uv, table), mfacs, stats, walk, trace),
                            width, height, spp, first_sample)


in_order_sums, resolve = VT.in_order_sums, VT.resolve
