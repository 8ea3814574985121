"""A numpy float32 twin of the rough-glass rule and of whole samples under it — test infrastructure only.

faced() and scatter() restate rough_glass_faced and rough_glass_scatter (include/rt06.h: rt_scene_set_rough_glass) in float32 numpy, every operation rounded on its
own, over the tapes of _mfac_twin.  radiance() is _mfac_twin.radiance with the table's rough-glass records let through to the loop of tests/_path_twin.py, whose
dielectric block runs faced() on them; with no glass record it is that function, and tests/test_rough_glass_cpu.py holds that bit for bit.  quadrature() is the
mathematics in float64, sharing no code with either.
"""
import numpy as np

import _env_tree_twin as VT
import _mfac_twin as MT
import _nmap_twin as NT
import _path_twin as PT
import _tri_twin as TT
from _mfac_twin import A_MIN, ABSORBED, BASE, GLASS, GLASS_MAPPED, SPECULAR, CaseTape, fmax, fmin, normalize  # noqa: F401
from _nee_twin import F, cross, dot

TRANSMITTED = 5
WAYS = {SPECULAR: "specular", TRANSMITTED: "transmitted", ABSORBED: "absorbed", BASE: "base"}
mfac_scatter = MT.scatter   # the two rules the loop calls on a recorded hit, by these names: faced() below and this one (tests/test_surfaces_cpu.py records both)


def visible_normal(N, v, co, r, tape, rows, live):
    """steps 2 to 7 of the §29 rule up to M, for the cases `live` (the others draw nothing, and their M means nothing): (M, a)"""
    n = len(r)
    one = F(1)
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
    if len(live):
        t1[live], t2[live] = tape.in_unit2(rows[live])
    q = F(0.5) * (one + h[:, 2])
    t11 = t1 * t1
    t2 = (one - q) * np.sqrt(fmax(one - t11, F(0))) + q * t2
    nh = (T1 * t1[:, None] + T2 * t2[:, None]) + h * np.sqrt(fmax((one - t11) - t2 * t2, F(0)))[:, None]
    m = normalize(np.stack([a * nh[:, 0], a * nh[:, 1], fmax(nh[:, 2], F(0))], axis=1))   # 7
    return ((T * m[:, 0:1] + B * m[:, 1:2]) + N * m[:, 2:3]).astype(F), a


def g1(a, c):
    c2 = c * c
    return (F(2) / (F(1) + np.sqrt(F(1) + ((a * a) * fmax(F(1) - c2, F(0))) / c2))).astype(F)


def faced(n_, eta, ray_d, roughness, tape, rows=None, detail=None):
    """steps 2 to 7 of the rule, from the facing (n, eta): (direction (k, 3), weight (k,), way out (k,)).  detail (a dict): gets total, mirror, M, v, ch, F."""
    nn, d = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (n_, ray_d))
    eta, r = (np.ascontiguousarray(x, F).reshape(-1) for x in (eta, roughness))
    k_ = len(r)
    rows = np.arange(k_) if rows is None else np.asarray(rows)
    one = F(1)
    with np.errstate(all="ignore"):
        v = ((-d) / np.sqrt(dot(d, d))[:, None]).astype(F)                       # 2
        co = dot(nn, v)
        base = ~(co > F(0))
        M, a = visible_normal(nn, v, co, r, tape, rows, np.nonzero(~base)[0])    # 3
        ch = dot(v, M)
        x = one - fmin(fmax(ch, F(0)), one)                                      # 4
        r0 = (one - eta) / (one + eta)
        r0 = r0 * r0
        x2 = x * x
        Fr = r0 + (one - r0) * ((x2 * x2) * x)
        k = one - eta * eta * (one - ch * ch)                                    # 5
        total = ~base & ~(k >= F(0))
        mirror = total.copy()
        toss = np.nonzero(~base & ~total)[0]
        if len(toss):
            mirror[toss] = Fr[toss] > tape.next(rows[toss])
        wr = M * (F(2) * ch)[:, None] - v                                        # 6
        cr = dot(nn, wr)
        i = -v                                                                   # 7
        dv = dot(M, i)
        kk = one - eta * eta * (one - dv * dv)
        wt = i * eta[:, None] - M * (eta * dv + np.sqrt(kk))[:, None]
        ct = -dot(nn, wt)
        w = np.where(mirror[:, None], wr, wt).astype(F)
        ci = np.where(mirror, cr, ct).astype(F)
        G = g1(a, ci)
    way = np.where(base, BASE, np.where(~(ci > F(0)), ABSORBED, np.where(mirror, SPECULAR, TRANSMITTED))).astype(np.uint32)
    goes = (way == SPECULAR) | (way == TRANSMITTED)
    if detail is not None:
        detail.update(total=total, mirror=mirror & ~base, M=M, v=v, ch=ch, F=Fr, a=a, eta=eta)
    return np.where(goes[:, None], w, F(0)).astype(F), np.where(goes, G, F(0)).astype(F), way


def scatter(normal, ray_d, roughness, ior, tape, rows=None, detail=None):
    """the rule on n cases, numbered as rt06.h numbers it; detail also gets back"""
    N, d = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (normal, ray_d))
    ior = np.ascontiguousarray(ior, F).reshape(-1)
    with np.errstate(all="ignore"):
        back = dot(d, N) > F(0)                                                  # 1
        nn = np.where(back[:, None], -N, N).astype(F)
        eta = np.where(back, ior, F(1) / ior).astype(F)
    out = faced(nn, eta, d, roughness, tape, rows, detail)
    if detail is not None:
        detail.update(back=back)
    return out


def case(normal, ray_d, roughness, ior, tapes, detail=None):
    """rt_rough_glass_batch: (directions, weights, ways out, uniforms consumed)"""
    tape = CaseTape(tapes)
    out = scatter(normal, ray_d, roughness, ior, tape, None, detail)
    return out + (tape.draws.astype(np.uint32),)


# ---- the mathematics no kernel shares: float64, n = +z, the viewer in the xz plane ---------------------------------------------------------------------------
def quadrature(r, co, eta, n_theta=2000, n_phi=4000, chunk=250):
    """(mean weight, transmitted share) of roughness r seen at cosine co through the ratio eta, by the midpoint rule over the micro-normals m of the upper
    hemisphere, weighted by the density of the normals the viewer sees, G1(v) max(0, v.m) D(m) / co.  The integrand is even in y: half the azimuths, doubled."""
    a = max(r * r, 2.0 ** -10)

    def G1(z):
        z = np.clip(z, 1e-150, 1.0)
        return 2.0 / (1.0 + np.sqrt(1.0 + a * a * (1.0 - z * z) / (z * z)))

    vx, vz = np.sqrt(max(0.0, 1.0 - co * co)), co
    g1v = float(G1(np.array(co)))
    dt, dp = 0.5 * np.pi / n_theta, 2.0 * np.pi / n_phi
    phi = (np.arange(n_phi // 2) + 0.5) * dp
    cp, sp = np.cos(phi)[None, :], np.sin(phi)[None, :]
    r0 = ((1.0 - eta) / (1.0 + eta)) ** 2
    weight = share = 0.0
    for lo in range(0, n_theta, chunk):
        theta = ((np.arange(lo, min(lo + chunk, n_theta)) + 0.5) * dt)[:, None]
        st, ct = np.sin(theta), np.cos(theta)
        mx, my, mz = st * cp, st * sp, ct + 0.0 * cp
        dens = 2.0 * g1v * np.maximum(0.0, mx * vx + mz * vz) * (a * a / (np.pi * (mz * mz * (a * a - 1.0) + 1.0) ** 2)) / co * st * dt * dp
        c = mx * vx + mz * vz
        cc = np.clip(c, 0.0, 1.0)
        fr = r0 + (1.0 - r0) * (1.0 - cc) ** 5
        k = 1.0 - eta * eta * (1.0 - c * c)
        fr = np.where(k >= 0.0, fr, 1.0)
        zr = 2.0 * c * mz - vz                               # the mirrored direction's cosine to n
        zt = eta * vz + (np.sqrt(np.maximum(k, 0.0)) - eta * c) * mz   # minus the refracted direction's
        gr = np.where(zr > 0.0, G1(zr), 0.0)
        gt = np.where(zt > 0.0, G1(zt), 0.0)
        weight += float((dens * (fr * gr + (1.0 - fr) * gt)).sum())
        share += float((dens * (1.0 - fr) * (zt > 0.0)).sum())
    return weight, share


# ---- whole samples --------------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    st = MT.new_stats()
    st.update({name: 0 for name in ("rough_glass", "rg_reflected", "rg_transmitted", "rg_absorbed", "rg_base", "rg_total", "rg_back", "rg_mapped")})
    return st


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, tree=None, tex=None, mfacs=None, stats=None, walk=None,
             trace=TT.closest_intersection):
    """_mfac_twin.radiance whose dielectric block consults the records: a hit on glass whose record is a rough-glass one runs faced() from the facing the block
    has computed; every other glass hit, and one the rule hands back, is the smooth dielectric it was.  ((n, 3) float32, followed (n,) bool)"""
    stats = PT.counters(stats, {"misses_by_bounce": np.zeros(max_depth, np.int64), **new_stats()})
    return VT.map_radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light, tree, tex, mfacs, stats, walk, trace, True)


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, vn, uv, nmaps, mfacs, table, light=None, tree=None, first_sample=0, stats=None, info=None):
    """(height, width, spp, 3) float32 and followed (height, width, spp): every sample of every pixel, plain (light None) or in mode 48, over the walk
    _nmap_twin.walk_of chooses (nmaps None = no normal-map table) and with the records of mfacs (None = no microfacet table), rough-glass records among them"""
    trace, walk = NT.walk_of(vn, uv, nmaps, table, info)
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, sky, light, tree, NT.tex_of(uv, table), mfacs, stats, walk, trace),
                            width, height, spp, first_sample)


in_order_sums, resolve = VT.in_order_sums, VT.resolve
