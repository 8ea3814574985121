"""A numpy float32 twin of the microfacet rule and of whole samples under it — test infrastructure only.

scatter() restates microfacet_scatter of include/rt06.h (rt_scene_set_microfacet) in float32 numpy, every operation rounded on its own, over any tape that
serves next(rows) and in_unit2(rows): CaseTape (the words of rt_microfacet_batch's cases), RandomTape (fresh uniforms, for the mathematics no kernel shares) or
_nee_twin's tape of a sample.  radiance() is a COPY of _env_tree_twin.radiance (the older twins stay untouched) with §29's lines marked: the records' rule before
the scatter branches and — so that a room with a glass ball is followed on every sample — the dielectric of material_scatter.  With no records and no glass it
is _env_tree_twin.radiance statement by statement; tests/test_microfacets_cpu.py pins that bit for bit.  The oracle does not know the rule: rt_microfacet_batch —
the kernels' own function on the host — is pinned to scatter() bit for bit before anything is compared with either.
"""
import numpy as np

import _env_tree_twin as VT
import _nmap_twin as NT
import _smooth_twin as ST
import _tex_twin as XT
import _tri_twin as TT
from _env_light_twin import density_of, draw
from _env_twin import primary_rays
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, PRIM_MOVING, cross, dot, near_zero

SPECULAR, BASE, ABSORBED, BACKSIDE = 1, 2, 3, 4
WAYS = {SPECULAR: "specular", BASE: "base", ABSORBED: "absorbed", BACKSIDE: "backside"}
OFF, CONSTANT, MAPPED = 0, 1, 2
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


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, tree=None, tex=None, mfacs=None, stats=None, walk=None):
    """_env_tree_twin.radiance statement by statement, but for the blocks marked §29: mfacs = one record of capi.MICROFACET_DT per material, or None; a
    dielectric hit is followed.  ((n, 3) float32, followed (n,) bool)"""
    assert cam.type == 0, "the twin restates the pinhole camera"
    assert tree is None or (light is not None and tree.refused is None)
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)
    both = tree is not None
    n_l = tree.n_l if both else 0
    scatters = (0, 1, 3, MAT_IMAGE) if tex is not None else (0, 1, 3)
    if stats is not None:
        stats.setdefault("misses_by_bounce", np.zeros(max_depth, np.int64))
        for key, zero in new_stats().items():
            stats.setdefault(key, zero)
    tape, ray_o, ray_d = primary_rays(cam, width, height, seed, gids, samples)
    rows = np.arange(n)
    from_light = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        atten = np.ones((n, 3), F)
        accum = np.zeros((n, 3), F)
        out = np.zeros((n, 3), F)
        followed = np.ones(n, bool)
        live = rows.copy()
        for bounce in range(max_depth):
            if len(live) == 0:
                break
            k = len(live)
            rays = np.zeros((k, 7), F)
            rays[:, 0:3], rays[:, 3:6] = ray_o[live], ray_d[live]
            hit, t, prim, normal = TT.closest_intersection(world, rays)
            o, d = rays[:, 0:3], rays[:, 3:6]
            miss = hit == 0
            if stats is not None:
                stats["light_half_hit"] += int((from_light[live] & ~miss).sum())
            if miss.any():
                out[live[miss]] = atten[live[miss]] * np.asarray(sky(d[miss]), F) + accum[live[miss]]
                if stats is not None:
                    stats["misses_by_bounce"][bounce] += int(miss.sum())
            mi = mat_of_prim[np.where(miss, 0, prim)]
            mt = np.where(miss, -1, m_type[mi])
            lit = mt == MAT_DIFFUSE_LIGHT
            accum[live[lit]] = accum[live[lit]] + atten[live[lit]] * m_albedo[mi[lit]]
            out[live[lit]] = accum[live[lit]]
            glass = mt == MAT_DIELECTRIC                                     # §29: followed here
            other = ~miss & ~lit & ~glass & ~np.isin(mt, scatters)
            followed[live[other]] = False
            out[live[other]] = np.nan
            go = np.isin(mt, scatters)
            if bounce + 1 >= max_depth:
                out[live[go | glass]] = accum[live[go | glass]]
                break
            carried = []   # §29: (rows, new direction, hit point, factor) of the hits that go on without the base's scatter
            gl = np.nonzero(glass)[0]
            if len(gl):   # §29: the dielectric of material_scatter: face, ratio, Schlick, one uniform unless the reflection is total
                rg, dg, ng = live[gl], d[gl], normal[gl]
                pg = o[gl] + dg * t[gl][:, None]
                behind = dot(dg, ng) > F(0)
                ng = np.where(behind[:, None], -ng, ng)
                ior = m_param[mi[gl]]
                ratio = np.where(behind, ior, F(1) / ior).astype(F)
                unit = normalize(dg)
                cos_t = np.minimum(dot(-unit, ng), F(1))
                sin_t = np.sqrt(F(1) - cos_t * cos_t)
                r0 = (F(1) - ratio) / (F(1) + ratio)
                r0 = r0 * r0
                x1 = F(1) - cos_t
                x2 = x1 * x1
                prob = r0 + (F(1) - r0) * ((x2 * x2) * x1)
                must = ratio * sin_t > F(1)
                reflects = must.copy()
                free = np.nonzero(~must)[0]
                if len(free):
                    reflects[free] = prob[free] > tape.next(rg[free])
                refl = unit - (ng * dot(ng, unit)[:, None]) * F(2)
                dv = dot(ng, unit)
                kk = F(1) - (ratio * ratio) * (F(1) - dv * dv)
                refr = np.where((kk >= F(0))[:, None], unit * ratio[:, None] - ng * (ratio * dv + np.sqrt(kk))[:, None], F(0)).astype(F)
                carried.append((rg, np.where(reflects[:, None], refl, refr).astype(F), pg, m_albedo[mi[gl]]))
                if stats is not None:
                    stats["glass"] += len(gl)
                    stats["glass_reflected"] += int(reflects.sum())
            sel = np.nonzero(go)[0]
            r = live[sel]
            if tex is not None:
                tuv = XT.hit_uv(world, tex[0], rays[sel], hit[sel], t[sel], prim[sel], normal[sel])
                tuv, walked = XT.prefer_walk_uv(tuv, walk, sel)   # §28: a mapped hit's (u, v) is the walk's, from before the map
            o, d, t, normal, mi, mt, prim_sel = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel], prim[sel]
            hit_p = o + d * t[:, None]
            if mfacs is not None and len(r):   # §29: the records' rule, before every draw of the base
                rec = mfacs[mi]
                has = np.nonzero(rec["on"] != OFF)[0]
                done = np.zeros(len(r), bool)
                if len(has):
                    rough = rec["roughness"][has].astype(F)
                    mp = rec["on"][has] == MAPPED
                    if mp.any():
                        assert tex is not None
                        XT.count_walk_uv(walk, walked[has][mp].sum())
                        green = XT.lookup(tex[1], rec["image"][has][mp].astype(np.int64), tuv[has][mp, 0], tuv[has][mp, 1])[:, 1]
                        rough[mp] = rough[mp] * green
                    is_coat = mt[has] != MAT_METAL
                    f0 = np.where(is_coat[:, None], rec["specular"][has].astype(F)[:, None], m_albedo[mi[has]]).astype(F)
                    new_w, factor, way = scatter(normal[has], d[has], rough, f0, is_coat, tape, r[has])
                    spec, gone = way == SPECULAR, way == ABSORBED
                    done[has] = spec | gone
                    out[r[has][gone]] = accum[r[has][gone]]
                    carried.append((r[has][spec], new_w[spec], hit_p[has][spec], factor[spec]))
                    if stats is not None:
                        stats["recorded"] += len(has)
                        stats["coat"] += int(is_coat.sum())
                        stats["conductor"] += int((~is_coat).sum())
                        stats["mapped"] += int(mp.sum())
                        for name, count in counts(way).items():
                            stats[name] += count
                keep = ~done
                r, o, d, t, normal, mi, mt, hit_p = r[keep], o[keep], d[keep], t[keep], normal[keep], mi[keep], mt[keep], hit_p[keep]
                if tex is not None:
                    tuv, walked = tuv[keep], walked[keep]
            k = len(r)
            lamb = mt != 1
            sampled = lamb & ((mt != MAT_IMAGE) | both)
            ok = np.ones(k, bool)
            new_d = np.zeros((k, 3), F)
            weight = np.ones(k, F)
            weighted = np.zeros(k, bool)
            to_light = np.zeros(k, bool)
            to_env = np.zeros(k, bool)
            drawn = np.full(k, -1, np.int64)
            if light is not None and sampled.any():
                if both:
                    had = tape.cur[r[sampled]].copy()
                    tl, te = VT.pick_half(tape, r[sampled], n_l)
                    to_light[np.nonzero(sampled)[0]], to_env[np.nonzero(sampled)[0]] = tl, te
                    if stats is not None:
                        stats["second_draws"] += int((tape.cur[r[sampled]] - had == 2).sum())
                        stats["image_sampled"] += int((mt[sampled] == MAT_IMAGE).sum())
                        stats["image_light_half"] += int((to_light & (mt == MAT_IMAGE)).sum())
                else:
                    c = tape.next(r[sampled])
                    to_light[np.nonzero(sampled)[0]] = c < F(0.5)
                    to_env = to_light.copy()
            if to_env.any():
                s = np.nonzero(to_env)[0]
                four = np.stack([tape.next(r[s]) for _ in range(4)], axis=1)
                new_d[s] = draw(light[0], light[1], four)[0]
                if stats is not None:
                    stats["light_half"] += len(s)
                    stats["map_draws"] += len(s) if both else 0
                    stats["checker_light_half"] += int((mt[s] == 3).sum())
            to_table = to_light & ~to_env
            if to_table.any():
                s = np.nonzero(to_table)[0]
                drawn[s], new_d[s] = VT.table_point(tape, r[s], tree, prims, quads, hit_p[s], stats)
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
            if len(chk):
                sp = hit_p[chk] * m_param[mi[chk]][:, None]
                ssum = np.trunc(sp).astype(np.int64).sum(axis=1)
                albedo[chk] = np.where((ssum % 2 == 0)[:, None], m_albedo[mi[chk]], m_albedo2[mi[chk]])
            img = np.nonzero(mt == MAT_IMAGE)[0]
            if len(img):
                albedo[img] = XT.lookup(tex[1], m_albedo2[mi[img]][:, 0].astype(np.int64), tuv[img, 0], tuv[img, 1])
                XT.count_walk_uv(walk, walked[img].sum())
            if light is not None:
                s = np.nonzero(sampled & ok)[0]
                if len(s):
                    dd, nn = new_d[s], normal[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    if both:
                        pdf_light, own_lost = VT.light_density(tree, light, prims, quads, hit_p[s], dd, len2, ln, to_table[s], drawn[s], stats)
                        if stats is not None:
                            stats["sphere_uncredited"] += int(own_lost.sum())
                    else:
                        pdf_light, own_lost = density_of(light[0], light[1], dd), np.zeros(len(s), bool)
                    pdf = F(0.5) * pdf_cos + F(0.5) * pdf_light
                    good = ~(pdf_cos == F(0)) & (pdf > F(0)) & ~own_lost
                    if stats is not None:
                        stats["below_surface"] += int((pdf_cos == F(0)).sum())
                    ok[s[~good]] = False
                    weight[s[good]] = pdf_cos[good] / pdf[good]
                    weighted[s[good]] = True
                albedo = np.where(weighted[:, None], albedo * weight[:, None], albedo)
            out[r[~ok]] = accum[r[~ok]]
            from_light[live] = False
            from_light[r] = to_env
            carried.append((r[ok], new_d[ok], hit_p[ok], albedo[ok]))
            r = np.concatenate([c[0] for c in carried])                         # §29: the base's hits and the carried ones go on together
            new_d, hit_p, albedo = (np.concatenate([c[i] for c in carried]).astype(F) for i in (1, 2, 3))
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = np.sort(r)
    return out, followed


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, vn, uv, nmaps, mfacs, table, light=None, tree=None, first_sample=0, stats=None, info=None):
    """(height, width, spp, 3) float32 and followed (height, width, spp): every sample of every pixel, plain (light None) or in mode 48, with the walk replaced as
    _nmap_twin.frame_samples replaces it (nmaps None = no normal-map table) and the records of mfacs (None = no microfacet table)"""
    saved = TT.closest_intersection
    if nmaps is not None:
        info = {} if info is None else info   # the walk's (u, v) travel to radiance() in it
        TT.closest_intersection = lambda w, rays, preset=None: NT.mapped_walk(w, vn, uv, nmaps, table, rays, preset, info)
    elif vn is not None and len(vn):
        TT.closest_intersection = lambda w, rays, preset=None: ST.closest_intersection_smooth(w, vn, rays, preset)
    try:
        gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
        smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
        tex = (uv if uv is not None and len(uv) else None, table) if table is not None else None
        rad, ok = radiance(world, cam, width, height, max_depth, seed, gids, smp, sky, light, tree, tex, mfacs, stats, info if nmaps is not None else None)
        return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)
    finally:
        TT.closest_intersection = saved


in_order_sums, resolve = VT.in_order_sums, VT.resolve
