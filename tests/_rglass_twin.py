"""A numpy float32 twin of the rough-glass rule and of whole samples under it — test infrastructure only.

faced() and scatter() restate rough_glass_faced and rough_glass_scatter (include/rt06.h: rt_scene_set_rough_glass) in float32 numpy, every operation rounded on its
own, over the tapes of _mfac_twin, which is imported and not edited.  radiance() is a COPY of _mfac_twin.radiance whose dielectric block consults the records; with
no glass record it is that function statement by statement, and tests/test_rough_glass_cpu.py pins that bit for bit.  quadrature() is the mathematics in float64,
sharing no code with either.
"""
import numpy as np

import _env_tree_twin as VT
import _mfac_twin as MT
import _nmap_twin as NT
import _smooth_twin as ST
import _tex_twin as XT
import _tri_twin as TT
from _env_light_twin import density_of, draw
from _env_twin import primary_rays
from _mfac_twin import (A_MIN, ABSORBED, BACKSIDE, BASE, CONSTANT, MAPPED, MAT_DIELECTRIC, MAT_IMAGE, MAT_METAL, OFF, SPECULAR, CaseTape, RandomTape, counts, fmax,
                        fmin, normalize)
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, PRIM_MOVING, cross, dot, near_zero

TRANSMITTED = 5
GLASS, GLASS_MAPPED = 4, 6
WAYS = {SPECULAR: "specular", TRANSMITTED: "transmitted", ABSORBED: "absorbed", BASE: "base"}
mfac_scatter = MT.scatter


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


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, tree=None, tex=None, mfacs=None, stats=None, walk=None):
    """_mfac_twin.radiance statement by statement, but for the dielectric block, marked §30: a hit on glass whose record is a rough-glass one runs faced() from
    the facing the block has computed; every other glass hit, and one the rule hands back, is the smooth dielectric it was.  ((n, 3) float32, followed (n,) bool)"""
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
            if len(gl):   # the dielectric of material_scatter: face, ratio — and then §30's rule where the material has a glass record, the smooth hit elsewhere
                rg, dg, ng = live[gl], d[gl], normal[gl]
                pg = o[gl] + dg * t[gl][:, None]
                behind = dot(dg, ng) > F(0)
                ng = np.where(behind[:, None], -ng, ng)
                ior = m_param[mi[gl]]
                ratio = np.where(behind, ior, F(1) / ior).astype(F)
                smooth = np.ones(len(gl), bool)
                if mfacs is not None:   # §30
                    rec = mfacs[mi[gl]]
                    has = np.nonzero(np.isin(rec["on"], (GLASS, GLASS_MAPPED)))[0]
                    if len(has):
                        rough = rec["roughness"][has].astype(F)
                        mp = rec["on"][has] == GLASS_MAPPED
                        if mp.any():
                            hm = gl[has][mp]
                            assert tex is not None   # (glass takes no normal map: on a sphere too the walk's normal is the one the kernel reads (u, v) from)
                            tuv_g = XT.hit_uv(world, tex[0], rays[hm], hit[hm], t[hm], prim[hm], normal[hm])
                            rough[mp] = rough[mp] * XT.lookup(tex[1], rec["image"][has][mp].astype(np.int64), tuv_g[:, 0], tuv_g[:, 1])[:, 1]
                        det = {}
                        new_w, g1, way = faced(ng[has], ratio[has], dg[has], rough, tape, rg[has], det)
                        goes, gone = (way == SPECULAR) | (way == TRANSMITTED), way == ABSORBED
                        smooth[has] = ~(goes | gone)
                        out[rg[has][gone]] = accum[rg[has][gone]]
                        carried.append((rg[has][goes], new_w[goes], pg[has][goes], (m_albedo[mi[gl[has]]] * g1[:, None]).astype(F)[goes]))
                        if stats is not None:
                            stats["rough_glass"] += len(has)
                            stats["rg_reflected"] += int((way == SPECULAR).sum())
                            stats["rg_transmitted"] += int((way == TRANSMITTED).sum())
                            stats["rg_absorbed"] += int(gone.sum())
                            stats["rg_base"] += int((way == BASE).sum())
                            stats["rg_total"] += int(det["total"].sum())
                            stats["rg_back"] += int(behind[has].sum())
                            stats["rg_mapped"] += int(mp.sum())
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
                free = np.nonzero(~must & smooth)[0]
                if len(free):
                    reflects[free] = prob[free] > tape.next(rg[free])
                refl = unit - (ng * dot(ng, unit)[:, None]) * F(2)
                dv = dot(ng, unit)
                kk = F(1) - (ratio * ratio) * (F(1) - dv * dv)
                refr = np.where((kk >= F(0))[:, None], unit * ratio[:, None] - ng * (ratio * dv + np.sqrt(kk))[:, None], F(0)).astype(F)
                carried.append((rg[smooth], np.where(reflects[:, None], refl, refr).astype(F)[smooth], pg[smooth], m_albedo[mi[gl]][smooth]))
                if stats is not None:
                    stats["glass"] += int(smooth.sum())
                    stats["glass_reflected"] += int(reflects[smooth].sum())
            sel = np.nonzero(go)[0]
            r = live[sel]
            if tex is not None:
                tuv = XT.hit_uv(world, tex[0], rays[sel], hit[sel], t[sel], prim[sel], normal[sel])
                tuv, walked = XT.prefer_walk_uv(tuv, walk, sel)   # §28: a mapped hit's (u, v) is the walk's, from before the map
            o, d, t, normal, mi, mt, prim_sel = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel], prim[sel]
            hit_p = o + d * t[:, None]
            if mfacs is not None and len(r):   # §29: the records' rule, before every draw of the base
                rec = mfacs[mi]
                has = np.nonzero(rec["on"] != OFF)[0]   # (the renderer admits a glass record on a dielectric alone, and those hits are not among these)
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
                    new_w, factor, way = mfac_scatter(normal[has], d[has], rough, f0, is_coat, tape, r[has])
                    spec, gone = way == SPECULAR, way == ABSORBED
                    done[has] = spec | gone
                    out[r[has][gone]] = accum[r[has][gone]]
                    carried.append((r[has][spec], new_w[spec], hit_p[has][spec], factor[spec]))
                    if stats is not None:
                        stats["recorded"] += len(has)
                        stats["coat"] += int(is_coat.sum())
                        stats["conductor"] += int((~is_coat).sum())
                        stats["mapped"] += int(mp.sum())
                        for name, count in MT.counts(way).items():
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
    _nmap_twin.frame_samples replaces it (nmaps None = no normal-map table) and the records of mfacs (None = no microfacet table), rough-glass records among them"""
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
