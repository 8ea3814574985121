"""The numpy float32 restatement of one whole sample: the one bounce loop every whole-sample twin runs ("One loop for a whole sample") — test
infrastructure only.

radiance() restates one_sample / sample_world: the pixel jitter's rejection loop and the camera's ray — pinhole, defocus or motion — (primary_rays), then per bounce
the miss, the emitter, the classification, the dielectric, the records' rules, the mixture of the light half and the cosine lobe, the Lambertian / metal /
isotropic scatter, the checker, image and noise albedo and the write-back, every operation a float32 operation rounded on its own.  What the twins differ in arrives as an argument and never as a module
attribute: the walk (`trace`), the colour of a miss (`sky`), the light rule (`rule`: _light_tree_twin.TableRule for modes 1 / 2 / 4 / 16,
_env_tree_twin.MapRule for modes 32 / 48, None for the cosine lobe alone), the texture table (`tex`), the microfacet and rough-glass records (`mfacs`), the
dict a mapped walk leaves its (u, v) in (`walk`), whether a dielectric hit is followed (`glass`), the interior records of solid glass (`interiors`), and whether
the walk is handed the tape so that a constant medium can draw inside it, the cameras draw their lens and time, and isotropic and noise hits are followed
(`media`; DESIGN.md §33 — without it the loop is what it was, and tests/test_path_twin_oracle_cpu.py pins it to the CPU oracle with it).  The ten modules tests/_*_twin.py keep their rules, their
counters and their radiance() / frame_samples() signatures and call down to here; tests/golden/frozen_twins.npz pins the result to the ten loops this replaced.

A rule serves two places of the loop.  pick(tape, r, sampled, mt, hit_p, new_d, stats) decides which of the hits `sampled` take the light half and writes their
directions into new_d — it consumes draws of the tape, so the order of its draws is the contract — and returns (to_light, from_map, picked);
density(picked, s, hp, dd, len2, ln, pdf_cos, stats) is the light half's density of the chosen directions dd of the hits s: (pdf_light, own_lost).  `images`
says whether an image-textured hit is sampled too.

Counters: `stats` is the caller's dict, prepared by counters(); a counter that only some twins keep (count()) is counted where the dict has it.
"""
import numpy as np

from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, PRIM_MOVING, _Tape, count, dot, near_zero

MAT_METAL, MAT_DIELECTRIC, MAT_CHECKER, MAT_ISOTROPIC, MAT_NOISE = 1, 2, 3, 5, 6


def keys(width, height, spp, first_sample=0):
    """(gids, samples) of samples [first_sample, first_sample + spp) of every pixel, pixel-major"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    return gids, smp


def frame_samples(radiance, width, height, spp, first_sample=0):
    """radiance(gids, samples) on every sample of every pixel: ((height, width, spp, 3) float32, followed (height, width, spp))"""
    rad, ok = radiance(*keys(width, height, spp, first_sample))
    return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)


def counters(stats, zeros):
    """the caller's dict with the counters `zeros` names (a twin's new_stats()) where it did not have them; None stays None"""
    if stats is not None:
        for key, zero in zeros.items():
            stats.setdefault(key, zero)
    return stats


def bump(stats, key, which):
    """stats[key] += the number of True in `which`, a counter made on first use"""
    stats[key] = stats.get(key, 0) + int(np.count_nonzero(which))


def primary_rays(cam, width, height, seed, gids, samples, timed=False):
    """one_sample: pixel centre in NDC, jitter in a disc of half a pixel, then the camera's sample_ray in orc_camera_tape's draw order — PinholeCamera's draws
    nothing, DefocusBlurCamera's the lens disc, MotionBlurCamera's the time: (tape, origin (n, 3), direction (n, 3)), and with `timed` (tape, rays (n, 7)) with the
    time in rays[:, 6].  A caller that does not take the time gets the pinhole camera alone."""
    assert timed or cam.type == 0, "without the rays' times: the pinhole camera"
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
        co, cu, cv, cw = (np.array(list(v), F) for v in (cam.o, cam.u, cam.v, cam.w))
        time = np.zeros(n, F)
        if cam.type == 1:   # DefocusBlurCamera::sample_ray: the lens disc after the pixel jitter
            dx, dy = tape.in_unit2(rows)
            offset = (cu[None, :] * dx[:, None] + cv[None, :] * dy[:, None]) * F(cam.lens_radius)
            forward = cw * F(cam.focus_dist)
            hori = (cu * F(cam.viewport_width)) * F(cam.focus_dist)
            vert = (cv * F(cam.viewport_height)) * F(cam.focus_dist)
            ray_o = co[None, :] + offset
            ray_d = ((forward[None, :] + hori[None, :] * sx[:, None]) + vert[None, :] * sy[:, None]) - offset
        else:
            ray_o = np.broadcast_to(co, (n, 3)).copy()
            ray_d = (cw[None, :] + cu[None, :] * sx[:, None]) + cv[None, :] * sy[:, None]
            if cam.type == 2:   # MotionBlurCamera::sample_ray: glm::mix(t0, t1, u)
                u = tape.next(rows)
                time = F(cam.t0) * (F(1) - u) + F(cam.t1) * u
    if timed:
        rays = np.zeros((n, 7), F)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = ray_o, ray_d, time
        return tape, rays
    return tape, ray_o, ray_d


def sky_constant(color):
    c = np.array(list(color), F)
    return lambda d: np.broadcast_to(c, d.shape)


def sky_gradient(d):
    """the reference's two-colour sky (Renderer.cu:150-151)"""
    inv = F(1) / np.sqrt(dot(d, d))
    tt = (d[:, 1] * inv) * F(0.5) + F(0.5)
    a, b = np.array([0.1, 0.2, 0.4], F), np.array([0.9, 0.9, 0.99], F)
    return a[None, :] + (b - a)[None, :] * tt[:, None]


def own_sky(world):
    """the world's own background: its constant colour, or the gradient"""
    return sky_constant(world.background_color) if world.background == 1 else sky_gradient


def radiance(world, cam, width, height, max_depth, seed, gids, samples, trace, sky=None, rule=None, tex=None, mfacs=None, walk=None, glass=False, stats=None,
             media=False, interiors=None, smooth_tris=None):
    """Radiance of sample samples[i] of pixel gids[i]: ((n, 3) float32, followed (n,) bool).  trace(world, rays (k, 7)) -> (hit, t, prim, normal); sky(directions
    (k, 3)) -> (k, 3), None: the world's own; rule: see above; tex = (uv table or None, [(image, wrap, filter), ...]): material 7 is followed; mfacs: one record
    of capi.MICROFACET_DT per material; walk: the dict a mapped walk (_nmap_twin.mapped_walk) leaves its (u, v) in; glass: a dielectric hit is followed; media: the walk
    is handed the tape and the rows it serves (trace(world, rays, tape=, rows=)), so that a constant medium draws inside it, and an isotropic and a noise hit are
    followed — under any camera, the rays at their own times; interiors: one record of _interior_twin.INTERIOR_DT per material, the solid-glass rule's factor
    on a glass hit (§32): the facing from the stored normal and expf(-(sigma * dist)), `trace` being the UNWRAPPED walk; smooth_tris: per triangle, whether it
    has vertex normals (a counter's).  A sample that meets anything else is not followed: its radiance is NaN and `followed` is False.  Without `media` the
    camera is the pinhole and every ray's time is 0, as before the loop knew them."""
    import _mfac_twin as MT   # the three stand above this module: their whole-sample functions call it
    import _rglass_twin as RG
    import _tex_twin as XT
    if interiors is not None:
        import _interior_twin as IT
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    sky = own_sky(world) if sky is None else sky
    prims, quads, mats = world_arrays(world)
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)
    scatters = (0, MAT_METAL, MAT_CHECKER) + ((XT.MAT_IMAGE,) if tex is not None else ()) + ((MAT_ISOTROPIC, MAT_NOISE) if media else ())
    if media:
        tape, first = primary_rays(cam, width, height, seed, gids, samples, timed=True)
        ray_o, ray_d, ray_time = first[:, 0:3].copy(), first[:, 3:6].copy(), first[:, 6].copy()
        draws = {} if stats is None else {"medium_info": stats}   # the walk's medium counters go where the loop's go
        if stats is not None:
            stats["lens_draws"] = stats.get("lens_draws", 0) + (n if cam.type == 1 else 0)
            stats["time_draws"] = stats.get("time_draws", 0) + (n if cam.type == 2 else 0)
    else:
        tape, ray_o, ray_d = primary_rays(cam, width, height, seed, gids, samples)
        ray_time = np.zeros(n, F)
    n_prims = len(prims)
    rows = np.arange(n)
    track = stats is not None and media   # (stats only) what a path has been through: a medium's draw, a rough transmission on the ray being traced, solid glass
    drew, now_rough, in_solid = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    from_map = np.zeros(n, bool)   # (stats only) the ray being traced was drawn from the map
    with np.errstate(all="ignore"):
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
            rays[:, 0:3], rays[:, 3:6], rays[:, 6] = ray_o[live], ray_d[live], ray_time[live]
            cur0 = tape.cur[live].copy()
            hit, t, prim, normal = trace(world, rays, tape=tape, rows=live, **draws) if media else trace(world, rays)
            if track:
                drew[live] |= tape.cur[live] > cur0
                after_rough, now_rough = now_rough, np.zeros(n, bool)
            o, d = rays[:, 0:3], rays[:, 3:6]
            miss = hit == 0
            if stats is not None:
                count(stats, "light_half_hit", int((from_map[live] & ~miss).sum()))
                if media and n_prims:
                    on_moving = ~miss & (prim < n_prims) & ((prims["mat"][np.clip(prim, 0, n_prims - 1)] & np.uint32(PRIM_MOVING)) != 0)
                    stats["moving_hits"] = stats.get("moving_hits", 0) + int((on_moving & (rays[:, 6] > F(0))).sum())
                    if walk and walk.get("uv") is not None:   # the normal-map rule ran on a sphere that had moved
                        bump(stats, "mapped_moving", walk["uv"][0] & on_moving & (rays[:, 6] > F(0.25)))
            if miss.any():
                out[live[miss]] = atten[live[miss]] * np.asarray(sky(d[miss]), F) + accum[live[miss]]
                if stats is not None and "misses_by_bounce" in stats:
                    stats["misses_by_bounce"][bounce] += int(miss.sum())
            mi = mat_of_prim[np.where(miss, 0, prim)]
            mt = np.where(miss, -1, m_type[mi])
            lit = mt == MAT_DIFFUSE_LIGHT   # a light of any kind: emits, never scatters
            accum[live[lit]] = accum[live[lit]] + atten[live[lit]] * m_albedo[mi[lit]]
            out[live[lit]] = accum[live[lit]]
            go = np.isin(mt, scatters)
            through = (mt == MAT_DIELECTRIC) if glass else np.zeros(k, bool)
            other = ~miss & ~lit & ~through & ~go
            followed[live[other]] = False
            out[live[other]] = np.nan
            if bounce + 1 >= max_depth:   # the last allowed bounce: whatever it scatters into is never traced
                out[live[go | through]] = accum[live[go | through]]
                break
            carried = []   # (rows, new direction, hit point, factor) of the hits that go on without the base's scatter
            gl = np.nonzero(through)[0]
            if len(gl):   # the dielectric of material_scatter: face, ratio — and then §30's rule where the material has a glass record, the smooth hit elsewhere
                rg, dg, ng = live[gl], d[gl], normal[gl]
                pg = o[gl] + dg * t[gl][:, None]
                ior = m_param[mi[gl]]
                albedo_g = m_albedo[mi[gl]]
                if interiors is None:
                    behind = dot(dg, ng) > F(0)
                    ng = np.where(behind[:, None], -ng, ng)
                    ratio = np.where(behind, ior, F(1) / ior).astype(F)
                else:   # §32: 1, the facing of a recorded flat primitive from its stored normal, the shading normal kept; 2, a back hit pays for the segment
                    rec_in, pm = interiors[mi[gl]], prim[gl]
                    solid, flat = rec_in["on"] != IT.OFF, pm >= n_prims
                    stored = quads["normal"][np.where(flat, pm - n_prims, 0)].astype(F) if len(quads) else np.zeros((len(gl), 3), F)
                    kept = solid & flat
                    behind = np.where(kept, dot(dg, stored) > F(0), dot(dg, ng) > F(0))
                    ng = np.where((behind & ~kept)[:, None], -ng, ng)
                    ratio, T = IT.interior_hit(behind, dg, t[gl], ior, rec_in["sigma"])
                    charged = solid & behind
                    albedo_g = np.where(charged[:, None], albedo_g * T, albedo_g).astype(F)
                total_rough = np.zeros(len(gl), bool)
                frosted = np.zeros(len(gl), bool)
                smooth = np.ones(len(gl), bool)
                if mfacs is not None:   # §30
                    rec = mfacs[mi[gl]]
                    has = np.nonzero(np.isin(rec["on"], (RG.GLASS, RG.GLASS_MAPPED)))[0]
                    if len(has):
                        rough = rec["roughness"][has].astype(F)
                        mp = rec["on"][has] == RG.GLASS_MAPPED
                        if mp.any():
                            hm = gl[has][mp]
                            assert tex is not None   # (glass takes no normal map: on a sphere too the walk's normal is the one the kernel reads (u, v) from)
                            tuv_g = XT.hit_uv(world, tex[0], rays[hm], hit[hm], t[hm], prim[hm], normal[hm])
                            rough[mp] = rough[mp] * XT.lookup(tex[1], rec["image"][has][mp].astype(np.int64), tuv_g[:, 0], tuv_g[:, 1])[:, 1]
                        det = {}
                        new_w, g1, way = RG.faced(ng[has], ratio[has], dg[has], rough, tape, rg[has], det)
                        goes, gone = (way == RG.SPECULAR) | (way == RG.TRANSMITTED), way == RG.ABSORBED
                        smooth[has] = ~(goes | gone)
                        out[rg[has][gone]] = accum[rg[has][gone]]
                        total_rough[has], frosted[has] = det["total"], True
                        carried.append((rg[has][goes], new_w[goes], pg[has][goes], (albedo_g[has] * g1[:, None]).astype(F)[goes]))
                        if track:
                            now_rough[rg[has][(way == RG.TRANSMITTED) & ~behind[has]]] = True
                            bump(stats, "rule_after_medium", drew[rg[has]])
                        if stats is not None and "rough_glass" in stats:
                            stats["rough_glass"] += len(has)
                            stats["rg_reflected"] += int((way == RG.SPECULAR).sum())
                            stats["rg_transmitted"] += int((way == RG.TRANSMITTED).sum())
                            stats["rg_absorbed"] += int(gone.sum())
                            stats["rg_base"] += int((way == RG.BASE).sum())
                            stats["rg_total"] += int(det["total"].sum())
                            stats["rg_back"] += int(behind[has].sum())
                            stats["rg_mapped"] += int(mp.sum())
                unit = MT.normalize(dg)   # Schlick, one uniform unless the reflection is total
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
                carried.append((rg[smooth], np.where(reflects[:, None], refl, refr).astype(F)[smooth], pg[smooth], albedo_g[smooth]))
                if track and interiors is not None:   # a path that went through a recorded face is inside the solid until it goes through one from behind
                    crossed = np.ones(len(gl), bool)
                    crossed[smooth] = ~reflects[smooth]
                    if mfacs is not None and len(has):
                        crossed[has[~smooth[has]]] = (way == RG.TRANSMITTED)[~smooth[has]]
                    in_solid[rg[crossed & solid]] = ~behind[crossed & solid]
                if stats is not None:
                    count(stats, "glass", int(smooth.sum()))
                    count(stats, "glass_reflected", int(reflects[smooth].sum()))
                if stats is not None and interiors is not None:   # _interior_twin.new_stats()
                    first_tri = n_prims + int((quads["kind"] == 0).sum())
                    tri, quad, sph = solid & flat & (pm >= first_tri), solid & flat & (pm < first_tri), solid & ~flat
                    for name, which in (("tri", tri), ("quad", quad), ("sphere", sph)):
                        count(stats, name + "_front", int((which & ~behind).sum()))
                        count(stats, name + "_back", int((which & behind).sum()))
                    if smooth_tris is not None and len(smooth_tris):
                        count(stats, "smooth_back", int((tri & behind & smooth_tris[np.clip(pm - first_tri, 0, len(smooth_tris) - 1)]).sum()))
                    count(stats, "total_inside", int((solid & behind & ((must & smooth) | total_rough)).sum()))
                    count(stats, "charged", int(charged.sum()))
                    count(stats, "frosted_front", int((solid & frosted & ~behind).sum()))
                    count(stats, "frosted_back", int((solid & frosted & behind).sum()))
                    count(stats, "unrecorded_mesh", int((~solid & flat & (pm >= first_tri)).sum()))
            sel = np.nonzero(go)[0]
            r = live[sel]
            if tex is not None:   # the texture coordinates of every hit that goes on, before the arrays are cut down to them
                tuv = XT.hit_uv(world, tex[0], rays[sel], hit[sel], t[sel], prim[sel], normal[sel])
                tuv, walked = XT.prefer_walk_uv(tuv, walk, sel)   # §28: a mapped hit's (u, v) is the walk's, from before the map
            o, d, t, normal, mi, mt = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel]
            hit_p = o + d * t[:, None]
            if track:
                iso = mt == MAT_ISOTROPIC
                bump(stats, "medium_after_rough_transmission", iso & after_rough[r])
                bump(stats, "inside_ended_on_medium", iso & in_solid[r])
                in_solid[r[~iso]] = False
            if mfacs is not None and len(r):   # §29: the records' rule, before every draw of the base
                rec = mfacs[mi]
                has = np.nonzero(rec["on"] != MT.OFF)[0]   # (the renderer admits a glass record on a dielectric alone, and those hits are not among these)
                done = np.zeros(len(r), bool)
                if len(has):
                    rough = rec["roughness"][has].astype(F)
                    mp = rec["on"][has] == MT.MAPPED
                    if mp.any():
                        assert tex is not None
                        XT.count_walk_uv(walk, walked[has][mp].sum())
                        green = XT.lookup(tex[1], rec["image"][has][mp].astype(np.int64), tuv[has][mp, 0], tuv[has][mp, 1])[:, 1]
                        rough[mp] = rough[mp] * green
                    is_coat = mt[has] != MAT_METAL
                    f0 = np.where(is_coat[:, None], rec["specular"][has].astype(F)[:, None], m_albedo[mi[has]]).astype(F)
                    new_w, factor, way = RG.mfac_scatter(normal[has], d[has], rough, f0, is_coat, tape, r[has])
                    spec, gone = way == MT.SPECULAR, way == MT.ABSORBED
                    done[has] = spec | gone
                    out[r[has][gone]] = accum[r[has][gone]]
                    carried.append((r[has][spec], new_w[spec], hit_p[has][spec], factor[spec]))
                    if track:
                        bump(stats, "recorded_noise", mt[has] == MAT_NOISE)
                        bump(stats, "rule_after_medium", drew[r[has]])
                    if stats is not None and "recorded" in stats:
                        stats["recorded"] += len(has)
                        stats["coat"] += int(is_coat.sum())
                        stats["conductor"] += int((~is_coat).sum())
                        stats["mapped"] += int(mp.sum())
                        for name, n_way in MT.counts(way).items():
                            stats[name] += n_way
                keep = ~done
                r, o, d, t, normal, mi, mt, hit_p = r[keep], o[keep], d[keep], t[keep], normal[keep], mi[keep], mt[keep], hit_p[keep]
                if tex is not None:
                    tuv, walked = tuv[keep], walked[keep]
            k = len(r)
            lamb = (mt != MAT_METAL) & (mt != MAT_ISOTROPIC)
            ok = np.ones(k, bool)
            new_d = np.zeros((k, 3), F)
            weight = np.ones(k, F)
            weighted = np.zeros(k, bool)
            to_light = to_map = np.zeros(k, bool)
            if rule is not None:   # the first draw of a sampled hit picks the half; the light half draws its direction and no on-unit vector
                sampled = lamb & ((mt != XT.MAT_IMAGE) | rule.images) & (mt != MAT_NOISE)   # a noise and an isotropic hit draw and scatter as with sampling off
                to_light, to_map, picked = rule.pick(tape, r, sampled, mt, hit_p, new_d, stats)
            s = np.nonzero(~to_light)[0]
            if len(s):
                on_unit = tape.on_unit3(r[s])
                metal, iso = mt[s] == MAT_METAL, mt[s] == MAT_ISOTROPIC
                sl, sm, si = s[lamb[s]], s[metal], s[iso]
                new_d[sl] = normal[sl] + on_unit[lamb[s]]
                ok[sl] = ~near_zero(new_d[sl])
                new_d[si] = on_unit[iso]   # the isotropic phase function: the on-unit vector itself, always scatters
                dn = dot(normal[sm], d[sm])
                refl = d[sm] - (normal[sm] * dn[:, None]) * F(2)
                new_d[sm] = refl + on_unit[metal] * m_param[mi[sm]][:, None]
                ok[sm] = ~((dot(new_d[sm], normal[sm]) < F(0)) | near_zero(new_d[sm]))
            albedo = m_albedo[mi].copy()
            chk = np.nonzero(mt == MAT_CHECKER)[0]
            if len(chk):   # checker_texture::value: ivec3 truncation of pos * scale, parity of the sum
                sp = hit_p[chk] * m_param[mi[chk]][:, None]
                ssum = np.trunc(sp).astype(np.int64).sum(axis=1)
                albedo[chk] = np.where((ssum % 2 == 0)[:, None], m_albedo[mi[chk]], m_albedo2[mi[chk]])
            nse = np.nonzero(mt == MAT_NOISE)[0]
            if len(nse):   # the marble at the hit point, with the world's Perlin tables
                import _noise_twin as NZ
                albedo[nse] = NZ.value(NZ.tables(world), m_albedo[mi[nse]], m_param[mi[nse]], hit_p[nse])
            if stats is not None and media:
                stats["medium_scatters"] = stats.get("medium_scatters", 0) + int((mt == MAT_ISOTROPIC).sum())
                stats["noise_hits"] = stats.get("noise_hits", 0) + len(nse)
            img = np.nonzero(mt == XT.MAT_IMAGE)[0]   # the albedo of an image hit, behind the direction: the table's entry at the hit's coordinates
            if len(img):
                albedo[img] = XT.lookup(tex[1], m_albedo2[mi[img]][:, 0].astype(np.int64), tuv[img, 0], tuv[img, 1])
                XT.count_walk_uv(walk, walked[img].sum())
            if rule is not None:   # the densities of the direction under both halves
                s = np.nonzero(sampled & ok)[0]
                if len(s):
                    dd, nn = new_d[s], normal[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    pdf_light, own_lost = rule.density(picked, s, hit_p[s], dd, len2, ln, pdf_cos, stats)
                    pdf = F(0.5) * pdf_cos + F(0.5) * pdf_light
                    good = ~(pdf_cos == F(0)) & (pdf > F(0)) & ~own_lost
                    ok[s[~good]] = False
                    weight[s[good]] = pdf_cos[good] / pdf[good]
                    weighted[s[good]] = True
                albedo = np.where(weighted[:, None], albedo * weight[:, None], albedo)
            out[r[~ok]] = accum[r[~ok]]   # a failed scatter keeps what the path has collected
            from_map[live] = False
            from_map[r] = to_map
            carried.append((r[ok], new_d[ok], hit_p[ok], albedo[ok]))
            r = np.concatenate([c[0] for c in carried])   # the base's hits and the carried ones go on together
            new_d, hit_p, albedo = (np.concatenate([c[i] for c in carried]).astype(F) for i in (1, 2, 3))
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = np.sort(r)
    if stats is not None:
        count(stats, "not_followed", int((~followed).sum()))
    return out, followed
