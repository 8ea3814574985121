"""A numpy float32 twin of one whole sample under the map and the light tree together (mode 48) — test infrastructure only.

radiance() is a COPY of _env_light_twin.radiance (the older twins stay untouched) with mode 48's lines marked §26.  With `light` None it is _env_twin.radiance,
with `light` = (tables, u0) and `tree` None it is _env_light_twin.radiance statement by statement — tests/test_env_tree_cpu.py pins both bit for bit — and with
`tree` = table_of(world) it is mode 48: a Lambertian, checker or image-textured hit draws c, below 0.5 — and with a light in the table — c2, takes the map below
0.5 and the table otherwise, and weighs the path by sp / pdf with pdf = 0.5 sp + 0.5 (0.5 pe + 0.5 pl).  The builder, the walk, the choice and the leaf term are
_light_tree_twin's own, called as they are; the map's rule and density are _env_light_twin's.

Material 7 (an image-textured Lambertian) is FOLLOWED when `tex` = (uv, table) is given — uv: the scene's table of texture coordinates or None, table:
[(image, wrap, filter), ...] as _tex_twin.lookup takes it — through _tex_twin.hit_uv and _tex_twin.lookup; it is sampled in mode 48 only.  `stats` counts what a
run exercised.
"""
import numpy as np

import _env_light_twin as LT
import _env_twin as ET
import _light_tree_twin as TR
import _tex_twin as XT
import _tri_twin as TT
from _env_light_twin import density_of, draw
from _env_twin import primary_rays
from _light_tree_twin import QUAD, SPHERE, TRIANGLE
from _nee2_twin import MAT_DIFFUSE_LIGHT, world_arrays
from _nee_twin import F, INV_PI, PRIM_MOVING, dot, near_zero

MODE = 48       # RT_LIGHT_SAMPLING_ENV_TREE
MAT_IMAGE = XT.MAT_IMAGE


class Empty:
    """the table of a world without lights: n_l = 0, which mode 48 accepts (§26)"""
    n_l, refused = 0, None


def table_of(world):
    """mode 16's permuted table, running sum and tree of the world (_light_tree_twin.tree_of), or Empty() for a world without lights"""
    prims, quads, mats = world_arrays(world)
    if len(TR.lights_of(prims, quads, mats, 4)[0]) == 0:
        return Empty()
    return TR.tree_of(world)


def pick_half(tape, rows, n_l):
    """§26's first draws of sampled hits `rows` (sample rows of the tape): c = next; c < 0.5 and n_l > 0: c2 = next, the map when c2 < 0.5, else the table;
    n_l == 0: the map, and no second draw.  (to_light, to_env) bool"""
    c = tape.next(rows)
    to_light = c < F(0.5)
    to_env = to_light.copy()
    if n_l > 0 and to_light.any():
        c2 = tape.next(rows[to_light])
        to_env[np.nonzero(to_light)[0]] = c2 < F(0.5)
    return to_light, to_env


def table_point(tape, rows, tree, prims, quads, hit_p, stats=None):
    """§20's choice and point for sampled hits `rows` (sample rows of the tape) at hit_p, as _light_tree_twin.radiance states them: x = next * A and the binary
    search (no draw when n_l == 1), then the kind's rule — a triangle's two draws folded, a parallelogram's two draws, a sphere's on-unit vector.
    (table position (k,), unnormalised direction (k, 3) float32)"""
    li = np.zeros(len(rows), np.int64)
    if tree.n_l > 1:
        li = TR.choose(tree.cdf, tape.next(rows) * tree.A)
    kind = tree.kind[li]
    new_d = np.zeros((len(rows), 3), F)
    if stats is not None:
        stats["table_draws"] += len(rows)
        stats["table_kinds"] += np.bincount(kind, minlength=3)[:3]
    sq_, ss_, st_ = np.nonzero(kind == QUAD)[0], np.nonzero(kind == SPHERE)[0], np.nonzero(kind == TRIANGLE)[0]
    if len(st_):
        la = tape.next(rows[st_])
        lb = tape.next(rows[st_])
        q = quads[tree.index[li[st_]]]
        new_d[st_] = TR._tri_point(la, lb, q["Q"].astype(F), q["u"].astype(F), q["v"].astype(F), hit_p[st_])
    if len(sq_):
        la = tape.next(rows[sq_])
        lb = tape.next(rows[sq_])
        q = quads[tree.index[li[sq_]]]
        new_d[sq_] = ((q["Q"].astype(F) + q["u"].astype(F) * la[:, None]) + q["v"].astype(F) * lb[:, None]) - hit_p[sq_]
    if len(ss_):
        u = tape.on_unit3(rows[ss_])
        sp_ = prims[tree.index[li[ss_]]]
        new_d[ss_] = (sp_["c0"].astype(F) + u * sp_["radius"].astype(F)[:, None]) - hit_p[ss_]
    return li, new_d


def light_density(tree, light, prims, quads, hit_p, dd, len2, ln, to_table=None, drawn=None, stats=None):
    """§26's pm of directions dd from hit_p: pe = the map's density of dd; n_l == 0: pm = pe; otherwise pl = §20's walk sum / A and pm = 0.5 pe + 0.5 pl.
    (pm (k,) float32, own_lost (k,) bool: a drawn sphere light (to_table, drawn) that the walk did not credit with disc > 0)"""
    pe = density_of(light[0], light[1], dd)
    own_lost = np.zeros(len(dd), bool)
    if tree.n_l == 0:
        return pe, own_lost
    credited = np.zeros(len(dd), bool)
    to_table = np.zeros(len(dd), bool) if to_table is None else to_table
    drawn = np.full(len(dd), -1, np.int64) if drawn is None else drawn

    def on_leaf(rr, j, term, met, pos):
        if tree.kind[j] == SPHERE:
            credited[rr] |= to_table[rr] & (drawn[rr] == j) & pos
        if stats is not None:
            stats["tree_leaves"] += len(rr)

    pl = TR.tree_density(tree, prims, quads, hit_p, dd, len2, ln, on_leaf) / tree.A
    own_lost = to_table & (tree.kind[np.maximum(drawn, 0)] == SPHERE) & ~credited
    return F(0.5) * pe + F(0.5) * pl, own_lost


def new_stats():
    """_env_light_twin's counters, and §26's: map_draws / table_draws: light-half draws sent to the map / to the table; second_draws: c2 draws made;
    image_sampled: image-textured hits that were sampled; image_light_half: of those, the ones that took the light half; sphere_uncredited: drawn sphere lights
    the walk did not credit; tree_leaves: leaf visits"""
    st = LT.new_stats()
    st.update({"map_draws": 0, "table_draws": 0, "second_draws": 0, "image_sampled": 0, "image_light_half": 0, "sphere_uncredited": 0, "tree_leaves": 0,
               "table_kinds": np.zeros(3, np.int64)})
    return st


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, tree=None, tex=None, stats=None, walk=None):
    """Radiance of sample samples[i] of pixel gids[i] with the miss colour sky(directions): ((n, 3) float32, followed (n,) bool).  light = (tables, u0) alone:
    §24's mixture at Lambertian and checker hits; with tree = table_of(world): §26's at Lambertian, checker and image hits.  _env_light_twin.radiance statement
    by statement, but for the blocks marked §26 — and §28: walk, the dict a substituted walk (_nmap_twin.mapped_walk) leaves its (u, v) in."""
    assert cam.type == 0, "the twin restates the pinhole camera"
    assert tree is None or (light is not None and tree.refused is None)   # §26
    gids = np.ascontiguousarray(gids, np.uint32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(gids)
    prims, quads, mats = world_arrays(world)
    mat_of_prim = np.concatenate([(prims["mat"] & ~np.uint32(PRIM_MOVING)), quads["mat"]]).astype(np.int64)
    m_type, m_albedo, m_albedo2, m_param = mats["type"].astype(np.int64), mats["albedo"].astype(F), mats["albedo2"].astype(F), mats["param"].astype(F)
    both = tree is not None                                   # §26: mode 48
    n_l = tree.n_l if both else 0                             # §26
    scatters = (0, 1, 3, MAT_IMAGE) if tex is not None else (0, 1, 3)   # §26: material 7 is followed where its images are known
    if stats is not None:
        stats.setdefault("misses_by_bounce", np.zeros(max_depth, np.int64))
        for key, zero in new_stats().items():
            stats.setdefault(key, zero)
    tape, ray_o, ray_d = primary_rays(cam, width, height, seed, gids, samples)
    rows = np.arange(n)
    from_light = np.zeros(n, bool)   # §24 (stats only): the ray being traced was drawn from the map
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
            lit = mt == MAT_DIFFUSE_LIGHT   # a light of either kind: emits, never scatters
            accum[live[lit]] = accum[live[lit]] + atten[live[lit]] * m_albedo[mi[lit]]
            out[live[lit]] = accum[live[lit]]
            other = ~miss & ~lit & ~np.isin(mt, scatters)
            followed[live[other]] = False
            out[live[other]] = np.nan
            go = np.isin(mt, scatters)
            if bounce + 1 >= max_depth:
                out[live[go]] = accum[live[go]]
                break
            sel = np.nonzero(go)[0]
            r = live[sel]
            if tex is not None:   # §26: the texture coordinates of every hit that goes on, before the arrays are cut down to them
                tuv = XT.hit_uv(world, tex[0], rays[sel], hit[sel], t[sel], prim[sel], normal[sel])
                tuv, walked = XT.prefer_walk_uv(tuv, walk, sel)   # §28: a mapped hit's (u, v) is the walk's, from before the map
            o, d, t, normal, mi, mt = o[sel], d[sel], t[sel], normal[sel], mi[sel], mt[sel]
            hit_p = o + d * t[:, None]
            k = len(r)
            lamb = mt != 1
            sampled = lamb & ((mt != MAT_IMAGE) | both)   # §26: an image hit is a diffuse hit; modes 0 and 32 leave it to the cosine lobe alone
            ok = np.ones(k, bool)
            new_d = np.zeros((k, 3), F)
            # §24: the first draw of a Lambertian / checker hit picks the half; the map's half draws x1, x2, a, b and no on-unit vector
            weight = np.ones(k, F)
            weighted = np.zeros(k, bool)
            to_light = np.zeros(k, bool)
            to_env = np.zeros(k, bool)          # §26: light-half draws that go to the map
            drawn = np.full(k, -1, np.int64)    # §26: the light of the table a light-half draw went to
            if light is not None and sampled.any():
                if both:   # §26: c, then — with a light in the table — c2
                    had = tape.cur[r[sampled]].copy()
                    tl, te = pick_half(tape, r[sampled], n_l)
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
            if to_table.any():   # §26: §20's choice and point
                s = np.nonzero(to_table)[0]
                drawn[s], new_d[s] = table_point(tape, r[s], tree, prims, quads, hit_p[s], stats)
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
            img = np.nonzero(mt == MAT_IMAGE)[0]   # §26: the albedo of an image hit, behind the direction: the table's entry at the hit's coordinates
            if len(img):
                albedo[img] = XT.lookup(tex[1], m_albedo2[mi[img]][:, 0].astype(np.int64), tuv[img, 0], tuv[img, 1])
                XT.count_walk_uv(walk, walked[img].sum())
            if light is not None:   # §24: the densities of the direction under both halves
                s = np.nonzero(sampled & ok)[0]
                if len(s):
                    dd, nn = new_d[s], normal[s]
                    len2 = dot(dd, dd)
                    ln = np.sqrt(len2)
                    cosn = dot(nn, dd) / ln
                    pdf_cos = np.where(cosn > F(0), cosn * INV_PI, F(0)).astype(F)
                    if both:   # §26: pm = 0.5 pe + 0.5 pl by §20's walk (n_l == 0: pe), and the silhouette rule for a drawn sphere
                        pdf_light, own_lost = light_density(tree, light, prims, quads, hit_p[s], dd, len2, ln, to_table[s], drawn[s], stats)
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
            from_light[r] = to_env
            r, new_d, hit_p, albedo = r[ok], new_d[ok], hit_p[ok], albedo[ok]
            atten[r] = atten[r] * albedo
            ray_d[r] = new_d
            ray_o[r] = hit_p + new_d * F(0.001)
            live = r
    return out, followed


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, light=None, tree=None, tex=None, first_sample=0, stats=None, walk=None):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    gids = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint32), width * height)
    rad, ok = radiance(world, cam, width, height, max_depth, seed, gids, smp, sky, light, tree, tex, stats, walk)
    return rad.reshape(height, width, spp, 3), ok.reshape(height, width, spp)


in_order_sums, resolve = ET.in_order_sums, ET.resolve
