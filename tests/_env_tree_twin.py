"""A numpy float32 twin of one whole sample under the map and the light tree together (mode 48) — test infrastructure only.

This module owns MapRule, the light rule of the map modes (32 and 48) as tests/_path_twin.py takes it, and its pieces: pick_half, table_point, light_density.
radiance() is that loop under it.  With `light` None it is _env_twin.radiance, with `light` = (tables, u0) and `tree` None it is _env_light_twin.radiance —
tests/test_env_tree_cpu.py holds both bit for bit — and with `tree` = table_of(world) it is mode 48: a Lambertian, checker or image-textured hit draws c, below
0.5 — and with a light in the table — c2, takes the map below 0.5 and the table otherwise, and weighs the path by sp / pdf with pdf = 0.5 sp + 0.5 (0.5 pe +
0.5 pl).  The builder, the walk, the choice and the leaf term are _light_tree_twin's own, called as they are; the map's draw and density are _env_light_twin's.

Material 7 (an image-textured Lambertian) is FOLLOWED when `tex` = (uv, table) is given — uv: the scene's table of texture coordinates or None, table:
[(image, wrap, filter), ...] as _tex_twin.lookup takes it — through _tex_twin.hit_uv and _tex_twin.lookup; it is sampled in mode 48 only.  `stats` counts what a
run exercised.
"""
import numpy as np

import _env_light_twin as LT
import _env_twin as ET
import _light_tree_twin as TR
import _path_twin as PT
import _tex_twin as XT
import _tri_twin as TT
from _env_light_twin import density_of, draw
from _light_tree_twin import QUAD, SPHERE, TRIANGLE
from _nee2_twin import world_arrays
from _nee_twin import F

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


class MapRule:
    """The light rule of the map modes for _path_twin.radiance: light = (tables, u0) alone is §24's (mode 32: a Lambertian or checker hit is sampled, and its
    light half is the map's); with tree = table_of(world) it is §26's (mode 48: an image-textured hit is sampled too, and the light half is shared by the map and
    the table)."""

    def __init__(self, world, light, tree=None):
        assert tree is None or tree.refused is None
        self.prims, self.quads, _ = world_arrays(world)
        self.light, self.tree, self.images = light, tree, tree is not None

    def pick(self, tape, r, sampled, mt, hit_p, new_d, stats):
        """The draws, in order: c and — mode 48, with a light in the table — c2 (pick_half); the map's x1, x2, a, b (draw), or §20's choice and point
        (table_point)."""
        tree, k = self.tree, len(r)
        to_light, to_env = np.zeros(k, bool), np.zeros(k, bool)   # to_env: light-half draws that go to the map
        drawn = np.full(k, -1, np.int64)                          # the light of the table a light-half draw went to
        if sampled.any():
            if tree is not None:
                had = tape.cur[r[sampled]].copy()
                tl, te = pick_half(tape, r[sampled], tree.n_l)
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
            new_d[s] = draw(self.light[0], self.light[1], four)[0]
            if stats is not None:
                stats["light_half"] += len(s)
                stats["checker_light_half"] += int((mt[s] == 3).sum())
                if tree is not None:
                    stats["map_draws"] += len(s)
        to_table = to_light & ~to_env
        if to_table.any():
            s = np.nonzero(to_table)[0]
            drawn[s], new_d[s] = table_point(tape, r[s], tree, self.prims, self.quads, hit_p[s], stats)
        return to_light, to_env, (to_table, drawn)

    def density(self, picked, s, hp, dd, len2, ln, pdf_cos, stats):
        """(the map's density of dd, or pm = 0.5 pe + 0.5 pl by §20's walk; own_lost: the silhouette rule for a drawn sphere)"""
        if self.tree is not None:
            pdf_light, own_lost = light_density(self.tree, self.light, self.prims, self.quads, hp, dd, len2, ln, picked[0][s], picked[1][s], stats)
            if stats is not None:
                stats["sphere_uncredited"] += int(own_lost.sum())
        else:
            pdf_light, own_lost = density_of(self.light[0], self.light[1], dd), np.zeros(len(s), bool)
        if stats is not None:
            stats["below_surface"] += int((pdf_cos == F(0)).sum())
        return pdf_light, own_lost


def map_radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light, tree, tex, mfacs, stats, walk, trace, glass):
    """the loop of _path_twin under the map's rule (light None: the cosine lobe alone), for this module and the surface twins above it"""
    assert tree is None or light is not None
    return PT.radiance(world, cam, width, height, max_depth, seed, gids, samples, trace, sky=sky, rule=MapRule(world, light, tree) if light is not None else None,
                       tex=tex, mfacs=mfacs, walk=walk, glass=glass, stats=stats)


def radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light=None, tree=None, tex=None, stats=None, walk=None, trace=TT.closest_intersection):
    """Radiance of sample samples[i] of pixel gids[i] with the miss colour sky(directions): ((n, 3) float32, followed (n,) bool).  light = (tables, u0) alone:
    §24's mixture at Lambertian and checker hits; with tree = table_of(world): §26's at Lambertian, checker and image hits.  walk: the dict a mapped walk
    (_nmap_twin.mapped_walk, passed as `trace`) leaves its (u, v) in (§28).  A dielectric hit is not followed."""
    stats = PT.counters(stats, {"misses_by_bounce": np.zeros(max_depth, np.int64), **new_stats()})
    return map_radiance(world, cam, width, height, max_depth, seed, gids, samples, sky, light, tree, tex, None, stats, walk, trace, False)


def frame_samples(world, cam, width, height, spp, max_depth, seed, sky, light=None, tree=None, tex=None, first_sample=0, stats=None, walk=None,
                  trace=TT.closest_intersection):
    """(height, width, spp, 3) float32: every sample of every pixel; followed (height, width, spp)"""
    return PT.frame_samples(lambda g, s: radiance(world, cam, width, height, max_depth, seed, g, s, sky, light, tree, tex, stats, walk, trace), width, height, spp,
                            first_sample)


in_order_sums, resolve = ET.in_order_sums, ET.resolve
