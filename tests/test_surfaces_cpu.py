"""Spheres under maps without a GPU: what tests/test_gpu_surfaces_twin.py and tests/test_gpu_surfaces_oracle.py rely on, checked on the twin
and the host alone.  The whole-sample twin follows every sample of sphere_room and of every random seed; the room, and the union of the seeds, leave every rule by
every way a frame can reach; the order the kernels have — (u, v) from the normal BEFORE the normal map, shared with the image lookup and the roughness map — is the
twin's, equals the other order where the maps are flat and differs from it where they bend; the three older rooms' frames are what they were; and the per-hit
inputs of the twin's rules, fed to the host functions the kernels share, give what the twin computed.  The counters are printed: `pytest -s` shows them."""
import numpy as np
import pytest

import _mfac_twin as MT
import _mfac_worlds as MW
import _nmap_twin as NT
import _nmap_worlds as NW
import _rglass_twin as GT
import _rglass_worlds as GW
import _surface_worlds as SW
import _tex_twin as XT
import _tri_worlds as TW
from _common import as_oracle_camera, bits_equal, mismatch_report, pkg
from _env_twin import primary_rays

F = np.float32
# what a run must have exercised: the rough-glass rule (mapped, from behind, total reflection, transmission), the microfacet rule (mapped, both kinds, every
# way out of RT_MFAC_*), and the normal-map rule on mapped hits, with the lookups that took the walk's (u, v) on a sphere
STATS = ("rg_mapped", "rg_back", "rg_total", "rg_transmitted", "mapped", "coat", "conductor", "specular", "base", "absorbed", "backside")
INFO = ("mapped", "replaced", "uv_lookups")


@pytest.fixture(scope="module")
def p():
    return pkg()


def counters(run):
    out = {k: int(run.stats[k]) for k in STATS}
    out.update({"nmap_" + k: int(run.info.get(k, 0)) for k in INFO + ("flat", "facing", "no_tangent", "no_length", "no_frame")})
    return out


# ---- 1. the twin follows, and the worlds exercise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_sphere_room_is_followed_and_takes_every_way_a_frame_can(env, as_list):
    run = SW.run(env, as_list)
    assert run.followed.all() and run.unrecorded_followed.all()
    c = counters(run)
    print(f"sphere_room {'mode 48' if env else 'plain'} {'list' if as_list else 'bvh'}: {c}")
    assert all(c[k] > 0 for k in STATS), c
    assert all(c["nmap_" + k] > 0 for k in INFO), c
    assert not bits_equal(run.samples, run.unrecorded)   # the records are in view
    assert len(run.mfacs) and int((run.mfacs["on"] != 0).sum()) == SW.SPHERE_ROOM_RECORDS


def test_the_poles_of_sphere_room_leave_the_rule_without_a_tangent(p):
    """The no-tangent way out needs dot(T, T) > 0 to fail: n.x^2 + n.z^2 must round to 0, so the hit point must have the pole's x and z to the last bit, which no
    sample of a frame does (the frames' count is 0, printed above; primary rays do meet the small sphere's cap around the pole, asserted here).  So the walk of
    this world — the same mapped_walk, tables and records — is given rays down the small sphere's axis: every one leaves by RT_NMAP_NO_TANGENT, normal unchanged."""
    run = SW.run(False)
    w, h, spp, _ = run.args
    gids = np.repeat(np.arange(w * h, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), w * h)
    _, o, d = primary_rays(as_oracle_camera(run.cam), w, h, SW.SEED, gids, smp)
    rays = np.zeros((len(o), 7), F)
    rays[:, 0:3], rays[:, 3:6] = o, d
    scene = run.scene
    walk = lambda r, info: NT.mapped_walk(run.world, scene.vertex_normals(), scene.texture_coords(), scene.normal_maps(), run.table, r, None, info)   # noqa: E731
    info = {}
    hit, _, prim, normal = walk(rays, info)
    prims = scene.arrays()[1]
    pole = int(np.nonzero((prims["radius"] == F(SW.POLE_RADIUS)))[0][0])
    on_cap = (hit != 0) & (prim == pole)
    assert on_cap.sum() > 20 and info["no_tangent"] == 0
    # the unmapped normal of those hits: the cap around the pole
    _, _, _, flat_normal = NT.mapped_walk(run.world, scene.vertex_normals(), scene.texture_coords(), np.zeros_like(scene.normal_maps()), run.table, rays[on_cap])
    assert (flat_normal[:, 1] > 0.9).sum() > 3 and flat_normal[:, 1].max() > 0.95, np.sort(flat_normal[:, 1])[-5:]
    info = {}
    axis = SW.pole_rays(16)
    hit, _, prim, normal = walk(axis, info)
    assert (hit != 0).all() and (prim == pole).all()
    assert info["mapped"] == 32 and info["no_tangent"] == 32, info
    _, _, _, unmapped = NT.mapped_walk(run.world, scene.vertex_normals(), scene.texture_coords(), np.zeros_like(scene.normal_maps()), run.table, axis)
    assert bits_equal(normal, unmapped) and not normal[:, [0, 2]].any() and (normal[:16, 1] > 0.99).all() and (normal[16:, 1] < -0.99).all()
    print(f"sphere_room pole rays: {{'mapped': {info['mapped']}, 'no_tangent': {info['no_tangent']}}}; primary hits on the cap: {int(on_cap.sum())}")


def test_every_seed_is_followed_and_their_union_takes_every_way_a_frame_can():
    total, builders, sky = {}, set(), 0
    for seed in SW.SEEDS:
        rr = SW.random_run(seed)
        builders.add(rr.recipe["builder"])
        sky += rr.env
        for run in (rr.plain, rr.mode48):
            if run is None:
                continue
            assert run.followed.all(), rr.recipe
            c = counters(run)
            assert run.stats["recorded"] + run.stats["rough_glass"] > 0, rr.recipe   # every seed has a recorded hit
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
    print(f"random surface worlds, seeds {SW.SEEDS[0]}..{SW.SEEDS[-1]} (base {SW.SEED_BASE}), {sky} under the sky: {total}")
    assert all(total[k] > 0 for k in STATS), total
    assert all(total["nmap_" + k] > 0 for k in INFO), total
    assert builders == set(SW.BUILDERS) and 2 <= sky <= 6   # every builder; about half under the sky map


def test_a_random_world_holds_at_most_24_primitives_and_one_mesh(p):
    for seed in SW.SEEDS:
        scene, table, _, recipe = SW.random_surface_world(p, seed)
        mesh = len(TW.mesh_io().uv_sphere(8, 4)[1]) if recipe["mesh"] else 0
        w = scene.getWorldPtr()
        assert w.n_prims == recipe["spheres"] and w.n_prims + w.n_quads <= 24 + mesh, recipe
        assert 2 <= len(table) <= 5 and w.traversal == 0


# ---- 2. the order ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_flat_maps_make_both_orders_one_and_bending_maps_tell_them_apart(env):
    """(u, v) before the map (the kernels', the twin's) against (u, v) after it (hit_uv of the replaced normal, the twin's `after_map` switch): with flat maps
    the normals are not bent and the two frames are one, bit for bit; with the bending maps they differ — the order is in view."""
    flat, flat_after = SW.run(env, flat=True), SW.run(env, flat=True, after_map=True)
    assert flat.info["flat"] == flat.info["mapped"] > 0 and flat.info["uv_lookups"] > 0 and flat_after.info.get("uv_lookups", 0) == 0
    assert bits_equal(flat.samples, flat_after.samples), mismatch_report(flat.samples, flat_after.samples)
    bent, bent_after = SW.run(env), SW.run(env, after_map=True)
    assert bent.followed.all() and bent_after.followed.all()
    differ = (bent.sums.view(np.uint32) != bent_after.sums.view(np.uint32)).any(axis=2)
    print(f"sphere_room {'mode 48' if env else 'plain'}: {int(differ.sum())} of {differ.size} pixels tell the two orders apart")
    assert differ.sum() > 10
    assert not bits_equal(bent.samples, flat.samples)


@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_the_three_older_rooms_are_what_they_were(env):
    """no sphere of §28's, §29's and §30's rooms has both a normal map and a lookup, so handing the walk's (u, v) on changes no bit of their frames: the twin
    with the hand-over switched off (hit_uv's coordinates, what it computed before) gives the samples the rooms' cached runs hold"""
    p = pkg()
    for run, twin, world_mod in ((NW.run(env), NT, NW), (MW.run(env), MT, MW), (GW.run(env), GT, GW)):
        s = run.scene
        sky, light, tree = GW.lights_of(p, s, run.world, env) if env else ((lambda d: np.broadcast_to(np.array(world_mod.BACKGROUND, F), (len(d), 3))), None, None)
        cam = as_oracle_camera(world_mod.camera(p))
        args = (run.world, cam, world_mod.W, world_mod.H, world_mod.SPP, world_mod.DEPTH, world_mod.SEED, sky, s.vertex_normals(), s.texture_coords(), s.normal_maps())
        if twin is NT:
            old, _ = NT.frame_samples(*args, run.table, light=light, tree=tree, info={"after_map": True})
        else:
            old, _ = twin.frame_samples(*args, s.microfacets(), run.table, light=light, tree=tree, info={"after_map": True})
        assert bits_equal(old, run.samples), (twin.__name__, mismatch_report(old, run.samples))


# ---- 3. the whole-sample twin against the host's rules, hit by hit -------------------------------------------------------------------------------------------------
class Recorder:
    """stands in for a rule function of the twin and keeps, call by call, its inputs, the words of the sample tapes it drew and its outputs"""

    def __init__(self, fn, tape_at=None):
        self.fn, self.tape_at, self.calls = fn, tape_at, []

    def __call__(self, *args, **kwargs):
        if self.tape_at is None:
            out = self.fn(*args, **kwargs)
            self.calls.append((args, out, None))
            return out
        tape, rows = args[self.tape_at], np.asarray(args[self.tape_at + 1])
        before = tape.cur[rows].copy()
        out = self.fn(*args, **kwargs)
        words = []
        for r, a, b in zip(rows, before, tape.cur[rows]):
            k = tape.u[r, a:b].astype(np.float64) * 2.0 ** 24
            assert (k == np.rint(k)).all() and (k >= 1).all() and (k <= 2 ** 24).all()   # u = k 2^-24: the words of the host batches
            words.append(k.astype(np.uint32))
        self.calls.append((args, out, words))
        return out


class WithoutTable:
    """a Recorder's calls with the table argument (the first) dropped and a single output made a tuple, so that gathered() sees per-case arrays alone"""

    def __init__(self, rec):
        self.calls = []
        for args, out, words in rec.calls:
            out = out if isinstance(out, tuple) else (out,)
            if len(out[0]):
                self.calls.append((tuple(args[1:]), out, words))


def gathered(rec, n_in, n_out, pick=256, seed=31, cover=None):
    """the first n_in inputs, the outputs and the words of `pick` of the recorded cases (all of them where there are fewer), drawn without replacement by a
    fixed generator; cover: the output (a way out) of whose every value the first case is among them"""
    ins = [np.concatenate([np.asarray(c[0][i]).reshape(len(np.asarray(c[1][0])), -1) for c in rec.calls]) for i in range(n_in)]
    outs = [np.concatenate([np.asarray(c[1][i]) for c in rec.calls]) for i in range(n_out)]
    words = sum((c[2] for c in rec.calls), []) if rec.calls[0][2] is not None else None
    n = len(outs[0])
    pick = min(pick, n)
    first = np.zeros(0, np.int64) if cover is None else np.unique(outs[cover], return_index=True)[1]
    rest = np.setdiff1d(np.arange(n), first)
    at = np.sort(np.concatenate([first, np.random.default_rng(seed).choice(rest, pick - len(first), replace=False)]))
    return [x[at].squeeze() if x.shape[1] == 1 else x[at] for x in ins], [x[at] for x in outs], (None if words is None else [words[i] for i in at]), n


def test_the_host_rules_give_what_the_twin_computed_on_256_hits_of_each_rule(p, monkeypatch):
    """The twin's run of sphere_room with its rule functions recorded; 256 of the hits of each rule (every hit of a rule with fewer) — the normal map with the (u, v) the walk handed on, the
    microfacet rule, rough glass from the facing the dielectric block left, and every texture lookup — go to rt_normal_map_batch, rt_microfacet_batch,
    rt_rough_glass_batch and rt_texture_lookup_batch, the functions the kernels share, and come back as the twin had them, bit for bit."""
    nmap, mfac, glass, look = Recorder(NT.case), Recorder(GT.mfac_scatter, 5), Recorder(GT.faced, 4), Recorder(XT.lookup)
    monkeypatch.setattr(NT, "case", nmap)
    monkeypatch.setattr(GT, "mfac_scatter", mfac)
    monkeypatch.setattr(GT, "faced", glass)
    monkeypatch.setattr(XT, "lookup", look)
    cached = SW.run(False)
    fresh = SW.Run(cached.scene, cached.table, cached.cam, *cached.args, False, unrecorded=False)
    monkeypatch.undo()
    assert bits_equal(fresh.samples, cached.samples)
    table = NW.api_table(cached.table)

    (surface, a, b, tri, normal, ray_d, u, v, index, strength), (want_n, want_path), _, n = gathered(WithoutTable(nmap), 10, 2, cover=1)
    got_n, got_path = p.api.normal_map_batch(table, surface, a, b, tri, normal, ray_d, u, v, index, strength)
    assert bits_equal(got_n, want_n) and (got_path == want_path).all(), mismatch_report(got_n, want_n)
    assert (surface == NT.SPHERE).all() and len(set(want_path.tolist())) >= 2
    print(f"host rules on sphere_room: normal map {n} hits", end="")

    (normal, ray_d, rough, f0, coat), (want_w, want_f, want_way), words, n = gathered(mfac, 5, 3, cover=2)
    got = p.api.microfacet_batch(normal, ray_d, rough, f0, coat.astype(np.uint32), words)
    assert bits_equal(got[0], want_w) and bits_equal(got[1], want_f) and (got[2] == want_way).all(), mismatch_report(got[0], want_w)
    assert (got[3] == [len(k) for k in words]).all() and set(want_way.tolist()) == set(MT.WAYS)
    print(f", microfacet {n}", end="")

    (facing, eta, ray_d, rough), (want_w, want_g, want_way), words, n = gathered(glass, 4, 3, cover=2)
    behind = eta == F(1.5)                       # the frosted ball's index: 1.5 from inside, 1 / 1.5 from outside
    assert (behind | (eta == F(1) / F(1.5))).all() and behind.any() and not behind.all()
    got = p.api.rough_glass_batch(np.where(behind[:, None], -facing, facing), ray_d, rough, np.full(len(eta), 1.5, F), words)
    assert bits_equal(got[0], want_w) and bits_equal(got[1], want_g) and (got[2] == want_way).all(), mismatch_report(got[0], want_w)
    assert (got[3] == [len(k) for k in words]).all()
    print(f", rough glass {n}", end="")

    assert n >= 100 and len(words) == min(n, 256)   # the room's frosted ball is met about a hundred times: every one of those hits
    (index, u, v), (want_c,), _, n = gathered(WithoutTable(look), 3, 1)
    got_c = p.api.texture_lookup_batch(table, index, u, v)
    assert bits_equal(got_c, want_c), mismatch_report(got_c, want_c)
    print(f", texture lookups {n}")
