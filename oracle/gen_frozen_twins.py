#!/usr/bin/env python3
"""Freeze what the whole-sample numpy twins compute as the committed fixture tests/golden/frozen_twins.npz (test infrastructure).

The twins under tests/_*_twin.py are what the `-m gpu` tests hold the light-sampling, environment, normal-map, microfacet and rough-glass kernels to, and several
of them are pinned only to one another.  This file records, per accepted mode or argument shape of every module, a small frame on the module's own room: the
samples as uint32 bit patterns (the NaNs of unfollowed samples included), `followed`, and every counter the call filled.  tests/test_twin_pins_cpu.py recomputes
every case and compares for equality.  The values come from IEEE float32 + - * / sqrt and the oracle's own math routines, as frozen_*.npz do.

It calls only each module's radiance-level API (frame_samples) and the scene builders of tests/_*_worlds.py, so the same script runs on any revision that has
those.  Regenerate with `python oracle/gen_frozen_twins.py` — identical unless a twin changed, and a change must be explained in the commit that updates it.

`--full` writes nothing: it prints one sha256 line per full-size run of the worlds modules (samples, followed, sorted counters) — the frames the GPU tests
compare kernels against — to be kept under profiles/ and compared between two revisions.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import _env_light_twin as LT  # noqa: E402
import _env_light_worlds as LW  # noqa: E402
import _env_tree_twin as VT  # noqa: E402
import _env_tree_worlds as VW  # noqa: E402
import _env_twin as ET  # noqa: E402
import _env_worlds as EW  # noqa: E402
import _light_tree_twin as TR  # noqa: E402
import _light_tree_worlds as TRW  # noqa: E402
import _mesh_light_twin as ML  # noqa: E402
import _mesh_light_worlds as MLW  # noqa: E402
import _mfac_twin as MF  # noqa: E402
import _mfac_worlds as MFW  # noqa: E402
import _nee2_twin as T2  # noqa: E402
import _nee2_worlds as N2W  # noqa: E402
import _nee_twin as T  # noqa: E402
import _nee_worlds as NW  # noqa: E402
import _nmap_twin as NM  # noqa: E402
import _nmap_worlds as NMW  # noqa: E402
import _rglass_twin as RG  # noqa: E402
import _rglass_worlds as RGW  # noqa: E402
import _smooth_twin as ST  # noqa: E402
import _smooth_worlds as SMW  # noqa: E402
import _surface_worlds as SW  # noqa: E402
import _tri_twin as TT  # noqa: E402
import _tri_worlds as TW  # noqa: E402
from _common import as_oracle_camera, as_oracle_world, pkg  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "frozen_twins.npz")
W, H, SPP = 16, 12, 2
F = np.float32

# Cases whose frame is larger than W x H x SPP, because at that size one of the counters of the case's own rule (its `must`) stayed at zero: name -> (w, h, spp),
# samples raised first.
SIZES = {}


def world_of(scene):
    world = as_oracle_world(scene.getWorldPtr())
    world.scene = scene   # the arrays the world points into live as long as it does
    return world


def cam_of(camera):
    return as_oracle_camera(camera)


def room_view(p, view, w, h):
    lookfrom, lookat, vfov = view
    return cam_of(p.PinholeCamera(lookfrom, lookat, (0, 1, 0), vfov, w / h))


def sky_lights(p, scene, world, env):
    """(sky, light, tree) of a room of the surface families: its constant background, or mode 48's map and table"""
    if env:
        image, u0 = scene.environment()
        return ET.sky_environment(image, u0), (p.api.environment_distribution(image), u0), VT.table_of(world)
    colour = np.array(list(world.background_color), F)
    return (lambda d: np.broadcast_to(colour, (len(d), 3))), None, None


def cases(p):
    """{name: (fn(w, h, spp) -> (samples, followed, counters), must)} — must: the counters of the case's own rule, which a pinned frame has to reach"""
    out = {}

    # ---- the world's own sky: table modes 0 / 1 / 2 / 4 / 16 ----
    def table_family(name, module, scene, view, depth, seed, modes, must_of, flag=None):
        world = world_of(scene)
        for mode in modes:
            def fn(w, h, spp, mode=mode):
                stats = {}
                kw = {flag: bool(mode)} if flag else {"mode": mode}
                s, f = module.frame_samples(world, room_view(p, view, w, h), w, h, spp, depth, seed, stats=stats, **kw)
                return s, f, stats
            out[f"{name}/mode{mode}"] = (fn, must_of(mode))

    table_family("nee", T, NW.two_light_room(p), NW.ROOM_VIEW, 8, NW.SEED, (0, 1), lambda m: ("light_samples", "cos_one_light") if m else (), flag="light_sampling")
    sphere_must = lambda m: {0: (), 1: ("light_samples",), 2: ("sphere_light_half", "both_roots")}[m]   # noqa: E731
    table_family("nee2", T2, N2W.mixed_room(p), N2W.ROOM_VIEW, 8, N2W.SEED, (0, 1, 2), sphere_must)
    table_family("tri", TT, TW.tri_room(p, lamp=True, tri_light=True), TW.VIEW, TW.DEPTH, TW.SEED, (0, 1, 2), sphere_must)
    mesh_must = lambda m: ("tri_light_half", "tri_folded") if m == 4 else sphere_must(m)   # noqa: E731
    table_family("mesh_light", ML, MLW.three_kinds(p), TW.VIEW, MLW.DEPTH, MLW.SEED, (0, 1, 2, 4), mesh_must)
    tree_must = lambda m: ("tree_leaves", "tri_light_half", "sphere_light_half") if m == 16 else mesh_must(m)   # noqa: E731
    table_family("light_tree", TR, MLW.three_kinds(p), TW.VIEW, TRW.DEPTH, TRW.SEED, (0, 1, 2, 4, 16), tree_must)
    table_family("light_tree_mixed", TR, TRW.scene("mixed"), TW.VIEW, TRW.DEPTH, TRW.SEED, (16,), tree_must)

    # ---- the walk substituted: smooth normals under every table mode ----
    smooth = SMW.smooth_room(p, lamp=True)
    smooth_world, vn = world_of(smooth), smooth.vertex_normals()
    assert np.any(ST.table(vn) != 0)
    for mode in (0, 1, 2, 4, 16):
        def fn(w, h, spp, mode=mode):
            info = {}
            s, f = ST.frame_samples(smooth_world, vn, room_view(p, TW.VIEW, w, h), w, h, spp, SMW.DEPTH, SMW.SEED, mode=mode, info=info)
            return s, f, info
        out[f"smooth/mode{mode}"] = (fn, ("smooth", "interpolated"))

    # ---- the `sky` callable: map modes 0 / 32 / 48 ----
    sky_room = EW.sky_room(p)
    env, u0 = sky_room.environment()
    for name, sky in (("constant", ET.sky_constant(EW.C)), ("gradient", ET.sky_gradient), ("map", ET.sky_environment(env, u0))):
        def fn(w, h, spp, sky=sky):
            stats = {}
            s, f = ET.frame_samples(world_of(sky_room), cam_of(EW.camera(p, w, h)), w, h, spp, EW.DEPTH, EW.SEED, sky, stats=stats)
            return s, f, stats
        out[f"env/{name}"] = (fn, ("misses_by_bounce",))

    mesh_room = LW.sky_mesh_room(p)
    env, u0 = mesh_room.environment()
    for name, light in (("plain", None), ("light", (p.api.environment_distribution(env), u0))):
        def fn(w, h, spp, light=light, env=env, u0=u0):
            stats = {}
            s, f = LT.frame_samples(world_of(mesh_room), cam_of(EW.camera(p, w, h)), w, h, spp, LW.DEPTH, LW.SEED, ET.sky_environment(env, u0), light=light, stats=stats)
            return s, f, stats
        out[f"env_light/{name}"] = (fn, ("light_half", "light_half_hit", "checker_light_half") if light else ("misses_by_bounce",))

    lamp_room = VW.sky_lamp_room(p)   # textured: a world with two image textures
    env, u0 = lamp_room.environment()
    lamp_world = world_of(lamp_room)
    tables = p.api.environment_distribution(env)
    for name, kw in (("plain", {}), ("light", {"light": (tables, u0)}), ("light_tree", {"light": (tables, u0), "tree": VT.table_of(lamp_world)})):
        for tex_name, tex in (("", None), ("+tex", VW.tex_of(lamp_room))):
            def fn(w, h, spp, kw=kw, tex=tex, env=env, u0=u0):
                stats = {}
                s, f = VT.frame_samples(lamp_world, cam_of(VW.camera(p, "room", w, h)), w, h, spp, VW.DEPTH, VW.SEED, ET.sky_environment(env, u0), tex=tex,
                                        stats=stats, **kw)
                return s, f, stats
            must = {"plain": ("misses_by_bounce",), "light": ("light_half",), "light_tree": ("map_draws", "table_draws", "second_draws", "tree_leaves")}[name]
            out[f"env_tree/{name}{tex_name}"] = (fn, must + (("image_sampled",) if tex and name == "light_tree" else ()))

    # ---- the surface families, plain and in mode 48, with their rooms' tables ----
    def surface_family(name, module, worlds, room, variants):
        for env in (False, True):
            scene = room(p, env=env)
            world = world_of(scene)
            table = worlds.room_table()
            for variant, pick, must in variants:
                if variant and env:   # the variants without a table are pinned plain
                    continue
                def fn(w, h, spp, scene=scene, world=world, env=env, pick=pick, table=table):
                    sky, light, tree = sky_lights(p, scene, world, env)
                    counters, info = {}, {}
                    args = (world, cam_of(worlds.camera(p, w, h)), w, h, spp, worlds.DEPTH, worlds.SEED, sky) + pick(scene)
                    kw = {"stats": counters} if module is not NM else {}
                    s, f = module.frame_samples(*args, table, light=light, tree=tree, info=info, **kw)
                    counters.update({"info." + k: v for k, v in info.items()})
                    return s, f, counters
                out[f"{name}/{'mode48' if env else 'plain'}{variant}"] = (fn, must + (("table_draws",) if env and module is not NM else ()))

    tables_of = lambda s: (s.vertex_normals(), s.texture_coords(), s.normal_maps())   # noqa: E731
    surface_family("nmap", NM, NMW, NMW.room, [
        ("", tables_of, ("info.mapped", "info.replaced")),
        ("/no_maps", lambda s: tables_of(s)[:2] + (None,), ()),                       # the smooth walk
        ("/flat_walk", lambda s: (None, s.texture_coords(), None), ())])              # the flat walk
    with_records = lambda s: tables_of(s) + (s.microfacets(),)   # noqa: E731
    no_records = lambda s: tables_of(s) + (None,)   # noqa: E731
    surface_family("mfac", MF, MFW, MFW.room, [
        ("", with_records, ("recorded", "specular", "base", "mapped", "glass", "info.mapped")),
        ("/no_records", no_records, ("glass", "glass_reflected"))])                   # glass is followed
    surface_family("rglass", RG, RGW, RGW.room, [
        ("", with_records, ("recorded", "rough_glass", "rg_reflected", "rg_transmitted", "rg_back", "rg_mapped", "glass")),
        ("/no_records", no_records, ("glass", "glass_reflected"))])
    return out


def counter_items(counters):
    """the numeric entries of a stats or info dict, as arrays, sorted by name (a walk's last (u, v), a test's switches and None are not counters)"""
    for key in sorted(counters):
        v = counters[key]
        if isinstance(v, (int, np.integer, np.ndarray)) and not isinstance(v, bool):
            yield key, np.asarray(v, np.int64)


def compute_case(name, case):
    """{array name: array} of one case, as the fixture stores them"""
    fn, must = case
    w, h, spp = SIZES.get(name, (W, H, SPP))
    samples, followed, counters = fn(w, h, spp)
    counters = dict(counter_items(counters))
    zero = [k for k in must if not np.any(counters[k])]
    assert not zero, f"{name}: {zero} stayed at zero at {w} x {h} x {spp}: raise the case's size in SIZES"
    arrays = {f"{name}/bits": np.ascontiguousarray(samples, F).view(np.uint32), f"{name}/followed": np.asarray(followed, bool)}
    arrays.update({f"{name}/stats/{key}": v for key, v in counters.items()})
    return arrays


def compute():
    arrays = {}
    for name, case in cases(pkg()).items():
        arrays.update(compute_case(name, case))
    return arrays


def digest(samples, followed, counters):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(samples, F).view(np.uint32).tobytes())
    h.update(np.ascontiguousarray(followed, bool).tobytes())
    for key, v in counter_items(counters or {}):
        h.update(key.encode())
        h.update(v.tobytes())
    return h.hexdigest()


def full():
    """one line per full-size run of the worlds modules"""
    def line(name, run, counters=None, samples="samples", followed="followed"):
        f = getattr(run, followed)
        f = getattr(run, "pixel_followed") if isinstance(f, bool) else f
        print(f"{digest(getattr(run, samples), f, counters)}  {name}", flush=True)

    for name in NW.WORLDS:
        line(f"nee {name}", NW.run(name), NW.run(name).stats)
    for name in N2W.WORLDS:
        line(f"nee2 {name}", N2W.run(name), N2W.run(name).stats)
    for as_list in (False, True):
        for mode, kw in ((0, {}), (1, {}), (2, {"lamp": True}), (0, {"tri_light": True}), (0, {"textured": True}), (2, {"lamp": True, "textured": True})):
            line(f"tri list={as_list} mode={mode} {kw}", TW.run(as_list=as_list, mode=mode, **kw))
    for name in MLW.WORLDS:
        if name != "sixty_five":
            line(f"mesh_light {name}", MLW.run(name), MLW.run(name).stats)
    for name in TRW.WORLDS:
        line(f"light_tree {name}", TRW.run(name), TRW.run(name).stats)
    line("light_tree three_kinds mode=4", TRW.run("three_kinds", 4), TRW.run("three_kinds", 4).stats)
    for as_list in (False, True):
        for mode, kw in ((0, {}), (1, {}), (2, {"lamp": True}), (4, {"lamp": True}), (16, {"lamp": True}), (0, {"flat": True}), (0, {"textured": True})):
            r = SMW.run(as_list=as_list, mode=mode, **kw)
            line(f"smooth list={as_list} mode={mode} {kw}", r, r.info)
    line("env sky_room", EW.sky_room_run(), EW.sky_room_run().stats)
    for name, as_list in (("forms", False), ("forms", True), ("sun", False), ("half_black", False), ("replaced", False)):
        line(f"env_light {name} list={as_list}", LW.run(name, as_list), LW.run(name, as_list).stats)
    for name, as_list in (("forms", False), ("forms", True), ("n_l=0", False), ("n_l=1", False), ("n_l=2", False), ("n_l=65", False), ("triangle_lamp", False), ("sun", False),
                          ("replaced", False), ("silhouette", False)):
        line(f"env_tree {name} list={as_list}", VW.run(name, as_list), VW.run(name, as_list).stats)
    for env in (False, True):
        for as_list in (False, True):
            r = NMW.run(env, as_list)
            line(f"nmap env={env} list={as_list}", r, r.info)
            line(f"nmap env={env} list={as_list} unmapped", r, samples="unmapped")
            r = MFW.run(env, as_list)
            line(f"mfac env={env} list={as_list}", r, r.stats)
            line(f"mfac env={env} list={as_list} unrecorded", r, samples="unrecorded")
            r = RGW.run(env, as_list)
            line(f"rglass env={env} list={as_list}", r, r.stats)
            line(f"rglass env={env} list={as_list} clear", r, samples="clear")
            r = SW.run(env, as_list)
            line(f"surface env={env} list={as_list}", r, {**r.stats, **{"info." + k: v for k, v in r.info.items()}})
            line(f"surface env={env} list={as_list} unrecorded", r, samples="unrecorded", followed="unrecorded_followed")
        line(f"nmap env={env} flat walk", NMW.run(env, False, False), NMW.run(env, False, False).info)
        line(f"surface env={env} flat map", SW.run(env, flat=True), SW.run(env, flat=True).stats)
        line(f"surface env={env} after_map", SW.run(env, after_map=True), SW.run(env, after_map=True).stats)
    for seed in SW.SEEDS:
        r = SW.random_run(seed)
        line(f"surface random {seed} plain", r.plain, r.plain.stats)
        if r.mode48 is not None:
            line(f"surface random {seed} mode48", r.mode48, r.mode48.stats)


if __name__ == "__main__":
    if "--full" in sys.argv[1:]:
        full()
    else:
        arrays = compute()
        np.savez_compressed(OUT, **arrays)
        print(f"{OUT}: {os.path.getsize(OUT) / 1024:.0f} KB, {sum(k.endswith('/bits') for k in arrays)} cases")
