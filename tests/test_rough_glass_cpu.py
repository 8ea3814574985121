"""Rough glass without a GPU: the host function the kernels share against the numpy twin, bit for bit, with every way out of the rule taken;
Snell's law and the mirror law in float64 on its outputs; mathematics no kernel code shares — the mean weight and the transmitted share by float64 quadrature
over the visible normals; the whole-sample twin on the room, and its identity with §29's twin while the glass records are off; the launch image; the host
surface with its refusals, old and new."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _mfac_twin as MT
import _rglass_twin as GT
import _rglass_worlds as GW
from _common import ROOT, bits_equal, mismatch_report, pkg

F = np.float32


@pytest.fixture(scope="module")
def p():
    pk = pkg()
    from ray_tracing_v06_amd import image_io, mesh_io  # noqa: F401  (now attributes of the package)
    return pk


def same(got, want):
    for g, w, name in zip(got, want, ("direction", "weight", "way", "draws")):
        if g.dtype == np.uint32:
            assert (g == w).all(), (name, np.nonzero(g != w)[0][:5])
        else:
            assert bits_equal(g, w), (name, mismatch_report(g, w))


def twin_cases(cases, detail=None):
    return GW.run_cases(lambda *a: GT.case(*a, detail=detail), cases)


# ---- 1. the twin ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_function_is_the_twin_bit_for_bit(p):
    cases = GW.random_cases()
    detail = {}
    got, want = GW.run_cases(p.api.rough_glass_batch, cases), twin_cases(cases, detail)
    same(got, want)
    direction, weight, way, draws = got
    c = {name: int((way == code).sum()) for code, name in GT.WAYS.items()}
    assert c["specular"] > 500 and c["transmitted"] > 1000 and c["absorbed"] > 50, c
    assert detail["back"].sum() > 1000 and (~detail["back"]).sum() > 1000 and detail["total"].sum() > 300
    goes = (way == GT.SPECULAR) | (way == GT.TRANSMITTED)
    assert not direction[~goes].any() and not weight[~goes].any()          # no direction and no factor but a reflected or transmitted case's
    assert (weight[goes] > 0).all() and (weight <= 1).all()
    assert (draws[way != GT.BASE] >= 2).all() and len(set(draws.tolist())) > 4   # the number of uniforms varies


def test_the_aimed_cases_take_every_way_out_of_the_rule(p):
    cases, expected, totals = GW.aimed_cases()
    detail = {}
    got, want = GW.run_cases(p.api.rough_glass_batch, cases), twin_cases(cases, detail)
    same(got, want)
    direction, weight, way, draws = got
    for name, e, w in zip(GW.AIMED, expected, way):
        assert e == 0 or e == w, (name, GT.WAYS[int(w)])
    assert set(way.tolist()) == set(GT.WAYS)                                # specular, transmitted, absorbed, base
    at = GW.AIMED.index
    assert np.isfinite(direction).all() and np.isfinite(weight).all()
    for name in totals:                                                     # a total reflection draws the disc's two uniforms and no toss
        assert detail["total"][at(name)] and way[at(name)] == GT.SPECULAR and draws[at(name)] == 2
    assert draws[at("edge on")] == 0                                        # the smooth dielectric's draws are its own
    assert draws[at("reflected at normal incidence")] == 3 and draws[at("an empty tape")] == 3
    assert way[at("toss at F exactly goes through")] == GT.TRANSMITTED     # F > u, not >=
    back = detail["back"]
    assert back[at("back face, transmitted")] and back[at("back face, reflected")] and not back[at("N = -z")]
    absorbed = way == GT.ABSORBED                                           # either absorbed way: below the surface after the mirror, above it after the refraction
    assert (absorbed & detail["mirror"]).any() and (absorbed & ~detail["mirror"]).any() and (absorbed & back).any() and (absorbed & ~back).any()
    straight = at("transmitted at normal incidence")
    assert direction[straight, 2] < -0.99 and direction[at("reflected at normal incidence"), 2] > 0.99
    one = at("index 1")                                                     # no interface: eta = 1, F = 0 — the ray goes straight through whatever the micro-normal
    v = -cases["ray_d"][one].astype(np.float64) / np.linalg.norm(cases["ray_d"][one].astype(np.float64))
    assert way[one] == GT.TRANSMITTED and np.abs(direction[one] + v).max() < 1e-6


# ---- 2. Snell's law and the mirror law ---------------------------------------------------------------------------------------------------------------------------
def test_snell_and_mirror_laws_in_float64(p):
    """On the outputs of the host batch, with M, v and eta as the twin (bit-equal to it) holds them.  Transmitted: cross(w, M) = eta cross(-v, M), |w| = 1; reflected:
    w + v is parallel to M.  The bound counts the fp32 roundings on the way from (v, M, eta) to w: ch is a 3-term dot (5 roundings), k takes 5 more, sqrt, the
    product and sum of the bracket 3, then each component one product with eta, one with the bracket and one difference — under 20 roundings, each of relative size
    2^-24 on quantities whose magnitude is at most eta + (eta + 1) <= 2 * 2.4 + 1 = 5.8 for the indices the cases use; v and M are unit to a few ulp themselves, which
    |w| = 1 inherits (v: 6 roundings, M: ~30 through the frame and two normalisations, entering |w|^2 twice).  20 * 5.8 * 2^-24 + 2 * 36 * 2^-24 < 200 * 2^-24."""
    cases = GW.random_cases()
    detail = {}
    direction, weight, way, _ = GW.run_cases(p.api.rough_glass_batch, cases)
    same((direction, weight, way), twin_cases(cases, detail)[:3])
    bound = 200 * 2.0 ** -24
    w, M, v, eta = direction.astype(np.float64), detail["M"].astype(np.float64), detail["v"].astype(np.float64), detail["eta"].astype(np.float64)
    t = way == GT.TRANSMITTED
    assert t.sum() > 1000
    snell = np.abs(np.cross(w[t], M[t]) - eta[t][:, None] * np.cross(-v[t], M[t])).max()
    length = np.abs(np.linalg.norm(w[t], axis=1) - 1.0).max()
    s = way == GT.SPECULAR
    mirror = np.abs(np.cross(w[s] + v[s], M[s])).max()
    print(f"snell {snell:.3e} |w|-1 {length:.3e} mirror {mirror:.3e} bound {bound:.3e}")
    assert snell <= bound and length <= bound and mirror <= bound


# ---- 3. mathematics no kernel shares ---------------------------------------------------------------------------------------------------------------------------
ROUGHNESSES, COSINES, DRAWS, IOR = (0.2, 0.5, 1.0), (0.05, 0.3, 0.7, 1.0), 1 << 20, 1.5
TRIPLES = [(r, co, back) for back in (False, True) for r in ROUGHNESSES for co in COSINES]
IDS = [f"r{r}-co{co}-{'back' if back else 'front'}" for r, co, back in TRIPLES]


@functools.lru_cache(maxsize=None)
def uniforms():
    """2^20 tapes of 24 words: the disc's rejection loop needs more than eleven pairs once in 2^24 cases, and the tape's own accepting word serves it then"""
    return np.random.default_rng(30).integers(1, 2 ** 24 + 1, (DRAWS, 24), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def sampled(r, co, back):
    """(mean weight with 0 where absorbed, transmitted share, largest weight) over 2^20 draws of the host batch; n = +z on the viewer's side"""
    v = np.array([np.sqrt(max(0.0, 1.0 - co * co)), 0.0, co])
    normal = np.array([0, 0, -1 if back else 1], F)
    _, weight, way, _ = pkg().api.rough_glass_batch(np.tile(normal, (DRAWS, 1)), np.tile((-v).astype(F), (DRAWS, 1)), np.full(DRAWS, r, F), np.full(DRAWS, IOR, F), uniforms())
    assert (way != GT.BASE).all()
    return float(weight.astype(np.float64).mean()), float((way == GT.TRANSMITTED).mean()), float(weight.max())


@functools.lru_cache(maxsize=None)
def integrals(r, co, back):
    """((mean weight, transmitted share) on the 2000 x 4000 grid, the same on the half-resolution grid)"""
    eta = IOR if back else 1.0 / IOR
    return GT.quadrature(r, co, eta, 2000, 4000), GT.quadrature(r, co, eta, 1000, 2000)


TOLERANCE = 5 * 0.5 / np.sqrt(DRAWS)   # both averaged quantities lie in [0, 1]: sigma <= 0.5, five standard errors of the mean = 2.44e-3


@pytest.mark.parametrize("r,co,back", TRIPLES, ids=IDS)
def test_mean_weight_and_transmitted_share(r, co, back):
    """the mean of the weight (0 where absorbed) over the rule's own draws is the integral of F G1(w_r) + (1 - F) G1(w_t) over the visible normals, and the share of
    transmitted draws the integral of 1 - F where the refracted ray leaves on the far side"""
    fine, coarse = integrals(r, co, back)
    mean, share, largest = sampled(r, co, back)
    print(f"r={r} co={co} back={back}: weight sampled {mean:.6f} quadrature {fine[0]:.6f} (half grid {coarse[0]:.6f}) delta {abs(mean - fine[0]):.2e}; "
          f"share sampled {share:.6f} quadrature {fine[1]:.6f} (half grid {coarse[1]:.6f}) delta {abs(share - fine[1]):.2e}")
    assert abs(mean - fine[0]) <= TOLERANCE + abs(fine[0] - coarse[0])
    assert abs(share - fine[1]) <= TOLERANCE + abs(fine[1] - coarse[1])
    assert largest <= 1.0


# ---- 4. whole samples -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_the_room_takes_every_way_and_follows_every_sample(env):
    run = GW.run(env)
    st = run.stats
    assert run.followed.all()
    for key in ("rg_reflected", "rg_transmitted", "rg_absorbed", "rg_total", "rg_back", "rg_mapped"):
        assert st[key] > 0, (key, st)
    assert st["rough_glass"] > 200 and st["glass"] > 10 and st["recorded"] > 500, st   # the clear ball and §29's records are still met
    assert not bits_equal(run.samples, run.clear)


@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_with_the_glass_records_off_the_twin_is_the_microfacet_twin(env):
    """the same room through _mfac_twin, which knows no rough glass: with the glass records off, and with a table that never had them"""
    run = GW.run(env)
    for mfacs in (run.mfacs_clear, GW.room(pkg(), env=env, glass_records=False).microfacets()):
        assert mfacs.tobytes() == run.mfacs_clear.tobytes()
        got, followed = MT.frame_samples(*run.args, mfacs, run.table, **run.lights)
        assert followed.all() and bits_equal(got, run.clear), mismatch_report(got, run.clear)
        again, _ = GT.frame_samples(*run.args, mfacs, run.table, **run.lights)
        assert bits_equal(again, run.clear)


# ---- 5. the launch image --------------------------------------------------------------------------------------------------------------------------------------
def test_a_table_with_glass_records_is_laid_out_like_any_other(tmp_path):
    """rt_launch_image.hpp's append_tail compiled into a small host program: records of kinds 4 and 6 are sixteen bytes like the others, last in the tail"""
    src = tmp_path / "tail.cpp"
    src.write_text(r'''
#include "rt_launch_image.hpp"
#include <cstdio>
struct Tex { uint32_t width, height, wrap, filter, first; };
int main() {
    using namespace rt_image;
    const Tex tex[1] = {{5, 3, 0, 0, 0}};
    const uint32_t mf[3][4] = {{4, 0, 0x3e800000u, 0}, {6, 0, 0x3f000000u, 0}, {1, 0, 0x3f000000u, 0x3d23d70au}};
    for (int with_mf = 0; with_mf < 2; with_mf++) {
        Riders<Tex> r;
        r.textures = true; r.texture = tex; r.n_textures = 1; r.texture_texels = 0x0102030405060708ull;
        if (with_mf) { r.microfacets = mf; r.n_microfacets = 3; }
        std::vector<Vec4> out;
        append_tail(out, r);
        std::printf("%d:", with_mf);
        for (const Vec4& v : out) std::printf(" %x %x %x %x", v.x, v.y, v.z, v.w);
        std::printf("\n");
    }
    return 0;
}
''')
    exe = tmp_path / "tail"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc"), "-o", str(exe), str(src)])
    off, on = (line.split(":")[1].split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert len(on) == len(off) + 3 * 4 and on[1:len(off)] == off[1:]
    assert int(on[0], 16) >> 1 == len(off) // 4 and int(off[0], 16) == 0
    assert on[len(off):] == ["4", "0", "3e800000", "0", "6", "0", "3f000000", "0", "1", "0", "3f000000", "3d23d70a"]


# ---- 6. the host surface --------------------------------------------------------------------------------------------------------------------------------------
def _scene(p):
    import _tex_worlds as XW
    s = p.Scene()
    mats = dict(lam=s.Lambertian((0.5, 0.5, 0.5)), metal=s.Metal((0.8, 0.8, 0.8), 0.2), glass=s.Dielectric((1, 1, 1), 1.5), water=s.Dielectric((1, 1, 1), 1.33),
                light=s.DiffuseLight((4, 4, 4)), fog=s.Isotropic((1, 1, 1), 0.5))
    s.set_image(XW.image(5, 3))
    rough = s.add_image(XW.image(8, 4, seed=2), "repeat", "bilinear")
    for k, x in enumerate(mats.values()):
        s.MakeSphere((2.0 * k, 0, 0), 0.7, x)
    return s, mats, rough


def test_scene_calls_and_refusals(p):
    s, mats, rough = _scene(p)
    assert s.microfacets() is None
    s.set_rough_glass(mats["glass"], 0.25)
    table = s.microfacets()
    assert len(table) == len(mats) and tuple(table[mats["glass"]]) == (p.capi.MICROFACET_GLASS, 0, F(0.25), F(0.0)) and (table["on"] != 0).sum() == 1
    s.set_microfacet(mats["lam"], 0.5, 0.3)
    before = s.microfacets().tobytes()
    for bad, why in ((lambda: s.set_rough_glass(mats["lam"], 0.5), "no dielectric"), (lambda: s.set_rough_glass(mats["metal"], 0.5), "no dielectric"),
                     (lambda: s.set_rough_glass(mats["light"], 0.5), "no dielectric"), (lambda: s.set_rough_glass(mats["fog"], 0.5), "no dielectric"),
                     (lambda: s.set_rough_glass(99, 0.5), "no material 99"), (lambda: s.set_rough_glass(mats["glass"], -0.5), "roughness"),
                     (lambda: s.set_rough_glass(mats["glass"], 1.5), "roughness"), (lambda: s.set_rough_glass(mats["glass"], float("nan")), "roughness"),
                     (lambda: s.set_rough_glass(mats["glass"], float("inf")), "roughness"),
                     (lambda: s.set_microfacet(mats["glass"], 0.5), "dielectric"),                    # §29's refusals, in §29's words
                     (lambda: s.set_microfacet(mats["water"], 0.5), "dielectric"),
                     (lambda: s.set_roughness_map(mats["water"], rough), "no microfacet record"),
                     (lambda: s.set_roughness_map(mats["glass"], 256), "image index")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            bad()
        assert e.value.code == 1   # RT_ERR_INVALID
        assert s.microfacets().tobytes() == before   # and the scene is unchanged
    s.set_roughness_map(mats["glass"], rough)                    # kind 4 becomes kind 6, and brings the texture table
    assert tuple(s.microfacets()[mats["glass"]]) == (p.capi.MICROFACET_GLASS_MAPPED, rough, F(0.25), F(0.0))
    s.set_roughness_map(mats["lam"], rough)                      # ... as kind 1 becomes kind 2, still
    assert s.microfacets()[mats["lam"]]["on"] == p.capi.MICROFACET_MAPPED
    s.set_rough_glass(mats["glass"], 0.75)                       # a new roughness keeps the map
    assert tuple(s.microfacets()[mats["glass"]]) == (p.capi.MICROFACET_GLASS_MAPPED, rough, F(0.75), F(0.0))
    s.clear_microfacet(mats["lam"])
    s.BuildBVH_SAH()
    w = s.getWorldPtr()
    assert w.microfacets.tobytes() == s.microfacets().tobytes() and len(w.textures[0]) == 2   # a mapped glass record alone brings the texture table too
    s.clear_microfacet(mats["glass"])
    assert s.microfacets() is None
    s.set_rough_glass(mats["water"], 0.0)                        # roughness 0 is no special case
    s.set_rough_glass(mats["glass"], 1.0)
    assert (s.microfacets()["on"] == p.capi.MICROFACET_GLASS).sum() == 2


def test_batch_refusals(p):
    cases, _, _ = GW.aimed_cases()
    n = len(cases["roughness"])
    for change, why in ((dict(roughness=np.full(n, -0.5, F)), "roughness"), (dict(roughness=np.full(n, 1.5, F)), "roughness"), (dict(roughness=np.full(n, np.nan, F)), "roughness")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            GW.run_cases(p.api.rough_glass_batch, dict(cases, **change))
        assert e.value.code == 1
    with pytest.raises(ValueError, match="one entry per case"):
        GW.run_cases(p.api.rough_glass_batch, dict(cases, ior=cases["ior"][:-1]))
    L = p.lib()
    raw = L.rt_rough_glass_batch
    saved = raw.argtypes
    raw.argtypes = [C.c_size_t] + [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 5   # (null arguments cannot pass the array types the mirror declares)
    try:
        assert raw(1, None, None, None, None, None, 0, None, None, None, None, None) != 0 and b"null argument" in L.rt_last_error()
        one = np.zeros(4, np.uint32)
        off = np.array([3, 4], np.uint32)                         # a tape range outside the tape
        f3, f1 = np.ones(3, F), np.full(1, 0.5, F)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert raw(1, ptr(f3), ptr(f3), ptr(f1), ptr(f1), ptr(one), 4, ptr(off), ptr(f3.copy()), ptr(f1.copy()), ptr(one.copy()), ptr(one.copy())) != 0
    finally:
        raw.argtypes = saved
    a = GW.random_cases(64)                                       # the two forms of the tapes argument are one
    width = max(len(t) for t in a["tapes"])
    square = np.full((64, width), MT.PAST_END, np.uint32)
    for i, t in enumerate(a["tapes"]):
        square[i, :len(t)] = t
    listed = GW.run_cases(p.api.rough_glass_batch, dict(a, tapes=list(square)))
    same(GW.run_cases(p.api.rough_glass_batch, dict(a, tapes=square)), listed)


MTL = """newmtl frosted
Kd 1 1 1
Ni 1.45
d 0.2
illum 7
Pr 0.4
map_Pr frost.png
newmtl film
Tr 0.75
newmtl chalk
Kd 0.8 0.8 0.8
Pr 0.5
"""


def test_load_mtl_reads_the_glass_keywords(p, tmp_path):
    (tmp_path / "m.mtl").write_text(MTL)
    mats = p.mesh_io.load_mtl(str(tmp_path / "m.mtl"))
    fr = mats["frosted"]
    assert (fr["ior"], fr["dissolve"], fr["illum"], fr["roughness"], fr["roughness_map"]) == (1.45, 0.2, 7, 0.4, os.path.join(str(tmp_path), "frost.png"))
    assert mats["film"]["dissolve"] == 0.25 and "ior" not in mats["film"] and "illum" not in mats["film"]      # Tr = 1 - d
    assert not {"ior", "dissolve", "illum"} & set(mats["chalk"]) and mats["chalk"]["roughness"] == 0.5         # a file without the keywords: the entry it was
    for text, why in (("newmtl x\nNi 0\n", "Ni must be"), ("newmtl x\nd 1.5\n", "d must be"), ("newmtl x\nTr -1\n", "Tr must be"), ("newmtl x\nillum x\n", "illum"),
                      ("Ni 1.5\n", "before any newmtl")):
        (tmp_path / "bad.mtl").write_text(text)
        with pytest.raises(ValueError, match=why):
            p.mesh_io.load_mtl(str(tmp_path / "bad.mtl"))


def test_both_languages_mirror_the_surface(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("rt_scene_set_rough_glass", "rt_rough_glass_batch", "rt_probe_rough_glass"):
        assert name in header and name in p.capi.SYMBOLS and hasattr(p.lib(), name)
    assert "RT_MICROFACET_GLASS = 4" in header and "RT_MICROFACET_GLASS_MAPPED = 6" in header and "RT_MFAC_TRANSMITTED = 5" in header
    assert "SetRoughGlass(" in hpp and hasattr(p.Scene, "set_rough_glass") and hasattr(p.api, "rough_glass_batch") and hasattr(p.api, "probe_rough_glass")
    assert (p.capi.MICROFACET_GLASS, p.capi.MICROFACET_GLASS_MAPPED, p.capi.MFAC_TRANSMITTED) == (GT.GLASS, GT.GLASS_MAPPED, GT.TRANSMITTED) == (4, 6, 5)
    assert p.capi.MICROFACET_DT.itemsize == 16
    L = p.lib()
    assert L.rt_scene_set_rough_glass(None, 0, 0.5) != 0 and b"rt_scene_set_rough_glass" in L.rt_last_error()
