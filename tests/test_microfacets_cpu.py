"""Microfacet surfaces without a GPU: the host function the kernels share against the numpy twin, bit for bit, with every way out of the rule
taken; mathematics no kernel code shares — the furnace integral and the mean cosine of the visible normals, by float64 quadrature; the identity of a table of
records that are all off; the kernel forms and the launch image; the host surface with its refusals."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _mfac_twin as MT
import _mfac_worlds as MW
import _nmap_worlds as NW
import _kernel_table as KT
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


# ---- 1. the twin ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_function_is_the_twin_bit_for_bit(p):
    cases = MW.random_cases()
    got, want = MW.run_cases(p.api.microfacet_batch, cases), MW.run_cases(MT.case, cases)
    same(got, want)
    c = MT.counts(got[2])
    assert c["specular"] > 500 and c["base"] > 300 and c["absorbed"] > 20 and c["backside"] > 1000, c
    direction, weight, way, draws = got
    spec = way == MT.SPECULAR
    assert not direction[~spec].any() and not weight[~spec].any()          # no direction and no factor but a specular case's
    assert (draws[way == MT.BACKSIDE] == 0).all() and (draws[spec & (cases["coat"] == 0)] >= 2).all() and (draws[spec & (cases["coat"] != 0)] >= 3).all()
    assert len(set(draws.tolist())) > 4                                     # the number of uniforms varies
    coat = spec & (cases["coat"] != 0)
    assert (weight[coat, 0] == weight[coat, 1]).all() and (weight[coat, 0] == weight[coat, 2]).all()


def test_the_aimed_cases_take_every_way_out_of_the_rule(p):
    cases, expected = MW.aimed_cases()
    got, want = MW.run_cases(p.api.microfacet_batch, cases), MW.run_cases(MT.case, cases)
    same(got, want)
    way = got[2]
    for name, e, w in zip(MW.AIMED, expected, way):
        assert e == 0 or e == w, (name, MT.WAYS[int(w)])
    assert set(way.tolist()) == set(MT.WAYS)                                # specular, base, absorbed, backside
    at = MW.AIMED.index
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    straight = at("normal incidence, l2 == 0")                              # T1 = (1, 0, 0): the frame of the disk needs no length
    assert way[straight] == MT.SPECULAR and got[0][straight, 2] > 0.5
    assert got[3][at("an empty tape")] == 3                                 # the tape's accepting word, twice, and the toss


# ---- 2. mathematics no kernel shares ------------------------------------------------------------------------------------------------------------------------------
ROUGHNESSES, COSINES, DRAWS = (0.2, 0.5, 1.0), (0.05, 0.3, 0.7, 1.0), 1 << 20
PAIRS = [(r, co) for r in ROUGHNESSES for co in COSINES]


@functools.lru_cache(maxsize=None)
def sampled(r, co):
    """(mean of G with 0 where absorbed, mean of m.z, largest weight with F0 = 1) over 2^20 draws of the twin's rule, N = +z"""
    n = DRAWS
    v = np.array([np.sqrt(max(0.0, 1.0 - co * co)), 0.0, co])
    detail = {}
    _, weight, way = MT.scatter(np.tile(np.array([0, 0, 1], F), (n, 1)), np.tile((-v).astype(F), (n, 1)), np.full(n, r, F), np.ones((n, 3), F), np.zeros(n),
                                MT.RandomTape(n, seed=int(1000 * r + 100 * co)), detail=detail)
    assert (way != MT.BACKSIDE).all() and (way != MT.BASE).all()
    g = np.where(way == MT.SPECULAR, detail["G"].astype(np.float64), 0.0)
    return float(g.mean()), float(detail["m"][:, 2].astype(np.float64).mean()), float(weight.max())


@functools.lru_cache(maxsize=None)
def integrals(r, co):
    """((furnace, mean cosine) on the 2000 x 4000 grid, the same on the half-resolution grid)"""
    return MT.quadrature(r, co, 2000, 4000), MT.quadrature(r, co, 1000, 2000)


TOLERANCE = 5 * 0.5 / np.sqrt(DRAWS)   # both averaged quantities lie in [0, 1]: sigma <= 0.5, five standard errors of the mean = 2.44e-3


@pytest.mark.parametrize("r,co", PAIRS)
def test_furnace(r, co):
    """the mean of G (0 where absorbed) over the rule's own draws is the integral of D G1(o) G1(i) / (4 co) over the directions"""
    fine, coarse = integrals(r, co)
    mean = sampled(r, co)[0]
    print(f"furnace r={r} co={co}: sampled {mean:.6f} quadrature {fine[0]:.6f} (half grid {coarse[0]:.6f}) delta {abs(mean - fine[0]):.2e}")
    assert abs(mean - fine[0]) <= TOLERANCE + abs(fine[0] - coarse[0])


@pytest.mark.parametrize("r,co", PAIRS)
def test_mean_cosine_of_the_visible_normals(r, co):
    """the mean of m.z is the integral of D_vis (m.N) over the normals, D_vis = G1(o) max(0, v.m) D / co"""
    fine, coarse = integrals(r, co)
    mean = sampled(r, co)[1]
    print(f"mean cosine r={r} co={co}: sampled {mean:.6f} quadrature {fine[1]:.6f} (half grid {coarse[1]:.6f}) delta {abs(mean - fine[1]):.2e}")
    assert abs(mean - fine[1]) <= TOLERANCE + abs(fine[1] - coarse[1])


@pytest.mark.parametrize("r,co", PAIRS)
def test_no_weight_exceeds_one_with_f0_one(r, co):
    assert sampled(r, co)[2] <= 1.0


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_a_table_of_records_that_are_all_off_is_no_table(p, env):
    """§28's room through this twin with a table whose records are all off, and with none: the samples _env_tree_twin's radiance gives through _nmap_twin"""
    run = NW.run(env)
    s = run.scene
    cam = MW.as_oracle_camera(NW.camera(p))
    if env:
        image, u0 = s.environment()
        sky, light, tree = MW.ET.sky_environment(image, u0), (p.api.environment_distribution(image), u0), MW.VT.table_of(run.world)
    else:
        colour = np.array(NW.BACKGROUND, F)
        sky, light, tree = (lambda d: np.broadcast_to(colour, (len(d), 3))), None, None
    off = np.zeros(len(s.arrays()[2]), p.capi.MICROFACET_DT)
    args = (run.world, cam, NW.W, NW.H, NW.SPP, NW.DEPTH, NW.SEED, sky, s.vertex_normals(), s.texture_coords(), s.normal_maps())
    for mfacs in (off, None):
        got, followed = MT.frame_samples(*args, mfacs, run.table, light=light, tree=tree)
        assert followed.all() and bits_equal(got, run.samples), mismatch_report(got, run.samples)


def test_the_room_takes_every_way_out_and_follows_every_sample():
    for env in (False, True):
        run = MW.run(env)
        st = run.stats
        assert run.followed.all()
        assert st["specular"] > 300 and st["base"] > 300 and st["absorbed"] > 0 and st["backside"] > 100, st
        assert st["conductor"] > 100 and st["coat"] > 500 and st["mapped"] > 50 and st["glass"] > 20, st
        assert not bits_equal(run.samples, run.unrecorded)


# ---- 4. the kernel forms and the launch image -----------------------------------------------------------------------------------------------------------------------
def test_form_list_is_the_set_of_instantiations_and_the_older_counts_stand():
    """every form of stream_kernel_for()'s MICROFACET and MICROFACET_ENV_TREE families has a recipe in the list the GPU tests run, and nothing else has"""
    import _tri_worlds as TW
    for family in ("MICROFACET", "MICROFACET_ENV_TREE"):
        shipped = KT.family(family)
        assert len(shipped) == KT.count(family) == 8 and shipped == set(MW.FORMS) == set(NW.FORMS), shipped ^ set(MW.FORMS)
    assert all(MW.FORMS[f] == TW.FORMS[f] for f in MW.FORMS)
    for family, count in (("NEE", 16), ("TRI", 16), ("TRI_NEE", 16), ("LIGHT_TREE", 16), ("ENV_LIGHT", 8), ("ENV_TREE", 8), ("NORMAL_MAP", 8), ("NORMAL_MAP_ENV_TREE", 8)):
        assert KT.count(family) == count, family   # nothing existing moved
    kernel = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_stream_kernel.hpp")).read()
    assert "static_assert(!MFAC || NMAP" in kernel and "bool MFAC = false, bool NMAP = false>" in kernel


def test_the_tail_is_what_it_was_without_a_table_and_says_where_the_records_are_with_one(tmp_path):
    """rt_launch_image.hpp's append_tail, compiled into a small host program, with and without a texture table (and its normal maps): with no microfacet table the
    bytes are those of a tail composed without the new fields ever set; with one, the records come last and the bits above bit 0 of the header's first lane are
    the number of vec4 from the header to them"""
    src = tmp_path / "tail.cpp"
    src.write_text(r'''
#include "rt_launch_image.hpp"
#include <cstdio>
struct Tex { uint32_t width, height, wrap, filter, first; };
int main() {
    using namespace rt_image;
    const float vn[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9}, uv[6] = {0, 0, 1, 0, 0, 1};
    const Tex tex[3] = {{5, 3, 0, 0, 0}, {8, 4, 1, 1, 15}, {2, 2, 0, 1, 47}};
    const uint32_t nm[2][4] = {{1, 2, 0x3f000000u, 0}, {0, 0, 0, 0}};
    const uint32_t mf[2][4] = {{2, 1, 0x3e800000u, 0x3d23d70au}, {1, 0, 0x3f000000u, 0}};
    for (int with_vn = 0; with_vn < 2; with_vn++)
        for (int with_tex = 0; with_tex < 2; with_tex++)
            for (int with_mf = 0; with_mf < 2; with_mf++) {
                Riders<Tex> r;
                if (with_vn) { r.normals = vn; r.n_normal_floats = 9; r.coords = uv; r.n_coord_floats = 6; }
                r.env = true; r.env_w = 16; r.env_h = 8; r.env_u0 = 0.25f; r.env_texels = 0x1122334455667788ull;
                if (with_tex) { r.textures = true; r.texture = tex; r.n_textures = 3; r.texture_texels = 0x0102030405060708ull; r.normal_maps = nm; r.n_normal_maps = 2; }
                if (with_mf) { r.microfacets = mf; r.n_microfacets = 2; }
                std::vector<Vec4> out(2, Vec4{7, 7, 7, 7});
                append_tail(out, r);
                std::printf("%d %d %d %zu:", with_vn, with_tex, with_mf, out.size());
                for (const Vec4& v : out) std::printf(" %x %x %x %x", v.x, v.y, v.z, v.w);
                std::printf("\n");
            }
    Riders<Tex> none;   // nothing but the records: one header, then they
    none.microfacets = mf; none.n_microfacets = 2;
    std::vector<Vec4> out;
    append_tail(out, none);
    std::printf("9 9 9 %zu:", out.size());
    for (const Vec4& v : out) std::printf(" %x %x %x %x", v.x, v.y, v.z, v.w);
    std::printf("\n");
    return 0;
}
''')
    exe = tmp_path / "tail"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    words = {tuple(int(x) for x in line.split(":")[0].split()[:3]): line.split(":")[1].split() for line in lines}
    records = ["2", "1", "3e800000", "3d23d70a", "1", "0", "3f000000", "0"]
    for with_vn in (0, 1):
        for with_tex in (0, 1):
            off, on = words[(with_vn, with_tex, 0)], words[(with_vn, with_tex, 1)]
            assert len(on) == len(off) + 2 * 4
            header = 2 * 4                                      # behind the two vec4 the vector held
            assert int(off[header], 16) == with_vn              # today's first lane: normals follow, or not
            at = int(on[header], 16)
            assert at & 1 == with_vn and at >> 1 == len(off) // 4 - 2   # bit 0 as it was; above it, the vec4 from the header to the records: the old tail's length
            assert on[:header] == off[:header] and on[header + 1:len(off)] == off[header + 1:]   # nothing else moved
            assert on[len(off):] == records
    assert words[(9, 9, 9)] == ["2", "0", "0", "0"] + records
    # the bytes without a table are the bytes the committed layout check holds: tests/cpp_launch_image builds and runs untouched
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_launch_image")])
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp_launch_image", "launch_image_check")])


# ---- 5. the host surface ------------------------------------------------------------------------------------------------------------------------------------------
def _scene(p):
    import _tex_worlds as XW
    s = p.Scene()
    mats = dict(lam=s.Lambertian((0.5, 0.5, 0.5)), metal=s.Metal((0.8, 0.8, 0.8), 0.2), glass=s.Dielectric((1, 1, 1), 1.5), checker=s.LambertianTexture((0, 0, 0), (1, 1, 1), 2.0),
                light=s.DiffuseLight((4, 4, 4)), fog=s.Isotropic((1, 1, 1), 0.5), image=None, noise=None)
    s.set_perlin(3)
    mats["noise"] = s.NoiseTexture(2.0)
    s.set_image(XW.image(5, 3))
    mats["image"] = s.ImageTexture(0)
    rough = s.add_image(XW.image(8, 4, seed=2), "repeat", "bilinear")
    for k, x in enumerate(mats.values()):
        s.MakeSphere((2.0 * k, 0, 0), 0.7, x)
    return s, mats, rough


def test_scene_adders_refusals_and_builders(p):
    s, mats, rough = _scene(p)
    assert s.microfacets() is None   # NULL, 0 while no material has a record
    takers = ("lam", "metal", "checker", "noise", "image")
    for name in takers:
        s.set_microfacet(mats[name], 0.125 * (1 + mats[name]), 0.5)
    s.set_microfacet(mats["lam"], 0.25)                         # the mirrors default the specular to 0.04
    table = s.microfacets()
    assert table.dtype == p.capi.MICROFACET_DT and table.dtype.itemsize == 16 and len(table) == len(mats)
    for name, m in mats.items():
        assert table[m]["on"] == (1 if name in takers else 0)
    assert tuple(table[mats["lam"]]) == (1, 0, F(0.25), F(0.04)) and tuple(table[mats["metal"]]) == (1, 0, F(0.125 * (1 + mats["metal"])), F(0.5))
    before = table.tobytes()
    for bad, why in ((lambda: s.set_microfacet(mats["glass"], 0.5), "dielectric"), (lambda: s.set_microfacet(mats["light"], 0.5), "light"),
                     (lambda: s.set_microfacet(mats["fog"], 0.5), "medium"), (lambda: s.set_microfacet(99, 0.5), "no material 99"),
                     (lambda: s.set_microfacet(mats["lam"], -0.5), "roughness"), (lambda: s.set_microfacet(mats["lam"], 1.5), "roughness"),
                     (lambda: s.set_microfacet(mats["lam"], float("nan")), "roughness"), (lambda: s.set_microfacet(mats["lam"], 0.5, 1.5), "specular"),
                     (lambda: s.set_microfacet(mats["lam"], 0.5, float("inf")), "specular"), (lambda: s.set_microfacet(mats["lam"], 0.5, -0.1), "specular"),
                     (lambda: s.set_roughness_map(mats["glass"], rough), "no microfacet record"), (lambda: s.set_roughness_map(mats["lam"], 256), "image index"),
                     (lambda: s.set_roughness_map(99, rough), "no material 99"), (lambda: s.clear_microfacet(99), "no material 99")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            bad()
        assert e.value.code == 1   # RT_ERR_INVALID
        assert s.microfacets().tobytes() == before   # and the scene is unchanged
    for build in (s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList):   # materials are never permuted: the table is the same under each
        build()
        assert s.microfacets().tobytes() == before
        w = s.getWorldPtr()
        assert w.microfacets.tobytes() == before and not hasattr(w, "normal_maps")   # ... travels beside the flat world, and brings no other table with it
    s.set_roughness_map(mats["image"], rough)
    assert tuple(s.microfacets()[mats["image"]])[:2] == (2, rough) and len(s.getWorldPtr().textures[0]) == 2   # a mapped record brings the texture table
    s.set_microfacet(mats["image"], 1.0, 0.1)                   # new values keep the map
    assert tuple(s.microfacets()[mats["image"]]) == (2, rough, F(1.0), F(0.1))
    for name in ("lam", "metal", "checker", "noise"):
        s.clear_microfacet(mats[name])
    assert (s.microfacets()["on"] != 0).sum() == 1
    s.clear_microfacet(mats["image"])
    assert s.microfacets() is None and not hasattr(s.getWorldPtr(), "microfacets")


def test_batch_refusals(p):
    cases, _ = MW.aimed_cases()
    n = len(cases["roughness"])
    for change, why in ((dict(roughness=np.full(n, -0.5, F)), "roughness"), (dict(roughness=np.full(n, 1.5, F)), "roughness"), (dict(roughness=np.full(n, np.nan, F)), "roughness")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            MW.run_cases(p.api.microfacet_batch, dict(cases, **change))
        assert e.value.code == 1
    with pytest.raises(ValueError, match="one entry per case"):
        MW.run_cases(p.api.microfacet_batch, dict(cases, coat=cases["coat"][:-1]))
    L = p.lib()
    raw = L.rt_microfacet_batch
    saved = raw.argtypes
    raw.argtypes = [C.c_size_t] + [C.c_void_p] * 6 + [C.c_size_t] + [C.c_void_p] * 5   # (null arguments cannot pass the array types the mirror declares)
    try:
        assert raw(1, None, None, None, None, None, None, 0, None, None, None, None, None) != 0 and b"null argument" in L.rt_last_error()
    finally:
        raw.argtypes = saved


MTL = """newmtl brass
Kd 0.9 0.7 0.4
Pm 1.0
Pr 0.35
newmtl lacquer
Kd 0.7 0.1 0.1
map_Kd lacquer.png
Pr 0.2
map_Pr -s 2 2 sub/lacquer_r.png   # a comment
norm lacquer_n.png
newmtl chalk
Kd 0.8 0.8 0.8
"""


def test_load_mtl_reads_the_roughness_and_metallic_keywords(p, tmp_path):
    (tmp_path / "m.mtl").write_text(MTL)
    mats = p.mesh_io.load_mtl(str(tmp_path / "m.mtl"))
    at = lambda *names: os.path.join(str(tmp_path), *names)   # noqa: E731
    assert (mats["brass"]["roughness"], mats["brass"]["roughness_map"], mats["brass"]["metallic"], mats["brass"]["Kd"]) == (0.35, None, 1.0, (0.9, 0.7, 0.4))
    assert (mats["lacquer"]["roughness"], mats["lacquer"]["roughness_map"], mats["lacquer"]["metallic"]) == (0.2, at("sub", "lacquer_r.png"), None)
    assert (mats["lacquer"]["map_Kd"], mats["lacquer"]["normal_map"], mats["lacquer"]["normal_strength"]) == (at("lacquer.png"), at("lacquer_n.png"), 1.0)   # the older keys stay
    assert (mats["chalk"]["roughness"], mats["chalk"]["roughness_map"], mats["chalk"]["metallic"], mats["chalk"]["normal_map"]) == (None, None, None, None)
    for text, why in (("newmtl x\nPr 1.5\n", "Pr must be"), ("newmtl x\nPm -1\n", "Pm must be"), ("Pr 0.5\n", "before any newmtl"), ("newmtl x\nmap_Pr\n", "needs a file name")):
        (tmp_path / "bad.mtl").write_text(text)
        with pytest.raises(ValueError, match=why):
            p.mesh_io.load_mtl(str(tmp_path / "bad.mtl"))


def test_both_languages_mirror_the_surface(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("rt_scene_set_microfacet", "rt_scene_set_roughness_map", "rt_scene_clear_microfacet", "rt_scene_microfacets", "rt_microfacet_batch", "rt_probe_microfacet",
                 "rt_renderer_microfacets", "rt_renderer_microfacets_info", "rt_renderer_kernel_microfacet", "rt_multi_renderer_microfacets", "rt_multi_renderer_microfacets_info"):
        assert name in header and name in p.capi.SYMBOLS and hasattr(p.lib(), name)
    for name in ("SetMicrofacet(", "SetRoughnessMap(", "ClearMicrofacet(", "Microfacets(", "SetMicrofacets("):
        assert name in hpp
    for name in ("set_microfacet", "set_roughness_map", "clear_microfacet", "microfacets"):
        assert hasattr(p.Scene, name)
    for name in ("microfacets", "microfacets_info", "kernel_microfacet"):
        assert hasattr(p.Renderer, name)
    assert hasattr(p.MultiRenderer, "microfacets") and hasattr(p.MultiRenderer, "microfacets_info")
    L, out = p.lib(), (C.c_uint32 * 2)()
    assert L.rt_renderer_microfacets(None, None, 0) != 0 and b"rt_renderer_microfacets" in L.rt_last_error()   # null handles are refused before any device is touched
    assert L.rt_renderer_microfacets_info(None, out) != 0 and L.rt_renderer_kernel_microfacet(None, out) != 0 and L.rt_multi_renderer_microfacets(None, None, 0) != 0
    assert L.rt_multi_renderer_microfacets_info(None, out) != 0
    assert hasattr(p.api, "microfacet_batch") and hasattr(p.api, "probe_microfacet")
    assert (p.capi.MFAC_SPECULAR, p.capi.MFAC_BASE, p.capi.MFAC_ABSORBED, p.capi.MFAC_BACKSIDE) == (MT.SPECULAR, MT.BASE, MT.ABSORBED, MT.BACKSIDE)
