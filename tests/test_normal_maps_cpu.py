"""Normal maps without a GPU: the host function the kernels share against the numpy twin, bit for bit, with every way out of the rule counted;
mathematics no kernel code shares, under a bound derived from the 8-bit step; the identity of flat maps and of strength 0; the host surface with its refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import _nmap_twin as NT
import _nmap_worlds as NW
import _tex_worlds as XW
import _kernel_table as KT
from _common import ROOT, bits_equal, mismatch_report, pkg

F = np.float32


@pytest.fixture(scope="module")
def p():
    pk = pkg()
    from ray_tracing_v06_amd import image_io, mesh_io  # noqa: F401  (now attributes of the package)
    return pk


# ---- 1. the twin ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_function_is_the_twin_bit_for_bit(p):
    tab, cases = NW.table(), NW.random_cases()
    got_n, got_path = NW.run_cases(p.api.normal_map_batch, NW.api_table(tab), cases)
    want_n, want_path = NW.run_cases(NT.case, tab, cases)
    assert (got_path == want_path).all(), np.nonzero(got_path != want_path)[0][:5]
    assert bits_equal(got_n, want_n), mismatch_report(got_n, want_n)
    c = NT.counts(got_path)
    assert c["replaced"] > 500 and c["flat"] > 500 and c["facing"] > 100 and c["no_frame"] == 0, c   # random coordinates span an area; the aimed cases do not
    kept = got_path != NT.REPLACED
    assert bits_equal(got_n[kept], cases["normal"][kept])   # where the normal stays, its bits stay
    assert not bits_equal(got_n[~kept], cases["normal"][~kept])


def test_the_aimed_cases_take_every_way_out_of_the_rule(p):
    tab, cases, expected = NW.aimed_cases()
    got_n, got_path = NW.run_cases(p.api.normal_map_batch, NW.api_table(tab), cases)
    want_n, want_path = NW.run_cases(NT.case, tab, cases)
    assert bits_equal(got_n, want_n), mismatch_report(got_n, want_n)
    assert got_path.tolist() == want_path.tolist() == expected.tolist(), list(zip(NW.AIMED, got_path.tolist(), expected.tolist()))
    c = NT.counts(got_path)
    assert c == {"replaced": 4, "flat": 3, "no_tangent": 2, "no_length": 1, "facing": 2, "no_frame": 2}, c   # every return path fires
    kept = got_path != NT.REPLACED
    assert bits_equal(got_n[kept], cases["normal"][kept])
    # mirrored coordinates turn the tangent around and the bitangent with it: the same map bends the normal the other way along u
    mirrored, upright = NW.AIMED.index("mirrored UVs"), NW.AIMED.index("upright UVs")
    assert got_n[mirrored][0] < 0 < got_n[upright][0] and got_n[mirrored][2] > 0.9 and got_n[upright][2] > 0.9
    # seen from inside a sphere the normal points along the ray, and so does the bent one
    inside = NW.AIMED.index("inside a sphere")
    assert float(np.dot(got_n[inside], cases["ray_d"][inside])) > 0


# ---- 2. mathematics no kernel shares ----------------------------------------------------------------------------------------------------------------------------
# A map stores round(127 n) per component, so a decoded component is off by at most half a step, 0.5 / 127; the bent vector g (an orthonormal frame applied to m)
# is off by at most sqrt(3) * 0.5 / 127 in length, and normalising two vectors, one of them of length 1, at most doubles their distance.  1e-5 covers fp32.
BOUND = 2.0 * np.sqrt(3.0) * 0.5 / 127.0 + 1e-5


def _surfaces(n, rng):
    """n cases each on an axis-aligned parallelogram, a UV triangle and a sphere: (surface, a, b, tri_uv, normal, dPdu, dPdv) with the analytic tangents"""
    out = []
    u, v = np.tile(np.array([2.0, 0, 0], F), (n, 1)), np.tile(np.array([0, 0, -3.0], F), (n, 1))
    nq = np.tile(np.array([0, 1.0, 0], F), (n, 1))   # cross(u, v) = (0, 6, 0)
    out.append((np.full(n, NT.PLANAR, np.uint32), u, v, np.zeros((n, 6), F), nq, u, v))
    tu, tv = np.tile(np.array([1.0, 0.5, 0], F), (n, 1)), np.tile(np.array([-0.5, 2.0, 0], F), (n, 1))
    t = np.tile(np.array([0.1, 0.2, 0.9, 0.3, 0.2, 0.8], F), (n, 1))   # det > 0
    du1, dv1, du2, dv2 = 0.8, 0.1, 0.1, 0.6
    pu, pv = tu.astype(np.float64) * dv2 - tv.astype(np.float64) * dv1, tv.astype(np.float64) * du1 - tu.astype(np.float64) * du2
    out.append((np.full(n, NT.TRI_UV, np.uint32), tu, tv, t, np.tile(np.array([0, 0, 1.0], F), (n, 1)), pu, pv))
    sn = rng.standard_normal((n, 3))
    sn[:, 1] *= 0.5   # away from the poles
    sn = (sn / np.linalg.norm(sn, axis=1, keepdims=True)).astype(F)
    out.append((np.full(n, NT.SPHERE, np.uint32), sn, np.zeros((n, 3), F), np.zeros((n, 6), F), sn,
                np.stack([sn[:, 2], np.zeros(n), -sn[:, 0]], axis=1), np.tile(np.array([0, 1.0, 0]), (n, 1))))
    return out


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_a_constant_tilt_bends_every_normal_by_the_analytic_vector(p, filt):
    rng = np.random.default_rng(3)
    m0 = np.array([0.3, -0.2, 1.0])
    m0 /= np.linalg.norm(m0)
    tab = [(np.broadcast_to(NT.encode(m0), (3, 4, 3)).copy(), "repeat", filt)]
    n = 64
    for surface, a, b, t, normal, dpdu, dpdv in _surfaces(n, rng):
        want, T, B = NT.apply64(np.tile(m0, (n, 1)), dpdu, dpdv, normal)
        ray_d = (-want - normal.astype(np.float64)).astype(F)   # sees both normals from the front
        got, path = p.api.normal_map_batch(tab, surface, a, b, t, normal, ray_d, rng.random(n) * 3 - 1, rng.random(n) * 3 - 1, np.zeros(n, np.uint32), np.ones(n, F))
        assert (path == NT.REPLACED).all()
        err = float(np.abs(got - want).max())
        assert err <= BOUND, (int(surface[0]), err, BOUND)
        assert float(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max()) < 1e-6


def test_a_sine_ridge_from_a_height_field_bends_normals_as_its_slope_says(p):
    W, H, A, k, scale = 16, 4, 0.8, 2, 1.5
    i = np.arange(W)
    height = np.tile(A * np.sin(2 * np.pi * k * i / W), (H, 1))
    img = p.image_io.height_to_normal_map(height, scale, wrap="repeat")
    assert img.shape == (H, W, 3) and img.dtype == np.uint8 and (img[:, :, 1] == 128).all()   # no slope along v
    slope = A * np.sin(2 * np.pi * k / W) * np.cos(2 * np.pi * k * i / W)   # the central difference of a sine, exactly
    field = np.stack([-scale * slope, np.zeros(W), np.ones(W)], axis=1)
    field /= np.linalg.norm(field, axis=1, keepdims=True)
    rng = np.random.default_rng(4)
    u = ((i + 0.5) / W).astype(F)   # texel centres: nearest and bilinear agree there up to rounding
    for filt in ("nearest", "bilinear"):
        for surface, a, b, t, normal, dpdu, dpdv in _surfaces(W, rng):
            want, _, _ = NT.apply64(field, dpdu, dpdv, normal)
            ray_d = (-want - normal.astype(np.float64)).astype(F)
            got, path = p.api.normal_map_batch([(img, "repeat", filt)], surface, a, b, t, normal, ray_d, u, np.full(W, 0.625, F), np.zeros(W, np.uint32), np.ones(W, F))
            flat = (img[0, :, 0] == 128)
            assert (path[~flat] == NT.REPLACED).all() and (path[flat] == NT.FLAT).all()
            assert float(np.abs(got - want).max()) <= BOUND
    assert (p.image_io.height_to_normal_map(np.full((3, 5), 2.5), 9.0, wrap="clamp") == np.array([128, 128, 255], np.uint8)).all()   # a constant field is the flat map
    ramp = p.image_io.height_to_normal_map(np.tile(np.arange(6.0), (2, 1)), 1.0, wrap="clamp")
    assert ramp[0, 2, 0] < ramp[0, 0, 0] < 128 and ramp[0, 2, 0] == ramp[0, 3, 0]   # clamped edges see half the slope; uphill along +u leans the normal to -u


def test_the_frame_is_orthogonal_and_the_bitangent_follows_v(p):
    rng = np.random.default_rng(5)
    n = 256
    normal = rng.standard_normal((n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(F)
    dpdu, dpdv = (rng.standard_normal((n, 3)) * 3).astype(F), (rng.standard_normal((n, 3)) * 3).astype(F)
    detail = {}
    NT.apply(np.tile(np.array([1.0, 0.2, 0.9], F), (n, 1)), np.ones(n, F), dpdu, dpdv, -normal, normal, detail)
    T, B, N = (detail[k].astype(np.float64) for k in "TBN")
    tol = 8 * np.finfo(F).eps   # a handful of fp32 roundings on unit vectors
    assert np.abs((T * N).sum(axis=1)).max() < tol * 4 and np.abs((B * N).sum(axis=1)).max() < tol * 4   # (cancellation in dPdu - N (N . dPdu) costs |dPdu| / |T| more)
    assert np.abs((T * B).sum(axis=1)).max() < tol
    assert ((B * dpdv).sum(axis=1) >= 0).all()
    # the same from the host function: a map of pure +u gives T, a map of pure +v gives B — for both handednesses of (dPdu, dPdv)
    tab = [(np.array([[[255, 128, 128], [128, 255, 128]]], np.uint8), "clamp", "nearest")]
    given = np.full(n, NT.GIVEN, np.uint32)
    for sign in (1.0, -1.0):
        dv = (dpdv * F(sign)).astype(F)
        want, T64, B64 = NT.apply64(np.tile([0.0, 1.0, 0.0], (n, 1)), dpdu, dv, normal)
        ray_d = (-normal.astype(np.float64) - T64 - B64).astype(F)
        got_t, path_t = p.api.normal_map_batch(tab, given, dpdu, dv, None, normal, ray_d, np.full(n, 0.25, F), np.zeros(n, F), np.zeros(n, np.uint32), np.ones(n, F))
        got_b, path_b = p.api.normal_map_batch(tab, given, dpdu, dv, None, normal, ray_d, np.full(n, 0.75, F), np.zeros(n, F), np.zeros(n, np.uint32), np.ones(n, F))
        assert (path_t == NT.REPLACED).all() and (path_b == NT.REPLACED).all()
        assert np.abs((got_t.astype(np.float64) * N).sum(axis=1)).max() < tol * 4 and np.abs((got_b.astype(np.float64) * N).sum(axis=1)).max() < tol * 4
        assert ((got_b.astype(np.float64) * dv).sum(axis=1) > 0).all()   # B points towards growing v
        assert np.abs(got_b - want).max() < 1e-5 and np.abs(got_t - T64).max() < 1e-5


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("wrap", ["clamp", "repeat"])
def test_flat_maps_and_strength_zero_replace_nothing(p, wrap, filt):
    flat = [(XW.constant(5, 3, (128, 128, 255)), wrap, filt), (XW.constant(2, 2, (128, 128, 7)), wrap, filt), (XW.constant(1, 1, (128, 128, 128)), wrap, filt)]
    anymap = [(XW.image(5, 3, seed=9), wrap, filt), (XW.image(8, 4, seed=9), wrap, filt), (XW.image(1, 1, seed=9), wrap, filt)]
    _, aimed, _ = NW.aimed_cases()
    for cases in (NW.random_cases(2048, seed=7), aimed):
        cases = dict(cases, index=(cases["index"] % 3).astype(np.uint32))
        got, path = NW.run_cases(p.api.normal_map_batch, flat, cases)   # a flat map at any strength
        assert (path != NT.REPLACED).all() and bits_equal(got, cases["normal"])
        assert np.isin(path, (NT.FLAT, NT.NO_FRAME)).all()
        got, path = NW.run_cases(p.api.normal_map_batch, anymap, dict(cases, strength=np.zeros_like(cases["strength"])))   # any map at strength 0
        assert (path != NT.REPLACED).all() and bits_equal(got, cases["normal"])


# ---- 4. the host surface ------------------------------------------------------------------------------------------------------------------------------------------
def _scene(p):
    s = p.Scene()
    mats = dict(lam=s.Lambertian((0.5, 0.5, 0.5)), metal=s.Metal((0.8, 0.8, 0.8), 0.2), glass=s.Dielectric((1, 1, 1), 1.5), checker=s.LambertianTexture((0, 0, 0), (1, 1, 1), 2.0),
                light=s.DiffuseLight((4, 4, 4)), fog=s.Isotropic((1, 1, 1), 0.5), image=None, noise=None)
    s.set_perlin(3)
    mats["noise"] = s.NoiseTexture(2.0)
    s.set_image(XW.image(5, 3))
    mats["image"] = s.ImageTexture(0)
    bump = s.add_image(XW.image(8, 4, seed=2), "repeat", "bilinear")
    for k, x in enumerate(mats.values()):
        s.MakeSphere((2.0 * k, 0, 0), 0.7, x)
    v, f = p.mesh_io.icosphere(0)
    s.MakeMesh(v, f, mats["lam"], translate=(0, 3, 0))
    return s, mats, bump


def test_scene_adders_refusals_and_builders(p):
    s, mats, bump = _scene(p)
    assert s.normal_maps() is None   # NULL, 0 while no material has one
    for name in ("lam", "metal", "checker", "noise", "image"):
        s.set_normal_map(mats[name], bump, 0.5 + mats[name])
    table = s.normal_maps()
    assert table.dtype == p.capi.NORMAL_MAP_DT and table.dtype.itemsize == 16 and len(table) == len(mats)
    for name, m in mats.items():
        takes = name in ("lam", "metal", "checker", "noise", "image")
        assert table[m]["on"] == (1 if takes else 0) and (not takes or (table[m]["image"] == bump and table[m]["strength"] == F(0.5 + m)))
    before = table.tobytes()
    for bad, why in ((lambda: s.set_normal_map(mats["glass"], bump), "dielectric"), (lambda: s.set_normal_map(mats["light"], bump), "light"),
                     (lambda: s.set_normal_map(mats["fog"], bump), "medium"), (lambda: s.set_normal_map(99, bump), "no material 99"),
                     (lambda: s.set_normal_map(mats["lam"], 256), "image index"), (lambda: s.set_normal_map(mats["lam"], bump, -1.0), "strength"),
                     (lambda: s.set_normal_map(mats["lam"], bump, float("nan")), "strength"), (lambda: s.set_normal_map(mats["lam"], bump, float("inf")), "strength"),
                     (lambda: s.clear_normal_map(99), "no material 99")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            bad()
        assert e.value.code == 1   # RT_ERR_INVALID
        assert s.normal_maps().tobytes() == before   # and the scene is unchanged
    for build in (s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList):   # materials are never permuted: the table is the same under each
        build()
        assert s.normal_maps().tobytes() == before
        assert s.getWorldPtr().normal_maps.tobytes() == before   # and travels beside the flat world
    s.set_normal_map(mats["lam"], 0, 2.0)   # a second call replaces the first
    assert tuple(s.normal_maps()[mats["lam"]])[:3] == (1, 0, F(2.0))
    for name in ("lam", "metal", "checker", "noise"):
        s.clear_normal_map(mats[name])
    assert s.normal_maps()["on"].sum() == 1
    s.clear_normal_map(mats["image"])
    assert s.normal_maps() is None and not hasattr(s.getWorldPtr(), "normal_maps")


def test_batch_refusals(p):
    tab, cases, _ = NW.aimed_cases()
    tab = NW.api_table(tab)
    for change, why in ((dict(index=np.full(14, 7, np.uint32)), "no entry 7"), (dict(surface=np.full(14, 4, np.uint32)), "unknown surface"),
                        (dict(strength=np.full(14, -1, F)), "strength"), (dict(strength=np.full(14, np.nan, F)), "strength"), (dict(tri_uv=None), "tri_uv is null")):
        with pytest.raises(p.capi.RtError, match=why):
            NW.run_cases(p.api.normal_map_batch, tab, dict(cases, **change))


MTL = """newmtl bricks
Kd 0.5 0.25 0.125
map_Kd bricks.png
map_Bump -bm 0.75 bricks_n.png
newmtl plain
Kd 0.8 0.1 0.1
newmtl a
norm sub/a_n.png
newmtl b
map_bump -s 2 2 -bm 2 b_n.png
newmtl c
bump c_n.png   # a comment
"""


def test_load_mtl_reads_the_four_keywords_and_bm(p, tmp_path):
    (tmp_path / "m.mtl").write_text(MTL)
    mats = p.mesh_io.load_mtl(str(tmp_path / "m.mtl"))
    at = lambda *names: os.path.join(str(tmp_path), *names)   # noqa: E731
    assert (mats["bricks"]["normal_map"], mats["bricks"]["normal_strength"], mats["bricks"]["map_Kd"]) == (at("bricks_n.png"), 0.75, at("bricks.png"))
    assert (mats["plain"]["normal_map"], mats["plain"]["normal_strength"]) == (None, 1.0)
    assert (mats["a"]["normal_map"], mats["a"]["normal_strength"]) == (at("sub", "a_n.png"), 1.0)
    assert (mats["b"]["normal_map"], mats["b"]["normal_strength"]) == (at("b_n.png"), 2.0)
    assert (mats["c"]["normal_map"], mats["c"]["normal_strength"]) == (at("c_n.png"), 1.0)
    (tmp_path / "bad.mtl").write_text("newmtl x\nbump -bm -1 x.png\n")
    with pytest.raises(ValueError, match="-bm"):
        p.mesh_io.load_mtl(str(tmp_path / "bad.mtl"))


def test_both_languages_mirror_the_surface(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("rt_scene_set_normal_map", "rt_scene_clear_normal_map", "rt_scene_normal_maps", "rt_normal_map_batch", "rt_probe_normal_map", "rt_renderer_normal_maps",
                 "rt_renderer_normal_maps_info", "rt_renderer_kernel_normal_map", "rt_multi_renderer_normal_maps", "rt_multi_renderer_normal_maps_info"):
        assert name in header and name in p.capi.SYMBOLS and hasattr(p.lib(), name)
    assert "SetNormalMap(" in hpp and "ClearNormalMap(" in hpp and "SetNormalMaps(" in hpp
    for name in ("set_normal_map", "clear_normal_map", "normal_maps"):
        assert hasattr(p.Scene, name)
    for name in ("normal_maps", "normal_maps_info", "kernel_normal_map"):
        assert hasattr(p.Renderer, name)
    assert hasattr(p.MultiRenderer, "normal_maps") and hasattr(p.MultiRenderer, "normal_maps_info")
    L, out = p.lib(), (C.c_uint32 * 2)()
    assert L.rt_renderer_normal_maps(None, None, 0) != 0 and b"rt_renderer_normal_maps" in L.rt_last_error()   # null handles are refused before any device is touched
    assert L.rt_renderer_normal_maps_info(None, out) != 0 and L.rt_renderer_kernel_normal_map(None, out) != 0 and L.rt_multi_renderer_normal_maps(None, None, 0) != 0
    assert hasattr(p.api, "normal_map_batch") and hasattr(p.api, "probe_normal_map") and hasattr(p.image_io, "height_to_normal_map")


# ---- 5. the kernel forms and the launch image -----------------------------------------------------------------------------------------------------------------------
def test_form_list_is_the_set_of_instantiations_and_the_older_counts_stand():
    """every form of stream_kernel_for()'s NORMAL_MAP and NORMAL_MAP_ENV_TREE families has a recipe in the list the GPU tests run, and nothing else has"""
    import _env_tree_worlds as VW
    import _tri_worlds as TW
    for family in ("NORMAL_MAP", "NORMAL_MAP_ENV_TREE"):
        shipped = KT.family(family)
        assert len(shipped) == KT.count(family) == 8   # (the reader raises on a line of the table it cannot read)
        assert shipped == set(NW.FORMS) == set(VW.FORMS), shipped ^ set(NW.FORMS)
    assert all(f[2] == 2 for f in NW.FORMS) and all(NW.FORMS[f] == TW.FORMS[f] for f in NW.FORMS)
    for family, count in (("NEE", 16), ("TRI", 16), ("TRI_NEE", 16), ("LIGHT_TREE", 16), ("ENV_LIGHT", 8), ("ENV_TREE", 8)):
        assert KT.count(family) == count, family   # nothing existing moved
    kernel = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_stream_kernel.hpp")).read()
    assert "static_assert(!NMAP || (EXT == 2 && TRI)" in kernel and "bool NMAP = false>" in kernel


def test_the_tail_is_what_it_was_without_a_table_and_points_at_the_records_with_one(tmp_path):
    """rt_launch_image.hpp's append_tail, compiled into a small host program: with no normal-map table the bytes are those of a tail composed without the new
    fields ever set; with one, the fourth lane of the texture header is the number of vec4 from it to the records, which follow the entries"""
    import subprocess
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
    for (int with_tex = 0; with_tex < 2; with_tex++)
        for (int with_nm = 0; with_nm < 2; with_nm++) {
            Riders<Tex> r;
            r.normals = vn; r.n_normal_floats = 9; r.coords = uv; r.n_coord_floats = 6;
            r.env = true; r.env_w = 16; r.env_h = 8; r.env_u0 = 0.25f; r.env_texels = 0x1122334455667788ull;
            if (with_tex) { r.textures = true; r.texture = tex; r.n_textures = 3; r.texture_texels = 0x0102030405060708ull; }
            if (with_nm) { r.normal_maps = nm; r.n_normal_maps = 2; }
            std::vector<Vec4> out(2, Vec4{7, 7, 7, 7});
            append_tail(out, r);
            std::printf("%d %d %zu:", with_tex, with_nm, out.size());
            for (const Vec4& v : out) std::printf(" %x %x %x %x", v.x, v.y, v.z, v.w);
            std::printf("\n");
        }
    return 0;
}
''')
    exe = tmp_path / "tail"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    words = {tuple(int(x) for x in line.split(":")[0].split()[:2]): line.split(":")[1].split() for line in lines}
    assert words[(0, 0)] == words[(0, 1)]   # records without a texture table to hang them off are not written
    off, on = words[(1, 0)], words[(1, 1)]
    assert len(on) == len(off) + 2 * 4 and len(off) == (2 + 1 + 3 + 2 + 2 + 1 + 3) * 4
    tex_at = int(off[2 * 4 + 3], 16)           # the tail header's fourth word
    header = (2 + tex_at) * 4
    assert off[header:header + 4] == ["5060708", "1020304", "3", "0"]   # today's header: (texels low, texels high, n, 0)
    assert on[header:header + 4] == ["5060708", "1020304", "3", "4"]    # ... and with a table: 1 + n entries on
    assert on[:header] == off[:header] and on[header + 4:len(off)] == off[header + 4:]   # nothing else moved
    assert on[len(off):] == ["1", "2", "3f000000", "0", "0", "0", "0", "0"]
    # the bytes without a table are the bytes the committed layout check holds: tests/cpp_launch_image builds and runs untouched
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_launch_image")])
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp_launch_image", "launch_image_check")])
