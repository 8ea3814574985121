"""Solid glass without a GPU: the host batches against the numpy twin, bit for bit; rt_expf's contract and its error against float64; physics no
kernel shares, in float64 on the rule's outputs — a ray through a slab leaves parallel to how it entered, and the transmittance is Beer-Lambert's; the winding
checks of mesh_io; the scene's records, the kernel forms and the parsing; the twin's two pins and the test room."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _interior_twin as IT
import _interior_worlds as IW
import _mfac_worlds as MW
import _path_twin as PT
import _kernel_table as KT
from _common import ROOT, bits_equal, mismatch_report, pkg

F = np.float32
U = 2.0 ** -24
# the worst error of rt_expf over EVERY fp32 x in [-87, 0], in fp32 ulp against float64 exp, as tools/verify_expf.py measured it (at x = -71.04561614990234,
# 0xc28e175b; profiles/e26_expf_exhaustive.txt), rounded up in the last place.  The function is deterministic: a sample can do no worse, and needs no margin.
EXPF_WORST_ULP = 1.212228


@pytest.fixture(scope="module")
def p():
    pk = pkg()
    from ray_tracing_v06_amd import image_io, mesh_io  # noqa: F401  (now attributes of the package)
    return pk


def same(got, want):
    for g, w, name in zip(got, want, ("back", "eta", "T")):
        if g.dtype == np.uint32:
            assert (g == w).all(), (name, np.nonzero(g != w)[0][:5])
        else:
            assert bits_equal(g, w), (name, mismatch_report(g, w))


# ---- 1. the twin ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_function_is_the_twin_bit_for_bit(p):
    cases = IW.random_cases()
    got, want = IW.run_cases(p.api.interior_batch, cases), IW.run_cases(IT.case, cases)
    same(got, want)
    back, eta, T = got
    assert 1500 < back.sum() < 2600 and (T[back == 0] == 1).all() and (eta[back == 1] == cases["ior"][back == 1]).all()
    inside = T[back == 1]
    assert (inside >= 0).all() and (inside <= 1).all() and (inside == 0).sum() > 50 and (inside == 1).sum() > 50 and ((inside > 0) & (inside < 1)).sum() > 1000


def test_the_aimed_cases(p):
    cases, expected = IW.aimed_cases()
    got, want = IW.run_cases(p.api.interior_batch, cases), IW.run_cases(IT.case, cases)
    same(got, want)
    back, eta, T = got
    assert (back == expected).all(), [(n, int(b)) for n, b, e in zip(IW.AIMED, back, expected) if b != e]
    at = IW.AIMED.index
    assert (T[back == 0] == 1).all() and (eta[back == 0] == F(1) / cases["ior"][back == 0]).all() and (eta[back == 1] == cases["ior"][back == 1]).all()
    assert bits_equal(T[at("sigma 0, back")], np.ones(3, F))                                   # sigma = 0 changes no bit
    past = T[at("sigma dist past 87")]
    assert past[0] == 0 and past[2] == 0                                                       # 90 and 3000 are flushed to 0
    edge = T[at("sigma dist at 87")]
    assert edge[0] == 0 and edge[1] >= np.finfo(F).tiny and edge[2] == 0                       # exactly 87 flushes, a hair less does not
    assert (T[at("total reflection from inside")] < 1).all()                                   # charged whether or not it gets out
    assert bits_equal(T[at("a long direction")], IT.expf(-(cases["sigma"][at("a long direction")] * (F(0.02) * np.sqrt(F(30 * 30 + 20 * 20 + 100 * 100))))))


def test_expf_contract_and_error(p):
    x = IW.expf_samples()
    assert len(x) >= (1 << 22) + 2 * 33 * len(IT.BOUNDARIES) // 2
    y = p.api.expf_batch(x)
    assert bits_equal(y, IT.expf(x))
    assert (y >= 0).all() and (y <= 1).all()
    live = x > F(-87)
    assert (y[~live] == 0).all() and (y[live] >= np.finfo(F).tiny).all()                       # flushed at -87 and below; no denormal above
    edge = p.api.expf_batch(np.array([0.0, -0.0, np.nan, -np.inf, -87.0, -88.0, -1e30, -1e-45, np.nextafter(F(-87), F(0))], F))
    assert edge[0] == 1 and edge[1] == 1 and (edge[2:7] == 0).all() and edge[7] == 1 and edge[8] > 0
    ref = np.exp(x[live].astype(np.float64))
    err = np.abs(y[live].astype(np.float64) - ref) / np.ldexp(1.0, np.frexp(ref)[1] - 1 - 23)
    worst = int(np.argmax(err))
    print(f"rt_expf: worst error on {live.sum()} samples {err[worst]:.6f} ulp at x = {x[live][worst]!r}; recorded worst over all of [-87, 0]: {EXPF_WORST_ULP} ulp")
    assert err[worst] <= EXPF_WORST_ULP
    recorded = np.array([-71.04561614990234], F)                                                 # where the exhaustive sweep found it
    e = abs(float(p.api.expf_batch(recorded)[0]) - np.exp(float(recorded[0]))) / np.ldexp(1.0, np.frexp(np.exp(float(recorded[0])))[1] - 1 - 23)
    assert EXPF_WORST_ULP - 1e-6 <= e <= EXPF_WORST_ULP


# ---- 2. physics no kernel shares: float64 on the rule's outputs ----------------------------------------------------------------------------------------------------
def refract64(d, n, eta):
    """Snell's law in float64: unit d, unit n against it"""
    c = -np.dot(n, d)
    k = 1.0 - eta * eta * (1.0 - c * c)
    assert k >= 0
    return eta * d + (eta * c - np.sqrt(k)) * n


def test_a_ray_through_a_slab_leaves_parallel_to_how_it_entered(p):
    """Two parallel faces of a glass box of index 1.5, z = 0 (stored normal -z) and z = 1 (stored normal +z), met obliquely from below.  The batch gives the facing
    and eta of both hits; the refractions are float64.  What separates the exit direction from the entry direction is then counted: eta_in eta_out = fl(1 / 1.5)
    1.5 = 1 + delta with |delta| <= 2^-24 turns it by delta tan(theta); the direction inside is handed to the second case in float32, three roundings of 2^-24,
    an angle of at most sqrt(3) 2^-24, which the exit magnifies by eta cos(theta_in) / cos(theta_out) <= 1.5 / cos(theta): bound = (1.5 sqrt(3) / cos(theta) +
    tan(theta)) 2^-24, 2.2e-7 at 32 degrees.  Measured worst: 3.7e-8.  Under the parent's rule — back taken on the shading normal, which faces the ray, so never —
    the ray bends inwards twice and leaves 9 to 26 degrees off: the test shows that too."""
    worst = 0.0
    for d in ((0.6, 0.2, 1.0), (0.1, -0.3, 1.0), (-0.8, 0.5, 1.0), (0.0, 0.0, 1.0), (1.2, 0.9, 1.0)):
        d = np.array(d, np.float64)
        u = d / np.linalg.norm(d)
        cos_t = u[2]
        lower, upper = (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)
        facing = (0.0, 0.0, -1.0)                                   # against the ray at both faces
        b1, e1, _ = p.api.interior_batch([lower], [facing], [d], [1.0], [1.5], [(0, 0, 0)], [0])
        assert b1[0] == 0
        inside = refract64(u, np.array(facing), float(e1[0]))
        inside32 = inside.astype(F)
        b2, e2, _ = p.api.interior_batch([upper], [facing], [inside32], [1.0], [1.5], [(0, 0, 0)], [0])
        assert b2[0] == 1 and e2[0] == F(1.5)
        i64 = inside32.astype(np.float64)
        out = refract64(i64 / np.linalg.norm(i64), np.array(facing), float(e2[0]))
        delta = float(np.linalg.norm(out / np.linalg.norm(out) - u))
        bound = (1.5 * np.sqrt(3.0) / cos_t + np.sqrt(1 - cos_t * cos_t) / cos_t) * U
        worst = max(worst, delta)
        print(f"slab: theta {np.degrees(np.arccos(cos_t)):.1f} deg, exit off by {delta:.2e}, bound {bound:.2e}")
        assert delta <= bound
        parent = refract64(i64 / np.linalg.norm(i64), np.array(facing), float(e1[0]))   # the parent: the facing normal says front again, eta = 1 / ior again
        off = float(np.linalg.norm(parent / np.linalg.norm(parent) - u))
        assert off > 1e-2 or cos_t == 1.0, off                      # (normal incidence goes straight through either way)
    assert worst > 0.0


def test_the_transmittance_is_beer_lamberts(p):
    """Directions whose length float32 holds exactly (Pythagorean quadruples times powers of two: dot and sqrt round nothing), so that the exponent x = -(sigma (t
    len)) carries the two roundings of its products alone, a relative 2 2^-24, which exp turns into a relative 2 |x| 2^-24 of T, at most 2 |x| ulp.  Bound:
    rt_expf's recorded worst plus 2 |x| ulp.  Measured worst excess over rt_expf's own error: see the printed line."""
    rng = np.random.default_rng(3232)
    quads = np.array([(1, 2, 2), (2, 3, 6), (3, 4, 12), (0, 0, 1), (4, 4, 7), (1, 4, 8), (2, 6, 9), (6, 6, 7)], np.float64)
    n = 4096
    d = quads[rng.integers(0, len(quads), n)] * rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.integers(-6, 7, (n, 1))
    length = np.linalg.norm(d, axis=1)
    assert (length == length.astype(F)).all()
    t = (10.0 ** rng.uniform(-3, 1, n)).astype(F)
    sigma = (10.0 ** rng.uniform(-2, 1.5, (n, 3))).astype(F)
    Ng = d / length[:, None]                                        # the stored normals of the faces the rays leave through: every case is a back hit
    back, _, T = p.api.interior_batch(Ng, -Ng, d, t, np.full(n, 1.5, F), sigma, np.zeros(n, np.uint32))
    assert back.all()
    x = -(sigma.astype(np.float64) * (t.astype(np.float64) * length)[:, None])
    keep = x > -86.0                                                # (below, the flush to 0 is the contract, tested above)
    ref = np.exp(x[keep])
    err = np.abs(T[keep].astype(np.float64) - ref) / np.ldexp(1.0, np.frexp(ref)[1] - 1 - 23)
    bound = EXPF_WORST_ULP + 2.0 * np.abs(x[keep]) * (1 + 1e-6)
    print(f"Beer-Lambert: {keep.sum()} channels, worst error {err.max():.3f} ulp, worst share of its bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert (T[~keep] < 1e-37).all()


# ---- 3. the winding ---------------------------------------------------------------------------------------------------------------------------------------------
def box_mesh():
    v = np.array([(x, y, z) for x in (0, 1) for y in (0, 2) for z in (0, 3)], F)   # index = 4 x + 2 y + z
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.uint32)
    return v, f


def test_closed_outward_and_orient_outward(p):
    io = p.mesh_io
    solids = [io.icosphere(0), io.icosphere(1), io.icosphere(2), io.tetrahedron(), box_mesh()]
    v, f, _, _ = io.uv_sphere(8, 4)
    solids.append((v, f))
    for v, f in solids:
        assert io.closed_outward(v, f) and io.signed_volume(v, f) > 0
        assert (io.orient_outward(v, f) == f).all()
        flipped = f.copy()
        flipped[3] = flipped[3][::-1]                                                    # one face the other way round: inconsistent
        assert not io.closed_outward(v, flipped)
        with pytest.raises(ValueError, match="not consistently wound"):
            io.orient_outward(v, flipped)
        assert not io.closed_outward(v, f[1:])                                           # a hole
        with pytest.raises(ValueError, match="open"):
            io.orient_outward(v, f[1:])
        inside_out = np.ascontiguousarray(f[:, ::-1])
        assert not io.closed_outward(v, inside_out) and io.consistently_closed(v, inside_out) and io.signed_volume(v, inside_out) < 0
        repaired = io.orient_outward(v, inside_out)
        assert io.closed_outward(v, repaired) and (repaired == f).all()
        assert not io.closed_outward(v, np.concatenate([f, f[:1]]))                      # a face twice: an edge with three faces
    assert abs(io.signed_volume(*box_mesh()) - 6.0) < 1e-12
    v, f = io.icosphere(0)
    assert io.closed_outward(v * F(-1.0), f[:, ::-1]) and not io.closed_outward(v * F(-1.0), f)   # a mirrored mesh turns its winding
    with pytest.raises(ValueError, match="no volume"):
        io.orient_outward(np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F), np.array([[0, 1, 2], [0, 2, 1]], np.uint32))   # a two-sided leaf: closed, and flat
    assert not io.closed_outward(v, np.zeros((0, 3), np.uint32))


def test_a_box_of_the_scene_is_wound_outward(p):
    """rt_scene_add_box's six parallelograms: every stored normal points away from the box's centre, so the rule's `back` means inside"""
    s = p.Scene()
    s.MakeBox((1, 2, 3), (2, 4, 7), s.Dielectric((1, 1, 1), 1.5), rotate_y=30.0, translate=(0.5, 0, -1))
    s.MakeHittableList()
    quads = s.quads()
    assert len(quads) == 6
    centre = (quads["Q"] + 0.5 * quads["u"] + 0.5 * quads["v"]).astype(np.float64)
    middle = centre.mean(axis=0)
    assert (np.einsum("ij,ij->i", quads["normal"].astype(np.float64), centre - middle) > 0.4).all()


# ---- 4. the scene, the forms, the parsing -----------------------------------------------------------------------------------------------------------------------------
def test_scene_calls_refusals_and_builders(p):
    s = p.Scene()
    mats = dict(lam=s.Lambertian((0.5, 0.5, 0.5)), metal=s.Metal((0.8, 0.8, 0.8), 0.2), glass=s.Dielectric((1, 1, 1), 1.5), light=s.DiffuseLight((4, 4, 4)),
                fog=s.Isotropic((1, 1, 1), 0.5), glass2=s.Dielectric((1, 1, 1), 1.33), glass3=s.Dielectric((1, 1, 1), 2.4))
    for k, m in enumerate(mats.values()):
        s.MakeSphere((2.0 * k, 0, 0), 0.7, m)
    assert s.interiors() is None                                # NULL, 0 while no material has a record
    s.set_interior(mats["glass"], sigma=(0.25, 0.0, 2.0)).set_interior(mats["glass2"]).set_interior(mats["glass3"], color=(0.5, 1.0, 0.25), at=2.0)
    table = s.interiors()
    assert table.dtype == p.capi.INTERIOR_DT == IT.INTERIOR_DT and table.dtype.itemsize == 16 and len(table) == len(mats)
    for name, m in mats.items():
        assert table[m]["on"] == (1 if name.startswith("glass") else 0)
    assert tuple(table[mats["glass"]]["sigma"]) == (F(0.25), F(0.0), F(2.0)) and not table[mats["glass2"]]["sigma"].any()
    assert bits_equal(table[mats["glass3"]]["sigma"], np.array([np.log(2.0) / 2.0, 0.0, np.log(4.0) / 2.0]).astype(F))   # -ln(color) / at, in double, then rounded
    assert not np.signbit(table[mats["glass3"]]["sigma"]).any()
    before = table.tobytes()
    for bad, why in ((lambda: s.set_interior(mats["lam"]), "no dielectric"), (lambda: s.set_interior(mats["metal"]), "no dielectric"),
                     (lambda: s.set_interior(mats["light"]), "no dielectric"), (lambda: s.set_interior(mats["fog"]), "no dielectric"),
                     (lambda: s.set_interior(99), "no material 99"), (lambda: s.clear_interior(99), "no material 99"),
                     (lambda: s.set_interior(mats["glass"], sigma=(0.1, -0.1, 0.1)), "absorption coefficient"),
                     (lambda: s.set_interior(mats["glass"], sigma=float("inf")), "absorption coefficient"),
                     (lambda: s.set_interior(mats["glass"], sigma=(0.1, float("nan"), 0.1)), "absorption coefficient")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            bad()
        assert e.value.code == 1 and s.interiors().tobytes() == before   # RT_ERR_INVALID, and the scene is unchanged
    for bad in (lambda: s.set_interior(mats["glass"], color=(0.5, 0.5, 0.5)), lambda: s.set_interior(mats["glass"], at=1.0),
                lambda: s.set_interior(mats["glass"], sigma=1.0, color=(0.5, 0.5, 0.5), at=1.0), lambda: s.set_interior(mats["glass"], color=(0.5, 0.0, 0.5), at=1.0),
                lambda: s.set_interior(mats["glass"], color=(0.5, 1.5, 0.5), at=1.0), lambda: s.set_interior(mats["glass"], color=(0.5, 0.5, 0.5), at=0.0)):
        with pytest.raises(ValueError, match="set_interior"):
            bad()
        assert s.interiors().tobytes() == before
    for build in (s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList):   # materials are never permuted: the table is the same under each
        build()
        assert s.interiors().tobytes() == before
        w = s.getWorldPtr()
        assert w.interiors.tobytes() == before and not hasattr(w, "microfacets") and not hasattr(w, "normal_maps") and not hasattr(w, "textures")
    s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 1, 0), mats["glass"])   # a parallelogram added later, and a new material: the table grows by an off record
    later = s.Dielectric((1, 1, 1), 1.1)
    s.BuildBVH_SAH()
    assert s.interiors()[:len(mats)].tobytes() == before and len(s.interiors()) == len(mats) + 1 and s.interiors()[later]["on"] == 0
    assert s.getWorldPtr().interiors.tobytes() == s.interiors().tobytes()
    s.clear_interior(mats["glass"]).clear_interior(mats["lam"])
    assert (s.interiors()["on"] != 0).sum() == 2 and not s.interiors()[mats["glass"]]["sigma"].any()
    s.clear_interior(mats["glass2"]).clear_interior(mats["glass3"])
    assert s.interiors() is None and not hasattr(s.getWorldPtr(), "interiors")


def test_form_list_is_the_set_of_instantiations_and_the_older_counts_stand():
    """every form of stream_kernel_for()'s INTERIOR and INTERIOR_ENV_TREE families has a recipe in the list the GPU tests run, and nothing else has"""
    import _tri_worlds as TW
    for family in ("INTERIOR", "INTERIOR_ENV_TREE"):
        shipped = KT.family(family)
        assert len(shipped) == KT.count(family) == 8 and shipped == set(IW.FORMS) == set(MW.FORMS), shipped ^ set(IW.FORMS)
    assert all(IW.FORMS[f] == TW.FORMS[f] for f in IW.FORMS)
    for family, count in (("NEE", 16), ("TRI", 16), ("TRI_NEE", 16), ("LIGHT_TREE", 16), ("ENV_LIGHT", 8), ("ENV_TREE", 8), ("NORMAL_MAP", 8), ("NORMAL_MAP_ENV_TREE", 8),
                          ("MICROFACET", 8), ("MICROFACET_ENV_TREE", 8)):
        assert KT.count(family) == count, family   # nothing existing moved
    kernel = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_stream_kernel.hpp")).read()
    assert "static_assert(!INTR || MFAC" in kernel and "bool INTR = false, bool MFAC = false, bool NMAP = false>" in kernel
    shade = kernel[kernel.index("if (cur == K::SHADE)"):]
    assert shade.count("q_back") >= 4 and "if constexpr (INTR)" in shade   # the boolean is kept where set_face_normal compares, under the template argument


MTL = """newmtl amber
Kd 0.9 0.7 0.4
d 0.1
Ni 1.52
Tf 0.9 0.6 0.2
newmtl smoke
illum 7
Tf 0.5   # one value stands for three
newmtl spectral
Tf spectral file.rfl 1.0
newmtl clear
d 0.2
"""


def test_load_mtl_reads_the_transmission_filter(p, tmp_path):
    (tmp_path / "m.mtl").write_text(MTL)
    mats = p.mesh_io.load_mtl(str(tmp_path / "m.mtl"))
    assert mats["amber"]["transmission_filter"] == (0.9, 0.6, 0.2) and mats["amber"]["ior"] == 1.52 and mats["amber"]["dissolve"] == 0.1   # the older keys stay
    assert mats["smoke"]["transmission_filter"] == (0.5, 0.5, 0.5) and mats["smoke"]["illum"] == 7
    assert "transmission_filter" not in mats["spectral"] and "transmission_filter" not in mats["clear"]
    for text, why in (("newmtl x\nTf 1.5 0 0\n", "Tf must be"), ("newmtl x\nTf -0.1\n", "Tf must be"), ("Tf 0.5\n", "before any newmtl"), ("newmtl x\nTf 0.1 0.2\n", "one value or three"),
                      ("newmtl x\nTf\n", "one value or three")):
        (tmp_path / "bad.mtl").write_text(text)
        with pytest.raises(ValueError, match=why):
            p.mesh_io.load_mtl(str(tmp_path / "bad.mtl"))


def test_both_languages_mirror_the_surface(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("rt_scene_set_interior", "rt_scene_clear_interior", "rt_scene_interiors", "rt_interior_batch", "rt_probe_interior", "rt_expf_batch", "rt_probe_expf",
                 "rt_renderer_interiors", "rt_renderer_interiors_info", "rt_renderer_kernel_interior", "rt_multi_renderer_interiors"):
        assert name in header and name in p.capi.SYMBOLS and hasattr(p.lib(), name)
    for name in ("SetInterior(", "ClearInterior(", "Interiors(", "SetInteriors("):
        assert name in hpp
    for name in ("set_interior", "clear_interior", "interiors"):
        assert hasattr(p.Scene, name)
    for name in ("interiors", "interiors_info", "kernel_interior"):
        assert hasattr(p.Renderer, name)
    assert hasattr(p.MultiRenderer, "interiors")
    L, out = p.lib(), (C.c_uint32 * 2)()
    assert L.rt_renderer_interiors(None, None, 0) != 0 and b"rt_renderer_interiors" in L.rt_last_error()   # null handles are refused before any device is touched
    assert L.rt_renderer_interiors_info(None, out) != 0 and L.rt_renderer_kernel_interior(None, out) != 0 and L.rt_multi_renderer_interiors(None, None, 0) != 0
    for name in ("interior_batch", "probe_interior", "expf_batch", "probe_expf"):
        assert hasattr(p.api, name)
    assert (p.capi.INTERIOR_OFF, p.capi.INTERIOR_SOLID) == (IT.OFF, IT.SOLID)
    with pytest.raises(ValueError, match="one entry per case"):
        cases = IW.aimed_cases()[0]
        IW.run_cases(p.api.interior_batch, dict(cases, t=cases["t"][:-1]))
    rule = header[header.index("solid glass (DESIGN.md §32"):]
    for line in ("back = dot(d, Ng) > 0", "eta = back ? ior : 1 / ior", "len = sqrt(dot(d, d))", "dist = t len", "T_c = rt_expf of -(sigma_c dist)"):
        assert line in rule, line   # the rule, stated line by line


# ---- 5. the twin's two pins and the room ---------------------------------------------------------------------------------------------------------------------------
VIEWS = [IW.OUTSIDE, IW.INSIDE]


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_with_every_sigma_zero_the_own_loop_is_the_one_loop(env, view):
    """the loop that carries the transmittance, with nothing to carry, against _path_twin.radiance over the wrapped walk: every sample, bit for bit"""
    run = IW.run(env, False, view)
    assert run.facing_followed.all() and bits_equal(run.untinted, run.facing), mismatch_report(run.untinted, run.facing)
    assert not bits_equal(run.samples, run.facing)               # ... and the tint is seen
    assert run.info["turned"] > 100                              # the wrapper did turn normals, and the loop turned them back


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_a_table_of_records_that_are_all_off_is_no_table(p, env, view):
    """both loops with every record off against _rglass_twin's frame of the same room"""
    run = IW.run(env, False, view)
    cam = MW.as_oracle_camera(IW.camera(p, view))
    sky, light, tree = IW.GT_lights(p, run.scene, run.world, env)
    import _smooth_twin as ST
    trace = ST.smooth_walk(run.scene.vertex_normals())
    args = (run.world, cam, IW.W, IW.H, IW.DEPTH, IW.SEED)
    off = IW.all_off(run.interiors)
    own, followed = PT.frame_samples(lambda g, s: IT.radiance(*args, g, s, sky, off, light, tree, run.mfacs, None, trace), IW.W, IW.H, IW.SPP)
    assert run.off_followed.all() and followed.all() and bits_equal(own, run.off), mismatch_report(own, run.off)
    one, followed = PT.frame_samples(lambda g, s: IT.facing_radiance(*args, g, s, sky, off, light, tree, None, run.mfacs, None, None, trace), IW.W, IW.H, IW.SPP)
    assert followed.all() and bits_equal(one, run.off)
    assert not bits_equal(run.off, run.facing)                   # the facing alone changes the frame: the parent's frame is not this tree's


def test_the_room_follows_every_sample_and_meets_every_case():
    """the cap on samples left out is zero, in both views, plain and under mode 48; every counter is positive in each view"""
    for env in (False, True):
        for view in VIEWS:
            run = IW.run(env, False, view)
            assert run.followed.all() and np.isfinite(run.samples).all()
            for key, value in run.stats.items():
                assert value > 0, (env, view, key, run.stats)
    assert len(IW.run(False).interiors) == len(IW.run(False).mfacs) and (IW.run(False).interiors["on"] != 0).sum() == IW.RECORDS
