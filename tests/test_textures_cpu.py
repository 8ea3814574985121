"""The texture table without a GPU: the host function the kernels share against the numpy twin, bit for bit; three properties no kernel code
shares; bilinear against float64 under a derived tolerance; the host surface with every refusal; OBJ material groups and MTL files."""
import ctypes as C
import os

import numpy as np
import pytest

import _tex_twin as XT
import _tex_worlds as XW
import _uv_twin as UT
from _common import bits_equal, mismatch_report, pkg

F = np.float32


@pytest.fixture(scope="module")
def p():
    return pkg()


def five_images():
    return [XW.image(w, h) for w, h in XW.SIZES]


# ---- 1. the twin ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", XT.MODES, ids=["clamp-nearest", "clamp-bilinear", "repeat-nearest", "repeat-bilinear"])
def test_the_host_function_is_the_twin_bit_for_bit(p, modes):
    images = five_images()
    table = [(img, *modes) for img in images]   # five entries of different sizes in one table: every first-texel offset is met
    for k, (w, h) in enumerate(XW.SIZES):
        u, v = XW.coords(w, h)
        index = np.full(len(u), k, np.uint32)
        got = p.api.texture_lookup_batch(table, index, u, v)
        want = XT.value(images[k], *modes, u, v)
        assert bits_equal(got, want), (w, h, mismatch_report(got, want))
        assert np.isfinite(got).all()   # a coordinate that is not a number lands on a texel
    nan = np.array([np.nan], F)
    got = p.api.texture_lookup_batch(table, np.array([2], np.uint32), nan, nan)   # column 0 and, after the flip, the bottom row
    zero = np.zeros(1, F)
    assert bits_equal(got, p.api.texture_lookup_batch(table, np.array([2], np.uint32), zero, zero))   # NaN is 0 under every mode pair
    if modes[1] == XT.NEAREST:
        assert bits_equal(got[0], images[2][2, 0].astype(F) * XT.SCALE)


def test_mixed_indices_in_one_call_reach_their_own_image(p):
    images = five_images()
    table = [(img, *XT.MODES[k % 4]) for k, img in enumerate(images)]
    rng = np.random.default_rng(5)
    index = rng.integers(0, 5, 4000).astype(np.uint32)
    u, v = (rng.random(4000, dtype=F) * F(4) - F(1.5)).astype(F), (rng.random(4000, dtype=F) * F(4) - F(1.5)).astype(F)
    got = p.api.texture_lookup_batch(table, index, u, v)
    want = XT.lookup(table, index, u, v)
    assert bits_equal(got, want), mismatch_report(got, want)


# ---- 2. clamp / nearest is image_texel -----------------------------------------------------------------------------------------------------------------------
def test_clamp_nearest_is_image_texel(p):
    for w, h in XW.SIZES:
        img = XW.image(w, h)
        u, v = XW.coords(w, h)
        ok = ~(np.isnan(u) | np.isnan(v))   # image_texel converts a NaN to an integer: it defines no texel for one
        got = p.api.texture_lookup_batch([(img, "clamp", "nearest")], np.zeros(int(ok.sum()), np.uint32), u[ok], v[ok])
        want = UT.texel(img, u[ok], v[ok])
        assert bits_equal(got, want), (w, h, mismatch_report(got, want))


# ---- 3. three properties that no kernel code shares ---------------------------------------------------------------------------------------------------------
def test_a_constant_image_is_exactly_constant(p):
    colour = np.array([201, 7, 99], np.uint8)
    for w, h in XW.SIZES:
        u, v = XW.coords(w, h)
        for modes in XT.MODES:
            got = p.api.texture_lookup_batch([(XW.constant(w, h, colour), *modes)], np.zeros(len(u), np.uint32), u, v)
            assert bits_equal(got, np.broadcast_to(colour.astype(F) * XT.SCALE, got.shape)), (w, h, modes)


def test_bilinear_at_texel_centres_of_power_of_two_images_is_nearest(p):
    for w, h in [(1, 1), (2, 2), (8, 4), (16, 16)]:
        img = XW.image(w, h)
        i, j = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
        u = ((i.reshape(-1).astype(F) + F(0.5)) / F(w)).astype(F)
        v = ((j.reshape(-1).astype(F) + F(0.5)) / F(h)).astype(F)
        zero = np.zeros(len(u), np.uint32)
        for wrap in ("clamp", "repeat"):
            near = p.api.texture_lookup_batch([(img, wrap, "nearest")], zero, u, v)
            bil = p.api.texture_lookup_batch([(img, wrap, "bilinear")], zero, u, v)
            assert bits_equal(bil, near), (w, h, wrap, mismatch_report(bil, near))
            assert bits_equal(near, img[h - 1 - j.reshape(-1), i.reshape(-1)].astype(F) * XT.SCALE)   # and it is that texel: row 0 is the top, v = 0 the bottom


def test_repeat_is_periodic_on_dyadic_coordinates(p):
    rng = np.random.default_rng(9)
    u = (rng.integers(0, 1024, 500).astype(F) / F(1024)).astype(F)   # k / 1024 + an integer within +-8 is exact in float32
    v = (rng.integers(0, 1024, 500).astype(F) / F(1024)).astype(F)
    k, m = rng.integers(-8, 9, 500).astype(F), rng.integers(-8, 9, 500).astype(F)
    for w, h in XW.SIZES:
        img = XW.image(w, h)
        zero = np.zeros(500, np.uint32)
        for filt in ("nearest", "bilinear"):
            base = p.api.texture_lookup_batch([(img, "repeat", filt)], zero, u, v)
            moved = p.api.texture_lookup_batch([(img, "repeat", filt)], zero, u + k, v + m)
            assert bits_equal(moved, base), (w, h, filt, mismatch_report(moved, base))


# ---- 4. bilinear against float64 -------------------------------------------------------------------------------------------------------------------------------
def test_bilinear_against_float64(p):
    """Tolerance 2^-16 absolute, derived: rounding u * W moves fx by at most W * 2^-24 <= 2^-18 for W <= 64; the slope is at most 1 per unit of fx; the three
    lerps and the 1/255 constant add under 2^-20.  Where floor(u * W - 0.5) steps, fp32 and fp64 may pick neighbouring cells; the value is continuous there (fx = 0
    of one cell is fx = 1 of the other), under CLAMP's edges and REPEAT's seam too, so the bound holds across the step."""
    rng = np.random.default_rng(11)
    for w, h in [(5, 3), (16, 16), (64, 7), (37, 64)]:
        img = XW.image(w, h)
        u = (rng.random(6000) * 5 - 2).astype(F)
        v = (rng.random(6000) * 5 - 2).astype(F)
        zero = np.zeros(len(u), np.uint32)
        for wrap, name in ((XT.CLAMP, "clamp"), (XT.REPEAT, "repeat")):
            got = p.api.texture_lookup_batch([(img, name, "bilinear")], zero, u, v)
            want = XT.value64(img, wrap, u.astype(np.float64), v.astype(np.float64))
            worst = float(np.abs(got.astype(np.float64) - want).max())
            print(f"{w}x{h} {name}: max |fp32 - fp64| = {worst:.3e}")
            assert worst <= 2.0 ** -16, (w, h, name, worst)


# ---- 5. the host surface ---------------------------------------------------------------------------------------------------------------------------------------
def test_scene_round_trip_and_the_flat_world(p):
    assert C.sizeof(p.capi.WorldFlat) == 128 and p.capi.TEXTURE_DT.itemsize == 20
    s = p.Scene()
    assert s.textures() is None
    s.image_sampling(0, "repeat", "bilinear")   # the modes of entry 0 before (or without) its image
    rec, tex = s.textures()
    assert len(rec) == 1 and tuple(rec[0]) == (0, 0, 1, 1, 0) and len(tex) == 0
    imgs = [XW.image(5, 3), XW.image(1, 1), XW.image(8, 4)]
    s.set_image(imgs[0])
    assert s.add_image(imgs[1]) == 1 and s.add_image(imgs[2], "repeat", "nearest") == 2
    rec, tex = s.textures()
    assert [tuple(r) for r in rec] == [(5, 3, 1, 1, 0), (1, 1, 0, 0, 15), (8, 4, 1, 0, 16)]
    assert np.array_equal(tex, np.concatenate([i.reshape(-1, 3) for i in imgs]))
    s.image_sampling(1, "clamp", "bilinear")
    assert tuple(s.textures()[0][1]) == (1, 1, 0, 1, 15)
    m, m0 = s.ImageTexture(2), s.ImageTexture()
    s.MakeSphere((0, 0, -1), 0.5, m)
    s.BuildBVH_TopDown()
    assert s.arrays()[2][m]["albedo2"][0] == 2.0 and s.arrays()[2][m0]["albedo2"][0] == 0.0   # the index rides in rt_material.albedo2[0]; every adder before this wrote 0
    assert s.add_material(p.capi.MAT_LAMBERTIAN_IMAGE, (1, 1, 1), 0.5) >= 0   # param means nothing for this type: callers have written anything there
    w = s.getWorldPtr()
    assert w.image_width == 5 and w.image_height == 3   # the flat world still says entry 0 and nothing else
    assert len(w.textures[0]) == 3
    plain = p.Scene()
    plain.set_image(imgs[0])
    plain.MakeSphere((0, 0, -1), 0.5, plain.ImageTexture())
    plain.BuildBVH_TopDown()
    assert not hasattr(plain.getWorldPtr(), "textures")   # one image under the default modes: the world as it always was, no table pushed


def test_refusals_of_the_host_surface(p):
    s = p.Scene()
    img = XW.image(2, 2)
    for bad, word in ((lambda: s.add_image(np.zeros((0, 4, 3), np.uint8)), "bad size"), (lambda: s.add_image(img, 2, 0), "wrap"), (lambda: s.add_image(img, 0, 7), "filter"),
                      (lambda: s.image_sampling(1, "clamp", "nearest"), "no image 1"), (lambda: s.image_sampling(0, 5, 0), "wrap"), (lambda: s.image_sampling(0, 0, 5), "filter"),
                      (lambda: s.ImageTexture(-1), "image index"), (lambda: s.ImageTexture(1.5), "image index"), (lambda: s.ImageTexture(256), "image index"),
                      (lambda: s.ImageTexture(float("nan")), "image index")):
        with pytest.raises(p.capi.RtError, match=word) as e:
            bad()
        assert e.value.code == 1
    assert s.textures() is None   # nothing was added
    for k in range(1, 256):
        assert s.add_image(img) == k
    with pytest.raises(p.capi.RtError, match="RT_MAX_IMAGES"):
        s.add_image(img)
    assert len(s.textures()[0]) == 256
    table = [(XW.image(5, 3), 0, 0), (None, 0, 0), (XW.image(2, 2), 1, 1)]
    one = np.zeros(1, F)
    for index, word in ((3, "no entry 3"), (1, "no entry 1")):   # past the end; an empty entry
        with pytest.raises(p.capi.RtError, match="rt_texture_lookup_batch.*" + word):
            p.api.texture_lookup_batch(table, np.array([index], np.uint32), one, one)
    rec, tex = p.api.texture_table(table)
    gap = rec.copy()
    gap["first"][2] = 16
    with pytest.raises(p.capi.RtError, match="back to back"):
        p.api.texture_lookup_batch((gap, tex), np.array([0], np.uint32), one, one)
    mode = rec.copy()
    mode["wrap"][0] = 2
    with pytest.raises(p.capi.RtError, match="wrap"):
        p.api.texture_lookup_batch((mode, tex), np.array([0], np.uint32), one, one)
    half = rec.copy()
    half["height"][1] = 1
    with pytest.raises(p.capi.RtError, match="empty entry is 0 x 0"):
        p.api.texture_lookup_batch((half, tex), np.array([0], np.uint32), one, one)
    assert p.api.texture_lookup_batch(table, np.array([2, 0], np.uint32), np.zeros(2, F), np.zeros(2, F)).shape == (2, 3)


# ---- 6. OBJ material groups and MTL files ----------------------------------------------------------------------------------------------------------------------
OBJ = """mtllib two.mtl other.mtl
v 0 0 0
v 2 0 0
v 2 2 0
v 0 2 0
v 0 0 1
vt 0 0
vt 3 0
vt 3 2.5
vt 0 2.5
vt -1 -1
f 1/1 2/2 5/5
usemtl floor
f 1/1 2/2 3/3 4/4
usemtl paint
f 1/5 3/3 5/1
usemtl floor
f 2/2 3/3 5/5
"""
MTL = """# a comment
newmtl floor
Ka 1 1 1
Kd 0.5 0.25 0.125
map_Kd tiles.png
Ns 10
newmtl paint
Kd 0.8 0.1 0.1
newmtl sub
map_Kd -s 2 2 sub/dir/wood.ppm
"""


def test_obj_material_groups_and_mtl(p, tmp_path):
    from ray_tracing_v06_amd import mesh_io
    obj = tmp_path / "two.obj"
    obj.write_text(OBJ)
    (tmp_path / "two.mtl").write_text(MTL)
    names, libs = mesh_io.load_obj_materials(str(obj))
    v, f, t, tf = mesh_io.load_obj_uvs(str(obj))
    assert libs == ["two.mtl", "other.mtl"]
    assert names == [None, "floor", "floor", "paint", "floor"] and len(names) == len(f)   # the quad is a fan of two triangles, both "floor"
    assert float(t.max()) == 3.0 and float(t.min()) == -1.0   # a tiled vt: coordinates beyond 1 come through as they are
    mats = mesh_io.load_mtl(str(tmp_path / "two.mtl"))
    assert list(mats) == ["floor", "paint", "sub"]
    assert mats["floor"]["Kd"] == (0.5, 0.25, 0.125) and mats["floor"]["map_Kd"] == str(tmp_path / "tiles.png")
    assert mats["paint"]["Kd"] == (0.8, 0.1, 0.1) and mats["paint"]["map_Kd"] is None
    assert mats["sub"]["Kd"] is None and mats["sub"]["map_Kd"] == os.path.join(str(tmp_path), "sub", "dir", "wood.ppm")   # options before the file name are skipped
    # the tiled floor under REPEAT: the rule at the vertices' own coordinates is the rule at their fractional parts
    img = XW.image(5, 3)
    got = p.api.texture_lookup_batch([(img, "repeat", "nearest")], np.zeros(len(t), np.uint32), t[:, 0], t[:, 1])
    want = XT.value(img, XT.REPEAT, XT.NEAREST, t[:, 0], t[:, 1])
    assert bits_equal(got, want)
    s = p.Scene()
    floor = s.add_image(img, "repeat", "bilinear")
    rows = [i for i, n in enumerate(names) if n == "floor"]
    first, added = s.MakeMesh(v, f[rows], s.ImageTexture(floor), uvs=t, uv_faces=tf[rows])
    assert added == 3 and float(np.abs(s.texture_coords()["t1"]).max()) == 3.0
