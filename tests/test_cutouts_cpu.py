"""Alpha cutouts without a GPU: the host batch against the numpy twin, bit for bit, over the three sources of coordinates; the rule's coordinates
and decision against a float64 restatement that shares no float32 code with the kernel; the scene's records through builders, list, later materials and clear,
with every set-time refusal; the MTL keyword, the PNG alpha reader and the procedural fence; the kernel forms; and the room the GPU tests render."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import _cutout_twin as CT
import _cutout_worlds as CW
import _interior_worlds as IW
import _tex_twin as XT
import _kernel_table as KT
from _common import ROOT, bits_equal, mismatch_report, pkg

F = np.float32


@pytest.fixture(scope="module")
def p():
    pk = pkg()
    from ray_tracing_v06_amd import image_io, mesh_io  # noqa: F401  (now attributes of the package)
    return pk


# ---- 1. the rule -------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_batch_is_the_twin_bit_for_bit(p):
    """a few thousand random cases: a parallelogram, a triangle under a record of coordinates, a triangle under the identity record; nearest / clamp and bilinear /
    repeat masks, a 1 x 1 and a 3 x 2 mask; cutoffs 0 and 1, and a cutoff equal to the value"""
    table, records = CW.case_table(), CW.case_records()
    assert [t[0].shape[:2] for t in table[3:5]] == [(1, 1), (2, 3)] and {(t[1], t[2]) for t in table[1:]} >= {(XT.CLAMP, XT.NEAREST), (XT.REPEAT, XT.BILINEAR)}
    given = p.api.texture_table(table)
    equal_to_cutoff = 0
    for name, quads, uv, rays, t, material in CW.batches():
        keep, tuv, value = p.api.cutout_batch(given, quads, uv, rays, t, records, material)
        want = CT.keeps(table, quads, uv, rays[:, 0:3], rays[:, 3:6], t, records, material)
        assert (keep == want[0]).all(), (name, np.nonzero(keep != want[0])[0][:5])
        assert bits_equal(tuv, want[1]), (name, mismatch_report(tuv, want[1]))
        assert bits_equal(value, want[2]), (name, mismatch_report(value, want[2]))
        rec = records[material]
        on = rec["on"] != 0
        assert (keep[~on] == 1).all() and not tuv[~on].any() and not value[~on].any()      # a record that is off asks nothing
        assert (keep[on & (rec["cutoff"] == 0)] == 1).all()                               # cutoff 0 keeps every hit
        ones = on & (rec["cutoff"] == 1)
        assert (keep[ones] == (value[ones] == 1)).all() and 0 < keep[ones].sum() < ones.sum()   # cutoff 1 keeps the fully opaque texels alone
        equal = on & (value == rec["cutoff"])
        assert (keep[equal] == 1).all()                                                   # a value equal to the cutoff is kept
        equal_to_cutoff += int((equal & (rec["cutoff"] > 0) & (rec["cutoff"] < 1)).sum())
        assert 200 < keep[on].sum() < on.sum() - 200
    assert equal_to_cutoff > 50
    name, quads, uv, rays, t, material = CW.batches()[2]   # the identity record gives the planar coordinates up to the sign of a zero: the same texel, the same decision
    planar = p.api.cutout_batch(given, quads, None, rays, t, records, material)
    under = p.api.cutout_batch(given, quads, uv, rays, t, records, material)
    assert (planar[0] == under[0]).all() and (planar[1] == under[1]).all() and bits_equal(planar[2], under[2])


def test_a_nan_keeps_the_hit_and_bad_cases_are_refused(p):
    table, records = CW.case_table(), CW.case_records()
    given = p.api.texture_table(table)
    name, quads, uv, rays, t, material = CW.batches()[0]
    bilinear = np.nonzero((records["on"] != 0) & (records["image"] == 2) & (records["cutoff"] == 0.5))[0][0]
    rays = rays[:4].copy()
    rays[:, 3] = np.inf   # an infinite direction: the coordinates are not numbers, and whatever the lookup makes of them, a value that is not a number keeps the hit
    keep, tuv, value = p.api.cutout_batch(given, quads[:4], None, rays, t[:4], records, np.full(4, bilinear, np.uint32))
    want = CT.keeps(table, quads[:4], None, rays[:, 0:3], rays[:, 3:6], t[:4], records, np.full(4, bilinear, np.uint32))
    assert (keep == want[0]).all() and bits_equal(value, want[2])
    assert (keep[np.isnan(value)] == 1).all()
    with pytest.raises(p.capi.RtError, match="there is no record"):
        p.api.cutout_batch(given, quads[:4], None, rays, t[:4], records, np.full(4, len(records), np.uint32))
    with pytest.raises(ValueError, match="one entry per case"):
        p.api.cutout_batch(given, quads[:4], None, rays, t[:3], records, material[:4])
    bad = records.copy()
    bad["image"][1] = len(table)
    with pytest.raises(p.capi.RtError, match="the table has no entry"):
        p.api.cutout_batch(given, quads[:4], None, rays, t[:4], bad, material[:4])
    bad = records.copy()
    bad["cutoff"][1] = 1.5
    with pytest.raises(p.capi.RtError, match="cutoff must be finite"):
        p.api.cutout_batch(given, quads[:4], None, rays, t[:4], bad, material[:4])


def test_the_rule_in_float64(p):
    """(u, v) and the decision against _uv_twin.tri_uv64 and _tex_twin.value64, which share no float32 code with the kernel, away from texel and cutoff
    boundaries.  fp32 evaluates the coordinates from a point with ~1e-6 of relative error on surfaces of size ~1 at distances ~10, and the texture coordinates
    span at most 4: 1e-4 is a generous bound for |(u, v) - (u, v)64|.  Under a bilinear mask of W x H <= 9 x 9 texels a coordinate error e moves the value by at
    most 2 * 9 * e, so a decision is compared only where |value64 - cutoff| > 0.01 — nearly everywhere."""
    table, records = CW.case_table(), CW.case_records()
    given = p.api.texture_table(table)
    checked = 0
    for (name, quads, uv, rays, t, material), image in zip(CW.batches(), (2, 2, 5)):
        rec = records[(records["on"] != 0) & (records["image"] == image)]
        material = np.arange(len(t)) % len(rec)
        keep, tuv, value = p.api.cutout_batch(given, quads, uv, rays, t, rec, material.astype(np.uint32))
        coords = np.broadcast_to(np.array([[0, 0], [1, 0], [0, 1]], np.float64), (len(t), 3, 2)) if uv is None else uv.astype(np.float64)
        keep64, tuv64, value64 = CT.keeps64(table[image][0], table[image][1], quads["Q"], quads["u"], quads["v"], coords[:, 0], coords[:, 1], coords[:, 2],
                                            rays[:, 0:3], rays[:, 3:6], t, rec["cutoff"][material])
        assert np.abs(tuv - tuv64).max() < 1e-4, np.abs(tuv - tuv64).max()
        assert np.abs(value - value64).max() < 2 * 9 * 1e-4
        clear = np.abs(value64 - rec["cutoff"][material]) > 0.01
        assert clear.mean() > 0.8 and ((keep != 0) == keep64)[clear].all()
        checked += int(clear.sum())
    assert checked > 3000


# ---- 2. the scene's bookkeeping ------------------------------------------------------------------------------------------------------------------------------------
def test_the_records_travel_through_builders_list_later_materials_and_clear(p):
    s = p.Scene()
    mats = dict(lam=s.Lambertian((0.5, 0.5, 0.5)), metal=s.Metal((0.8, 0.8, 0.8), 0.1), glass=s.Dielectric((1, 1, 1), 1.5), light=s.DiffuseLight((4, 4, 4)),
                fog=s.Isotropic((0.5, 0.5, 0.5), 0.3), solid=s.Dielectric((1, 1, 1), 1.5), checker=s.LambertianTexture((0, 0, 0), (1, 1, 1), 1.0))
    image = s.add_image(CW.grey([[0, 255]]))
    assert s.cutouts() is None
    s.set_interior(mats["solid"])
    for name, args, why in (("light", (image, 0.5), "whole area as emitting"), ("fog", (image, 0.5), "is a medium"), ("solid", (image, 0.5), "a holed solid has no inside"),
                            ("lam", (256, 0.5), "image index"), ("lam", (image, -0.1), "cutoff"), ("lam", (image, 1.01), "cutoff"), ("lam", (image, np.nan), "cutoff"),
                            ("lam", (image, np.inf), "cutoff")):
        with pytest.raises(p.capi.RtError, match=why) as e:
            s.set_cutout(mats[name], *args)
        assert e.value.code == 1 and s.cutouts() is None
    with pytest.raises(p.capi.RtError, match="no material 7"):
        s.set_cutout(7, image)
    s.set_cutout(mats["lam"], image).set_cutout(mats["metal"], image, 0.25).set_cutout(mats["glass"], image, 1.0).set_cutout(mats["checker"], 0, 0.0)
    with pytest.raises(p.capi.RtError, match="a holed solid has no inside"):   # ... and from the other side, a refusal on new ground only
        s.set_interior(mats["glass"])
    table = s.cutouts()
    assert table.dtype == p.capi.CUTOUT_DT and len(table) == 7 and list(table["on"]) == [1, 1, 1, 0, 0, 0, 1]
    assert table[mats["metal"]].tolist() == (1, image, 0.25, 0) and table[mats["lam"]]["cutoff"] == 0.5 and table[mats["checker"]].tolist() == (1, 0, 0.0, 0)
    before = table.tobytes()
    s.MakeQuad((0, 0, 0), (1, 0, 0), (0, 1, 0), mats["lam"])
    s.MakeSphere((0, 1, 0), 1.0, mats["glass"])
    for build in (s.BuildBVH_TopDown, s.BuildBVH_SAH, s.BuildBVH_BottomUp, s.MakeHittableList):
        build()
        assert s.cutouts().tobytes() == before
        w = s.getWorldPtr()
        assert w.cutouts.tobytes() == before and w.textures is not None and w.interiors is not None   # the table of the masks travels with the records
    later = s.Lambertian((1, 1, 1))   # a material added later: the table grows by an off record
    s.BuildBVH_SAH()
    assert s.cutouts()[:7].tobytes() == before and len(s.cutouts()) == 8 and s.cutouts()[later]["on"] == 0
    s.clear_cutout(mats["lam"]).clear_cutout(mats["light"])
    assert (s.cutouts()["on"] != 0).sum() == 3 and s.cutouts()[mats["lam"]].tolist() == (0, 0, 0.0, 0)
    s.clear_cutout(mats["metal"]).clear_cutout(mats["glass"]).clear_cutout(mats["checker"])
    assert s.cutouts() is None and not hasattr(s.getWorldPtr(), "cutouts")
    s.set_interior(mats["glass"])   # with the cutout gone the glass takes its inside


def test_both_languages_mirror_the_surface(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("rt_scene_set_cutout", "rt_scene_clear_cutout", "rt_scene_cutouts", "rt_cutout_batch", "rt_probe_cutout", "rt_renderer_cutouts",
                 "rt_renderer_cutouts_info", "rt_renderer_kernel_cutout", "rt_multi_renderer_cutouts", "rt_multi_renderer_cutouts_info"):
        assert name in header and name in p.capi.SYMBOLS and hasattr(p.lib(), name)
    for name in ("SetCutout(", "ClearCutout(", "Cutouts(", "SetCutouts("):
        assert name in hpp
    for name in ("set_cutout", "clear_cutout", "cutouts"):
        assert hasattr(p.Scene, name)
    for name in ("cutouts", "cutouts_info", "kernel_cutout"):
        assert hasattr(p.Renderer, name)
    assert hasattr(p.MultiRenderer, "cutouts") and hasattr(p.api, "cutout_batch") and hasattr(p.api, "probe_cutout")
    L, out = p.lib(), (C.c_uint32 * 2)()
    assert L.rt_renderer_cutouts(None, None, 0) != 0 and b"rt_renderer_cutouts" in L.rt_last_error()   # null handles are refused before any device is touched
    assert L.rt_renderer_cutouts_info(None, out) != 0 and L.rt_renderer_kernel_cutout(None, out) != 0 and L.rt_multi_renderer_cutouts(None, None, 0) != 0
    assert (p.capi.CUTOUT_OFF, p.capi.CUTOUT_MASKED) == (CT.OFF, CT.MASKED) and p.capi.CUTOUT_DT == CT.CUTOUT_DT and p.capi.CUTOUT_DT.itemsize == 16
    rule = header[header.index("alpha cutouts (DESIGN.md §34"):]
    for line in ("hit_p = o + d t", "tri_uv of the triangle's rt_tri_uvs record", "c = texture_value(entry[image], u, v)", "kept iff !(c.green < cutoff)"):
        assert line in rule, line   # the rule, stated line by line
    fields = header[header.index("int rt_renderer_kernel_form("):]
    assert "cutout" not in fields[:fields.index(";")]   # the query of its own: rt_renderer_kernel_form keeps its fields


def test_form_list_is_the_set_of_instantiations_and_the_older_counts_stand():
    """every form of stream_kernel_for()'s CUTOUT and CUTOUT_ENV_TREE families has a recipe in the list the GPU tests run, and nothing else has"""
    import _tri_worlds as TW
    for family in ("CUTOUT", "CUTOUT_ENV_TREE"):
        shipped = KT.family(family)
        assert len(shipped) == KT.count(family) == 8 and shipped == set(CW.FORMS) == set(IW.FORMS), shipped ^ set(CW.FORMS)
    assert all(CW.FORMS[f] == TW.FORMS[f] for f in CW.FORMS)
    for family, count in (("NEE", 16), ("TRI", 16), ("TRI_NEE", 16), ("LIGHT_TREE", 16), ("ENV_LIGHT", 8), ("ENV_TREE", 8), ("NORMAL_MAP", 8), ("NORMAL_MAP_ENV_TREE", 8),
                          ("MICROFACET", 8), ("MICROFACET_ENV_TREE", 8), ("INTERIOR", 8), ("INTERIOR_ENV_TREE", 8)):
        assert KT.count(family) == count, family   # nothing existing moved
    kernel = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_stream_kernel.hpp")).read()
    assert "static_assert(!CUT || INTR" in kernel and "bool CUT = false, bool INTR = false, bool MFAC = false, bool NMAP = false>" in kernel
    leaf, shade = kernel[kernel.index("phase 2: leaves"):kernel.index("phase 3: shade")], kernel[kernel.index("phase 3: shade"):]
    assert "if constexpr (CUT)" in leaf and "cutout_keeps(" in leaf and "cutout_keeps(" not in shade and "CUT" not in shade   # the rule lives in the leaf phase alone
    funcs = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_device_funcs.hpp")).read()
    probes = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_probes.hip")).read()
    assert funcs.count("RT_HD bool cutout_keeps(") == 1 and probes.count("cutout_keeps(") == 1   # one function: the kernel, the host batch and the probe call it


# ---- 3. assets -----------------------------------------------------------------------------------------------------------------------------------------------------
MTL = """newmtl leaf
Kd 0.2 0.6 0.2
map_Kd leaf.png
map_d -imfchan m masks/leaf_alpha.png
newmtl fence
map_d fence.png   # the last name counts
map_d  -s 2 2 1 other\\\\fence2.png
newmtl solid
d 0.5
"""


def test_load_mtl_reads_map_d(p, tmp_path):
    (tmp_path / "m.mtl").write_text(MTL)
    mats = p.mesh_io.load_mtl(str(tmp_path / "m.mtl"))
    assert mats["leaf"]["cutout_map"] == str(tmp_path / "masks" / "leaf_alpha.png") and mats["leaf"]["map_Kd"] == str(tmp_path / "leaf.png")
    assert mats["fence"]["cutout_map"] == str(tmp_path / "other" / "fence2.png")
    assert "cutout_map" not in mats["solid"] and mats["solid"]["dissolve"] == 0.5   # the key is present only when the file has the keyword
    for text, why in (("map_d a.png\n", "before any newmtl"), ("newmtl x\nmap_d\n", "needs a file name")):
        (tmp_path / "bad.mtl").write_text(text)
        with pytest.raises(ValueError, match=why):
            p.mesh_io.load_mtl(str(tmp_path / "bad.mtl"))


def write_png(path, pixels, filters=None):
    """an 8-bit RGB or RGBA PNG of pixels [H][W][3 or 4], scanline y under filter type filters[y] (0: none, 1: sub, 2: up)"""
    h, w, bpp = pixels.shape
    raw, prev = b"", np.zeros(w * bpp, np.int64)
    for y in range(h):
        line = pixels[y].reshape(-1).astype(np.int64)
        kind = 0 if filters is None else filters[y]
        left = np.concatenate([np.zeros(bpp, np.int64), line[:-bpp]])
        coded = line if kind == 0 else ((line - left) & 255 if kind == 1 else (line - prev) & 255)
        raw += bytes([kind]) + coded.astype(np.uint8).tobytes()
        prev = line

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if bpp == 3 else 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_read_png_alpha(p, tmp_path):
    rng = np.random.default_rng(34)
    rgba = rng.integers(0, 256, (5, 7, 4)).astype(np.uint8)
    for name, filters in (("plain.png", None), ("filtered.png", [1, 2, 0, 2, 1])):
        write_png(str(tmp_path / name), rgba, filters)
        alpha = p.image_io.read_png_alpha(str(tmp_path / name))
        assert alpha.dtype == np.uint8 and alpha.shape == (5, 7) and (alpha == rgba[:, :, 3]).all()
        assert (p.image_io.read_png(str(tmp_path / name)) == rgba[:, :, :3]).all()   # read_png is what it was: alpha dropped
    write_png(str(tmp_path / "rgb.png"), rgba[:, :, :3])
    assert p.image_io.read_png_alpha(str(tmp_path / "rgb.png")) is None and (p.image_io.read_png(str(tmp_path / "rgb.png")) == rgba[:, :, :3]).all()
    (tmp_path / "not.png").write_bytes(b"P6 1 1 255 abc")
    with pytest.raises(ValueError, match="not a PNG"):
        p.image_io.read_png_alpha(str(tmp_path / "not.png"))


def test_lattice_mask(p):
    m = p.image_io.lattice_mask(32, 16, 4, 2, 0.25)
    assert m.dtype == np.uint8 and m.shape == (16, 32, 3) and set(np.unique(m)) == {0, 255} and (m[:, :, 0] == m[:, :, 1]).all() and (m[:, :, 1] == m[:, :, 2]).all()
    on = m[:, :, 0] == 255
    columns, rows = on.all(axis=0), on.all(axis=1)
    assert columns.sum() == 4 * 2 and rows.sum() == 2 * 2   # four bars of two texels, two bars of two texels
    assert (np.diff(np.nonzero(columns)[0][::2]) == 8).all() and (on == (columns[None, :] | rows[:, None])).all()
    assert not p.image_io.lattice_mask(8, 8, 3, 3, 0.0).any() and (p.image_io.lattice_mask(8, 8, 3, 3, 1.0) == 255).all()
    assert not p.image_io.lattice_mask(8, 8, 0, 0, 0.5).any()
    assert (p.image_io.lattice_mask(5, 3, 2, 1, 0.5) == p.image_io.lattice_mask(5, 3, 2, 1, 0.5)).all()
    for bad in ((0, 4, 1, 1, 0.5), (4, 4, -1, 1, 0.5), (4, 4, 1, 1, 1.5)):
        with pytest.raises(ValueError, match="lattice_mask"):
            p.image_io.lattice_mask(*bad)


# ---- 4. the room ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_the_room_follows_every_sample_and_meets_every_case(env, as_list):
    """the room the GPU tests render is not vacuous: the twin follows every sample, and the rule turns down at least 100 candidates of each kind"""
    run = CW.run(env, as_list)
    assert run.followed.all() and run.off_followed.all() and np.isfinite(run.samples).all()
    for key in ("rejected_quad", "rejected_tri_uv", "rejected_tri_plain", "rejected_deep", "then_farther", "then_miss"):
        assert run.stats[key] >= 100, (key, run.stats)
    assert run.stats["kept"] >= 100 and run.stats["tested"] == run.stats["kept"] + run.stats["rejected"]
    assert (run.sums.view(np.uint32) != run.off_sums.view(np.uint32)).any(axis=2).sum() > 100   # the holes are seen


@pytest.mark.parametrize("env", [False, True], ids=["plain", "mode48"])
def test_the_room_with_every_kind_of_record_live(env):
    """masked cards beside a solid-glass box with an interior record, a rough conductor and a coated card that is masked too: the one loop of _path_twin follows
    every sample with the cutout walk as its trace, the rule still turns down 100 candidates of each kind, and the two roads to the facing agree — the loop's
    `interiors` argument with every sigma zero, and _interior_twin.solid_walk wrapped around the cutout walk — bit for bit"""
    run, plain = CW.run(env, live=True), CW.run(env)
    assert run.followed.all() and run.off_followed.all() and run.facing_followed.all() and np.isfinite(run.samples).all()
    assert (run.scene.interiors()["on"] != 0).sum() == 1 and (run.scene.microfacets()["on"] != 0).sum() == 2 and (run.cutouts["on"] != 0).sum() == CW.RECORDS
    assert run.scene.microfacets()[run.scene.names["card"]]["on"] != 0 and run.cutouts[run.scene.names["card"]]["on"] != 0   # one material, both records
    for key in ("rejected_quad", "rejected_tri_uv", "rejected_tri_plain", "rejected_deep", "then_farther", "then_miss"):
        assert run.stats[key] >= 100, (key, run.stats)
    untinted, followed = CW.twin_frame(run.scene, run.cutouts, env, interiors=IW.no_tint(run.scene.interiors()))
    assert followed.all() and bits_equal(VT_sums(untinted), run.facing_sums), mismatch_report(VT_sums(untinted), run.facing_sums)
    assert not bits_equal(run.facing_sums, run.sums)        # the tint is seen
    assert not bits_equal(run.sums, run.off_sums)           # ... and so are the holes
    assert (run.sums.view(np.uint32) != plain.sums.view(np.uint32)).any(axis=2).sum() > 50   # ... and the other records


def test_the_walk_without_a_record_is_the_walk(p):
    """with every record off, and with an opaque mask on every material, the walk of its own returns what _tri_twin's returns: the copy of the loops is a copy"""
    run = CW.run(False)
    off = np.zeros(len(run.cutouts), CT.CUTOUT_DT)
    samples, followed = CW.twin_frame(run.scene, off, False)
    assert followed.all() and bits_equal(VT_sums(samples), run.off_sums)
    stats = CT.new_stats()
    opaque = CW.all_of(p, run.scene, run.scene.names["images"]["white"])
    samples, followed = CW.twin_frame(run.scene, opaque, False, stats=stats)
    assert followed.all() and bits_equal(VT_sums(samples), run.off_sums) and stats["tested"] > 1000 and stats["rejected"] == 0


def VT_sums(samples):
    import _env_tree_twin as VT
    return VT.in_order_sums(samples)
