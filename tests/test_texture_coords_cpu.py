"""Texture coordinates without a GPU: the rule's numpy twin against the kernels' own function on the host, the mathematics no kernel shares,
texel selection, the host plumbing that carries the records, the file readers, the ABI programs and the list of kernel forms."""
import os
import re
import subprocess

import numpy as np
import pytest

import _tri_worlds as TW
import _uv_twin as UT
import _uv_worlds as UW
import _kernel_table as KT
from _common import ROOT, as_oracle_world, bits_equal, mismatch_report, pkg

F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden")
# item 2: the largest |float32 twin - float64 restatement| of an affine coordinate function over the hits below, measured on the CPU with
# coordinates of magnitude <= 2: 1.253e-7 over the 9967 hits of icosphere(1..3), 2.205e-7 over 2000 random triangles (about two ulps of 1: the planar
# coordinates carry the rounding of hit_p and of w).  The bound is 4 x the larger one; DESIGN.md §22 records both.
AFFINE_MEASURED = 2.205e-7
AFFINE_BOUND = 4 * AFFINE_MEASURED


@pytest.fixture(scope="module")
def p():
    return pkg()


def random_hits(p, n, seed):
    """n random triangles, a record each from [-0.25, 1.25), and a ray at a random point of each (some a little outside it) -> tris, uv, rays (n, 6), t"""
    rng = np.random.default_rng(seed)
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    pts = []
    while len(pts) < n:
        a, e1, e2 = (rng.standard_normal(3) * 2).astype(F), (rng.standard_normal(3) * 1.5).astype(F), (rng.standard_normal(3) * 1.5).astype(F)
        try:
            s.MakeTriangle(a, a + e1, a + e2, m)
        except Exception as e:
            if "degenerate triangle" not in str(e):
                raise
            continue
        pts.append((a, e1, e2))
    s.MakeHittableList()
    tris = s.quads()
    assert len(tris) == n
    ab = rng.random((n, 2)) * 1.1 - 0.05
    ab[ab.sum(axis=1) > 1.05] *= 0.5
    target = tris["Q"].astype(np.float64) + tris["u"].astype(np.float64) * ab[:, :1] + tris["v"].astype(np.float64) * ab[:, 1:]
    origin = target + tris["normal"].astype(np.float64) * rng.uniform(0.5, 4.0, (n, 1)) + rng.standard_normal((n, 3)) * 0.3
    rays = np.zeros((n, 6), F)
    rays[:, 0:3] = origin.astype(F)
    rays[:, 3:6] = (target - rays[:, 0:3].astype(np.float64)).astype(F)
    return tris, UW.random_uvs(3 * n, seed=seed + 1).reshape(n, 3, 2), rays, np.ones(n, F)


# ---- 1. the rule's twin --------------------------------------------------------------------------------------------------------------------------------
def test_host_batch_equals_the_twin_on_random_hits(p):
    tris, uv, rays, t = random_hits(p, 4096, seed=3)
    got = p.api.tri_uv_batch(tris, uv, rays, t)
    want = UT.tri_uv(tris, uv, rays[:, 0:3], rays[:, 3:6], t)
    assert bits_equal(got, want), mismatch_report(got, want)
    assert (got < 0).any() and (got > 1).any()   # before the clamp


def test_host_batch_equals_the_twin_on_crafted_hits(p):
    names, tris, uv, rays, t = UW.crafted_arrays(p)
    got = p.api.tri_uv_batch(tris, uv, rays, t)
    want = UT.tri_uv(tris, uv, rays[:, 0:3], rays[:, 3:6], t)
    assert bits_equal(got, want), mismatch_report(got, want)
    by_name = dict(zip(names, got))
    for vertex, k in (("vertex a", 0), ("vertex b", 1), ("vertex c", 2)):   # at a vertex the record's own value, exactly (the triangle's sides are powers of two)
        assert tuple(by_name[f"general: {vertex}"]) == UW.GENERAL[k]
        assert tuple(by_name[f"below 0 and above 1: {vertex}"]) == UW.WIDE[k]
    assert tuple(by_name["exactly 0.0 and 1.0: vertex a"]) == (0.0, 0.0) and tuple(by_name["exactly 0.0 and 1.0: vertex c"]) == (1.0, 1.0)
    assert all(tuple(by_name[f"three equal: {pn}"]) == UW.EQUAL[0] for pn, _ in UW.POINTS)
    assert tuple(by_name["general: midpoint ab"]) == (0.5, 0.3125)
    assert tuple(by_name["identity: alpha + beta == 1"]) == (0.25, 0.75)


# ---- 2. mathematics no kernel shares ---------------------------------------------------------------------------------------------------------------------
def affine_hits(p):
    """hits on icosphere(1..3) (scaled by 1.5) from outside, and on random triangles: (tris, rays, t) with t from the twin's own walk where a world is walked"""
    out = []
    for level in (1, 2, 3):
        s, rays, _ = TW.closed_mesh_world(p, as_list=False, level=level)
        world = as_oracle_world(s.getWorldPtr())
        hit, t, prim, _ = UT.TT.closest_intersection(world, rays)
        keep = hit != 0
        out.append((s.quads()[prim[keep]], rays[keep, 0:6], t[keep]))
    tris, _, rays, t = random_hits(p, 2000, seed=9)
    out.append((tris, rays, t))
    return out


def test_affine_coordinates_interpolate_to_the_affine_function_of_the_hit_point(p):
    A = np.array([[0.21, -0.13, 0.08], [0.05, 0.17, -0.22]])
    c = np.array([0.4, 0.55])
    worst32 = worst64 = 0.0
    for tris, rays, t in affine_hits(p):
        Q, u, v = (tris[k].astype(np.float64) for k in ("Q", "u", "v"))
        t0, t1, t2 = Q @ A.T + c, (Q + u) @ A.T + c, (Q + v) @ A.T + c
        hit_p = rays[:, 0:3].astype(np.float64) + rays[:, 3:6].astype(np.float64) * t[:, None].astype(np.float64)
        unit = np.cross(u, v)
        unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        on_plane = hit_p - unit * ((hit_p - Q) * unit).sum(axis=1, keepdims=True)   # the function is judged on the plane (its normal in float64, from u and v)
        want = on_plane @ A.T + c
        got64 = UT.tri_uv64(Q, u, v, t0, t1, t2, on_plane)
        worst64 = max(worst64, float(np.abs(got64 - want).max()))
        rec = np.stack([t0, t1, t2], axis=1).astype(F)
        got32 = UT.tri_uv(tris, rec, rays[:, 0:3], rays[:, 3:6], t)
        worst32 = max(worst32, float(np.abs(got32.astype(np.float64) - want).max()))
        print(f"affine: {len(tris)} hits: float32 twin off by at most {float(np.abs(got32.astype(np.float64) - want).max()):.3e}")
    print(f"affine: float64 {worst64:.3e}, float32 twin {worst32:.3e} (bound {AFFINE_BOUND:.3e})")
    assert worst64 < 1e-12
    assert worst32 < AFFINE_BOUND


# ---- 3. texel selection ------------------------------------------------------------------------------------------------------------------------------------
def test_texel_selection_clamps_flips_and_takes_the_last_column_at_one():
    for w, h in ((1, 1), (5, 3)):
        assert UT.texel_index(w, h, F(1.0), F(0.5))[0] == w - 1            # u == 1.0: column W - 1, not W
        assert UT.texel_index(w, h, F(0.0), F(0.0)) == (0, h - 1)          # v is flipped: v = 0 is the bottom row
        assert UT.texel_index(w, h, F(0.0), F(1.0)) == (0, 0)
        assert UT.texel_index(w, h, F(-3.0), F(7.0)) == (0, 0) and UT.texel_index(w, h, F(9.0), F(-1.0)) == (w - 1, h - 1)
        assert UT.texel_index(w, h, F(-0.0), F(-0.0)) == UT.texel_index(w, h, F(0.0), F(0.0))
    img = UW.pair_image()
    assert UT.texel_index(5, 3, F(0.39999), F(0.5)) == (1, 1) and UT.texel_index(5, 3, F(0.4), F(0.5))[0] == 2
    assert bits_equal(UT.texel(img, F([0.5]), F([0.5]))[0], img[1, 2].astype(F) * UW.ALBEDO_SCALE)


def test_identity_record_selects_the_planar_lookups_texel_on_every_hit(p):
    tris, uv, rays, t = random_hits(p, 4096, seed=3)
    names, ctris, _, crays, ct = UW.crafted_arrays(p)
    tris, rays, t = np.concatenate([tris, ctris]), np.concatenate([rays, crays]), np.concatenate([t, ct])
    ident = np.broadcast_to(UT.IDENTITY, (len(tris), 3, 2))
    tuv = p.api.tri_uv_batch(tris, ident, rays, t)
    alpha, beta = UT.planar(tris, rays[:, 0:3], rays[:, 3:6], t)
    assert ((alpha == 0) | (beta == 0)).any()                                   # hits where a planar coordinate is +-0 are among them
    assert np.array_equal(tuv[:, 0], alpha) and np.array_equal(tuv[:, 1], beta)   # equal as numbers: the same up to the sign of a zero
    for w, h in ((1, 1), (5, 3), (4, 4)):
        assert all(np.array_equal(a, b) for a, b in zip(UT.texel_index(w, h, tuv[:, 0], tuv[:, 1]), UT.texel_index(w, h, alpha, beta)))


def test_constant_faces_land_in_their_texel_on_every_hit_of_the_room(p):
    """item 10's premise: under three equal coordinates at a texel centre every hit of the palette mesh selects that texel"""
    scene = UW.palette_room(p)
    world = as_oracle_world(scene.getWorldPtr())
    uv = scene.texture_coords()
    assert len(uv) == scene.n_triangles()
    rays = TW.room_rays(4000, seed=5)
    rays[2000:, 3:6] = (F([5, 5.2, 6.5]) + (np.random.default_rng(1).random((2000, 3), dtype=F) - F(0.5)) * F(2.4)) - rays[2000:, 0:3]
    hit, t, prim, tuv = UT.closest_intersection_uv(world, uv, rays)
    tab = UT.table(uv)
    first_tri = world.n_prims + world.n_quads - len(tab)
    const = np.nonzero((tab[:, 0] == tab[:, 1]).all(axis=1) & (tab[:, 0] == tab[:, 2]).all(axis=1))[0]
    assert len(const) == 20
    rows = np.nonzero((hit != 0) & np.isin(prim - first_tri, const))[0]
    assert len(rows) > 300
    want_col, want_row = UT.texel_index(4, 4, tab[prim[rows] - first_tri, 0, 0], tab[prim[rows] - first_tri, 0, 1])
    got_col, got_row = UT.texel_index(4, 4, tuv[rows, 0], tuv[rows, 1])
    assert np.array_equal(got_col, want_col) and np.array_equal(got_row, want_row)
    assert np.abs(tuv[rows] - tab[prim[rows] - first_tri, 0]).max() < 1e-5   # a texel centre is 0.125 from a boundary


# ---- 4. host plumbing ------------------------------------------------------------------------------------------------------------------------------------
def tagged_scene(p):
    """triangles added one by one and as a mesh, every one with a record of its own; returns (scene, {bytes of (Q, u, v): record (3, 2)})"""
    s = p.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    rng = np.random.default_rng(12)
    s.MakeSphere((0, 0, 0), 0.5, m)
    s.MakeQuad((-4, -1, -4), (8, 0, 0), (0, 0, 8), m)
    for k in range(9):
        a = (rng.standard_normal(3) * 3).astype(F)
        kw = {"uvs": rng.random((3, 2), dtype=F)} if k % 3 else {}
        if k % 2:
            kw["normals"] = rng.standard_normal((3, 3)).astype(F)
        s.MakeTriangle(a, a + F([1, 0, 0.2]), a + F([0, 1, 0.3]), m, **kw)
    v, f = TW.mesh_io().icosphere(1)
    s.MakeMesh(v, f, m, 1.2, 30.0, (1, 2, 1), uvs=rng.random((len(f) * 3, 2), dtype=F), uv_faces=np.arange(len(f) * 3).reshape(-1, 3))
    s.MakeHittableList()
    quads, tab = s.quads(), UT.table(s.texture_coords())
    tris = quads[quads["kind"] == 1]
    assert len(tab) == len(tris) == 89
    return s, {tris[i][["Q", "u", "v"]].tobytes(): tab[i].copy() for i in range(len(tris))}


@pytest.mark.parametrize("build", ["MakeHittableList", "BuildBVH_TopDown", "BuildBVH_SAH", "BuildBVH_BottomUp"])
def test_records_follow_their_triangles(p, build):
    s, by_record = tagged_scene(p)
    assert sum((r != UT.IDENTITY).any() for r in by_record.values()) == 86   # three of the free triangles were given none
    getattr(s, build)()
    s.MakeQuad((-4, 5, -4), (8, 0, 0), (0, 0, 8), s.Lambertian((0.1, 0.1, 0.1)))   # a parallelogram added afterwards goes in front of the triangles
    getattr(s, build)()
    quads, tab, vn = s.quads(), UT.table(s.texture_coords()), s.vertex_normals()
    tris = quads[quads["kind"] == 1]
    assert len(tab) == len(tris) == len(vn) == 89 and (quads["kind"][:2] == 0).all()
    for i in range(len(tris)):
        assert bits_equal(tab[i], by_record[tris[i][["Q", "u", "v"]].tobytes()]), i


def test_all_identity_scenes_report_no_table(p):
    s = TW.tri_room(p, textured=True)
    assert len(s.texture_coords()) == 0 and not hasattr(s.getWorldPtr(), "texture_coords")
    s2 = p.Scene()
    m = s2.Lambertian((0.5, 0.5, 0.5))
    s2.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m, uvs=UT.IDENTITY)   # given, but the identity
    s2.MakeHittableList()
    assert len(s2.texture_coords()) == 0
    s2.MakeTriangle((0, 0, 1), (1, 0, 1), (0, 1, 1), m, uvs=((0, 0), (1, 0), (0, 0.5)))
    s2.MakeHittableList()
    tab = UT.table(s2.texture_coords())
    assert len(tab) == 2 and bits_equal(tab[0], UT.IDENTITY) and bits_equal(tab[1], F([[0, 0], [1, 0], [0, 0.5]]))
    assert len(s2.getWorldPtr().texture_coords) == 2


def test_a_failed_add_leaves_the_scene_unchanged(p):
    s, _ = tagged_scene(p)
    m = s.Lambertian((0.5, 0.5, 0.5))
    s.MakeHittableList()
    before = TW.flat_bytes(s), s.texture_coords().tobytes(), s.vertex_normals().tobytes()
    v, f = TW.mesh_io().tetrahedron()
    good = np.random.default_rng(1).random((len(v), 2), dtype=F)
    bad = good.copy()
    bad[2, 1] = np.nan
    with pytest.raises(Exception, match="not finite"):
        s.MakeMesh(v, f, m, uvs=bad)
    with pytest.raises(Exception, match="out of range"):
        s.MakeMesh(v, f, m, uvs=good[:3])                               # the vertex indices reach 3
    with pytest.raises(Exception, match="out of range"):
        s.MakeMesh(v, f, m, uvs=good, uv_faces=np.full_like(f, 4))
    with pytest.raises(Exception, match="not finite"):
        s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m, uvs=((0, 0), (np.inf, 0), (0, 1)))
    with pytest.raises(Exception, match="normal"):
        s.MakeTriangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m, uvs=UT.IDENTITY, normals=np.zeros((3, 3)))
    assert (TW.flat_bytes(s), s.texture_coords().tobytes(), s.vertex_normals().tobytes()) == before


def test_mesh_without_uv_faces_uses_the_vertex_indices(p):
    v, f = TW.mesh_io().tetrahedron()
    t = np.random.default_rng(4).random((len(v), 2), dtype=F)
    s = p.Scene()
    s.MakeMesh(v, f, s.Lambertian((0.5, 0.5, 0.5)), uvs=t)
    s.MakeHittableList()
    assert bits_equal(UT.table(s.texture_coords()), t[f.astype(np.int64)])
    assert len(s.vertex_normals()) == 0   # texture coordinates alone bring no normals


# ---- 5. file readers ---------------------------------------------------------------------------------------------------------------------------------------
def test_load_obj_uvs_reads_the_cube_fixture(p):
    m = TW.mesh_io()
    v, f, t, tf = m.load_obj_uvs(os.path.join(GOLDEN, "uv_cube.obj"))
    assert v.shape == (8, 3) and f.shape == (12, 3) and t.shape == (14, 2) and tf.shape == (12, 3)
    v0, f0 = m.load_obj(os.path.join(GOLDEN, "uv_cube.obj"))
    assert np.array_equal(v, v0) and np.array_equal(f, f0)
    assert t.min() == 0.0 and t.max() == 1.0 and tf.max() == 13
    # the atlas: every face of the cube is a 0.25 x 0.25 square of it, so each triangle's coordinates span a right triangle of legs 0.25
    e1, e2 = t[tf[:, 1]] - t[tf[:, 0]], t[tf[:, 2]] - t[tf[:, 0]]
    assert np.allclose(np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 0.0625)
    assert m.load_obj_uvs(os.path.join(GOLDEN, "uv_cube_incomplete.obj"))[2:] == (None, None)
    assert m.load_obj_uvs(os.path.join(GOLDEN, "uv_cube_incomplete.obj"))[1].shape == (12, 3)


def test_load_obj_uvs_negative_indices_polygons_and_forms(p, tmp_path):
    m = TW.mesh_io()
    path = tmp_path / "fan.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 1.5 0\nvt 0 0\nvt 1 0 0\nvt 1 1\nvt 0 1\nvt 0.5 1.5\nvn 0 0 1\n"
                    "f 1/1 2/2 3/3 4/4 5/5   # a polygon, v/vt\nf -5/-5/1 -4/-4/1 -3/-3/-1  # negative, v/vt/vn\n")
    v, f, t, tf = m.load_obj_uvs(str(path))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2]] and tf.tolist() == f.tolist()
    assert t.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 1.5]]
    (tmp_path / "none.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")
    assert m.load_obj_uvs(str(tmp_path / "none.obj"))[2:] == (None, None)
    (tmp_path / "bad.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/2 3/1\n")
    with pytest.raises(ValueError, match="out of range"):
        m.load_obj_uvs(str(tmp_path / "bad.obj"))


def test_image_readers_round_trip_the_writers_and_read_the_fixtures(p, tmp_path):
    from ray_tracing_v06_amd import image_io as io
    fb = np.random.default_rng(8).random((7, 11, 4), dtype=F)
    io.write_ppm(str(tmp_path / "a.ppm"), fb)
    io.write_png(str(tmp_path / "a.png"), fb)
    want = io.to_rgb8(fb)
    assert io.read_ppm(str(tmp_path / "a.ppm")).tobytes() == want.tobytes() and io.read_png(str(tmp_path / "a.png")).tobytes() == want.tobytes()
    a, b = io.read_ppm(os.path.join(GOLDEN, "uv_atlas_8x4.ppm")), io.read_png(os.path.join(GOLDEN, "uv_atlas_8x4.png"))
    assert a.shape == (4, 8, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert len(np.unique(a.reshape(-1, 3), axis=0)) == 32
    with pytest.raises(ValueError):
        io.read_png(os.path.join(GOLDEN, "uv_atlas_8x4.ppm"))
    with pytest.raises(ValueError):
        io.read_ppm(os.path.join(GOLDEN, "uv_atlas_8x4.png"))


def test_read_png_undoes_all_five_filter_types(p, tmp_path):
    """the committed PNG's four rows use filter types 1 to 4 (it was written by hand for that; write_png's files, read above, use type 0); an RGBA file
    written here uses all five"""
    import struct
    import zlib
    from ray_tracing_v06_amd import image_io as io
    raw = open(os.path.join(GOLDEN, "uv_atlas_8x4.png"), "rb").read()
    pos, idat = 8, b""
    while pos < len(raw):
        n, tag = struct.unpack(">I", raw[pos:pos + 4])[0], raw[pos + 4:pos + 8]
        if tag == b"IDAT":
            idat += raw[pos + 8:pos + 8 + n]
        pos += 12 + n
    lines = zlib.decompress(idat)
    assert sorted({lines[y * 25] for y in range(4)}) == [1, 2, 3, 4]   # 8 x 3 bytes + the filter byte per row
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 6, 4)).astype(np.uint8)

    def paeth(a, b, c):
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        return a if pa <= pb and pa <= pc else (b if pb <= pc else c)
    out = b""
    flat = img.reshape(5, 24).astype(int)
    for y in range(5):
        cur, prev = flat[y], flat[y - 1] if y else np.zeros(24, int)
        left = lambda x, r=cur: r[x - 4] if x >= 4 else 0
        pred = {0: lambda x: 0, 1: lambda x: left(x), 2: lambda x: prev[x], 3: lambda x: (left(x) + prev[x]) >> 1,
                4: lambda x: paeth(left(x), prev[x], left(x, prev))}[y]
        out += bytes([y]) + bytes((cur[x] - pred(x)) & 255 for x in range(24))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    path = tmp_path / "rgba.png"
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 5, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(out)) + chunk(b"IEND", b""))
    assert np.array_equal(io.read_png(str(path)), img[:, :, :3])


def test_uv_sphere(p):
    m = TW.mesh_io()
    for n_lon, n_lat in ((8, 4), (5, 3), (64, 32)):
        v, f, n, t = m.uv_sphere(n_lon, n_lat)
        assert len(v) == len(n) == len(t) == (n_lat + 1) * (n_lon + 1) and len(f) == 2 * n_lon * (n_lat - 1)
        assert t.min() == 0.0 and t.max() == 1.0
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
        grid = v.reshape(n_lat + 1, n_lon + 1, 3)
        assert np.abs(grid[:, 0] - grid[:, -1]).max() < 1e-6                      # the seam column is there twice,
        tg = t.reshape(n_lat + 1, n_lon + 1, 2)
        assert (tg[:, 0, 0] == 0).all() and (tg[:, -1, 0] == 1).all()             # once with u = 0 and once with u = 1
        tri = v[f.astype(np.int64)].astype(np.float64)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert (np.linalg.norm(nrm, axis=1) > 1e-6).all() and ((nrm * tri.mean(axis=1)).sum(axis=1) > 0).all()   # no degenerate face, all seen from outside
        assert (np.abs(t[f.astype(np.int64)][:, :, 0].max(axis=1) - t[f.astype(np.int64)][:, :, 0].min(axis=1)) <= 1.0 / n_lon + 1e-6).all()   # no face spans the seam
        # the convention of image_value (sphere::get_sphere_uv): u = (atan2(-z, x) + pi) / 2 pi, v = acos(-y) / pi, away from the poles and the seam
        inner = (t[:, 1] > 0) & (t[:, 1] < 1) & (t[:, 0] > 0) & (t[:, 0] < 1)
        x, y, z = n[inner].astype(np.float64).T
        assert np.abs((np.arctan2(-z, x) + np.pi) / (2 * np.pi) - t[inner, 0]).max() < 1e-6 and np.abs(np.arccos(-y) / np.pi - t[inner, 1]).max() < 1e-6


# ---- 6. ABI --------------------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_program(p):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])   # as the other ABI tests do: the check is built where it is missing
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_uv")])
    exe = os.path.join(ROOT, "tests", "cpp_uv", "uv_abi_check")
    assert os.path.exists(exe) and os.access(os.path.join(ROOT, "tests", "cpp_uv", "uv_app"), os.X_OK), "tests/cpp_uv compiles and links"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "uv ABI ok" in out.stdout, out.stdout + out.stderr


def test_symbols_and_mirrors(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    L = p.capi.lib()
    for name in ("rt_scene_add_triangle_uv", "rt_scene_add_mesh_uv", "rt_scene_texture_coords", "rt_tri_uv_batch", "rt_renderer_texture_coords",
                 "rt_renderer_texture_coords_info", "rt_multi_renderer_texture_coords", "rt_probe_tri_uv"):
        assert name in p.capi.SYMBOLS and re.search(r"\b" + name + r"\(", header), name
        assert getattr(L, name).argtypes, name
    assert p.capi.TRI_UVS_DT.itemsize == 24
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert "void SetTextureCoords(const rt_tri_uvs* table, uint32_t n)" in hpp and "rt_scene_add_mesh_uv" in hpp and "rt_scene_add_triangle_uv" in hpp
    assert callable(p.Renderer.texture_coords) and callable(p.Renderer.texture_coords_info) and callable(p.MultiRenderer.texture_coords)
    assert "--texture" in open(os.path.join(ROOT, "tools", "render.py")).read()


# ---- 7. kernel list ----------------------------------------------------------------------------------------------------------------------------------------
def test_stream_kernel_table_gains_no_instantiation():
    """the kernel forms held against rt_device.hip without a GPU are what they were: texture coordinates ride on a wave-uniform header, not on a
    template argument"""
    for family, n in (("NEE", 16), ("TRI", 16), ("TRI_NEE", 16), ("LIGHT_TREE", 16)):
        assert KT.count(family) == n, family
    kernel = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_stream_kernel.hpp")).read()
    head = kernel[kernel.index("template <"):kernel.index("render_kernel_stream(")]
    assert "UV" not in head.rsplit("template <", 1)[1]
    assert len(UW.EXT2_FORMS) == 8
