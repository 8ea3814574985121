"""Environment maps without a GPU: the rule's numpy twin against the kernels' own function on the host, the mathematics no kernel shares,
the scene plumbing, the Radiance file reader and writer, and the whole-sample twin pinned to the one it copies."""
import functools

import numpy as np
import pytest

import _env_twin as ET
import _env_worlds as EW
import _tri_twin as TT
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

F = np.float32


@pytest.fixture(scope="module")
def p():
    return pkg()


def image_io():
    pkg()
    from ray_tracing_v06_amd import image_io as m
    return m


# ---- 1. the rule's twin ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u0", EW.ROTATIONS, ids=EW.ROTATION_IDS)
@pytest.mark.parametrize("size", EW.SIZES, ids=[f"{w}x{h}" for w, h in EW.SIZES])
def test_host_batch_equals_the_twin(p, size, u0):
    w, h = size
    env = EW.random_map(w, h)
    dirs = EW.directions()
    rgb, texel = p.api.environment_batch(env, u0, dirs)
    want_rgb, want_texel = ET.lookup(env, u0, dirs)
    assert np.array_equal(texel, want_texel), f"{int((texel != want_texel).sum())} texel indices differ; first at {np.nonzero(texel != want_texel)[0][:3]}"
    assert bits_equal(rgb, want_rgb), mismatch_report(rgb, want_rgb)
    assert texel.max() < w * h
    assert len(np.unique(texel)) >= 0.95 * w * h   # (nearly) every texel is seen: the rows at the poles of the 64 x 32 map are thin


def test_the_crafted_directions_are_what_they_claim(p):
    names, crafted = EW.crafted_directions()
    by_name = dict(zip(names, crafted))
    w, h = 16, 8
    col = lambda name, u0=0.0: int(ET.texel_of(w, h, u0, by_name[name][None, :])[0]) % w
    row = lambda name: int(ET.texel_of(w, h, 0.0, by_name[name][None, :])[0]) // w
    assert row("+y") == 0 and row("-y") == h - 1   # row 0 is the top
    assert row("pole up, tiny x z") == 0 and row("pole down, tiny x z") == h - 1
    assert col("+x") == w // 2 and col("-z") == 3 * w // 4 and col("+z") == w // 4
    for name in ("seam z=+0", "seam z=-0", "seam z=+1e-30", "seam z=-1e-30"):   # on the seam phi is 0 or 2 pi, and u = 1 wraps to 0: the first column
        assert col(name) == 0, name
    for u0, tag in zip(EW.ROTATIONS, EW.ROTATION_IDS):   # the fans around u == 1: before the wrap some u are >= 1 and some below, by ulps
        fan = np.stack([d for n, d in zip(names, crafted) if n.startswith(f"fan {tag} ")])
        with np.errstate(all="ignore"):
            inv = F(1) / np.sqrt(ET.dot(fan, fan))
            n = fan * inv[:, None]
            raw = (ET._math(3, -n[:, 2], n[:, 0]) + ET.PI) / ET.TWO_PI + F(u0)
        near = np.abs(raw.astype(np.float64) - 1.0) <= 2.0 ** -23
        assert near.any() and (raw >= F(1)).any() and (raw < F(1)).any(), (tag, raw)
        cols = ET.texel_of(w, h, u0, fan) % w
        assert set(cols.tolist()) == {0, w - 1}, (tag, cols)
    nan = np.array([[np.nan, 1, 0], [0, 0, 0], [np.inf, 0, 0]], F)   # a NaN coordinate lands on texel 0 of its axis, on the host as in the twin
    env = EW.random_map(w, h)
    rgb, texel = p.api.environment_batch(env, 0.25, nan)
    want_rgb, want_texel = ET.lookup(env, 0.25, nan)
    assert np.array_equal(texel, want_texel) and bits_equal(rgb, want_rgb)
    assert texel[1] == (h - 1) * w   # all NaN: u = 0, v = 0 -> flipped to the last row, first column


# ---- 2. the rule against mathematics no kernel shares -----------------------------------------------------------------------------------------------------
def float64_coordinates(u0, dirs, w, h):
    d = dirs.astype(np.float64)
    n = d / np.linalg.norm(d, axis=1)[:, None]
    theta = np.arccos(np.clip(-n[:, 1], -1.0, 1.0))
    phi = np.arctan2(-n[:, 2], n[:, 0]) + np.pi
    u = np.mod(phi / (2.0 * np.pi) + float(u0), 1.0)
    v = 1.0 - theta / np.pi
    return u * w, v * h


@pytest.mark.parametrize("u0", EW.ROTATIONS, ids=EW.ROTATION_IDS)
def test_the_twin_picks_the_float64_texel_away_from_texel_borders(u0):
    w, h = 64, 32
    dirs = EW.random_directions(100000, seed=5)
    fi, fj = float64_coordinates(u0, dirs, w, h)
    # the pinned accuracy of rt_acosf / rt_atan2f is 5e-7 rad: under 2e-5 texels at W = 64, so 1e-3 texels from a border is a wide margin
    clear = (np.abs(fi - np.rint(fi)) >= 1e-3) & (np.abs(fj - np.rint(fj)) >= 1e-3)
    assert 1.0 - clear.mean() < 0.02, f"{1.0 - clear.mean():.4f} of the directions lie near a texel border"   # uniform coordinates: about 0.4 %
    want = (np.floor(fj).astype(np.int64) * w + np.floor(fi).astype(np.int64))[clear]
    got = ET.texel_of(w, h, u0, dirs)[clear].astype(np.int64)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {len(want)} differ"
    # the rotation: u0 turns the world about y by 360 u0 degrees
    a = 2.0 * np.pi * float(u0)
    d = dirs.astype(np.float64)
    turned = np.stack([d[:, 0] * np.cos(a) + d[:, 2] * np.sin(a), d[:, 1], -d[:, 0] * np.sin(a) + d[:, 2] * np.cos(a)], axis=1).astype(F)
    assert np.array_equal(ET.texel_of(w, h, 0.0, turned)[clear].astype(np.int64), got)


# ---- 3. scene plumbing --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", TW.BUILDERS)
def test_a_scene_carries_its_environment_through_every_builder(p, builder):
    env = EW.random_map(7, 3)
    s = p.Scene()
    s.MakeSphere((0, 0, -1), 0.5, s.Lambertian((0.5, 0.5, 0.5)))
    s.MakeSphere((1, 0, -2), 0.5, s.Metal((0.5, 0.5, 0.5), 0.1))
    assert s.environment() is None
    s.set_environment(env, rotate_y=90.0)
    getattr(s, builder)()
    w = s.getWorldPtr()
    assert w.background == 2
    got, u0 = s.environment()
    assert bits_equal(got, env) and got.shape == (3, 7, 3) and u0 == F(0.25)
    assert bits_equal(w.environment[0], env) and w.environment[1] == F(0.25)
    s.set_environment(env, rotate_y=-90.0)
    assert s.environment()[1] == F(0.75)
    s.set_environment(env, rotate_y=720.0)
    assert s.environment()[1] == F(0.0)
    s.set_background((0.1, 0.2, 0.3))   # a constant colour drops the map
    assert s.environment() is None and s.getWorldPtr().background == 1 and not hasattr(s.getWorldPtr(), "environment")
    s.set_environment(env)
    s.set_background(None)              # and so does the gradient
    assert s.environment() is None and s.getWorldPtr().background == 0


def test_a_bad_environment_is_refused_and_leaves_the_scene_as_it_was(p):
    s = p.Scene()
    s.MakeSphere((0, 0, -1), 0.5, s.Lambertian((0.5, 0.5, 0.5)))
    good = EW.random_map(4, 2)
    s.set_environment(good, rotate_y=36.0)
    nan, neg, inf = good.copy(), good.copy(), good.copy()
    nan[1, 2, 0], neg[0, 0, 2], inf[1, 3, 1] = np.nan, -1e-6, np.inf
    for bad, why in ((nan, "not finite"), (inf, "not finite"), (neg, "negative"), (np.zeros((0, 4, 3), F), "zero"), (np.zeros((4, 0, 3), F), "zero")):
        with pytest.raises(p.capi.RtError, match="rt_scene_set_environment.*" + why) as e:
            s.set_environment(bad)
        assert e.value.code == 1   # RT_ERR_INVALID
    with pytest.raises(p.capi.RtError, match="rt_scene_set_environment.*2\\^25"):   # too large: refused on its dimensions, before a texel is read
        p.capi.check(p.capi.lib().rt_scene_set_environment(s.h, 8192, 4097, good.ctypes.data, 0.0))
    with pytest.raises(p.capi.RtError, match="rt_scene_set_environment.*rotation"):
        s.set_environment(good, rotate_y=float("nan"))
    got, u0 = s.environment()
    assert bits_equal(got, good) and u0 == F(np.float64(36.0) / 360.0 - np.floor(np.float64(36.0) / 360.0))
    for bad_u0 in (1.0, -0.1, float("nan")):   # the host function validates as the renderer does
        with pytest.raises(p.capi.RtError, match="rt_environment_batch.*u0"):
            p.api.environment_batch(good, bad_u0, np.ones((1, 3), F))
    with pytest.raises(p.capi.RtError, match="rt_environment_batch.*negative"):
        p.api.environment_batch(neg, 0.0, np.ones((1, 3), F))


# ---- 4. image_io --------------------------------------------------------------------------------------------------------------------------------------------
def test_hdr_round_trip_to_rgbe_precision(tmp_path):
    io = image_io()
    rng = np.random.default_rng(9)
    img = (rng.random((9, 13, 3)) * 10.0 ** rng.uniform(-6, 5, (9, 13, 1))).astype(F)
    img[0, 0] = 0.0
    img[1, 1] = (0.0, 0.0, 123456.0)
    img[2, 2] = (1.0, 0.5, 0.25)
    path = tmp_path / "a.hdr"
    io.write_hdr(str(path), img)
    back = io.read_hdr(str(path))
    assert back.shape == img.shape and back.dtype == F
    # the format: an 8-bit mantissa per channel against the exponent of the pixel's LARGEST channel (its mantissa is >= 128), truncated by the writer and
    # read back at the middle of its step: no channel is off by more than 2^-8 of the largest channel of its pixel
    bound = img.max(axis=2, keepdims=True).astype(np.float64) * 2.0 ** -8
    assert (np.abs(back.astype(np.float64) - img.astype(np.float64)) <= bound).all()
    assert (back[0, 0] == 0).all()
    io.write_hdr(str(path), back)   # what was read is on the format's grid up to the half step
    again = io.read_hdr(str(path))
    assert (np.abs(again.astype(np.float64) - back.astype(np.float64)) <= back.max(axis=2, keepdims=True) * 2.0 ** -8).all()
    sky = io.sky_environment(32, 16)
    assert sky.shape == (16, 32, 3) and sky.dtype == F and np.isfinite(sky).all() and (sky >= 0).all() and sky.max() > 10 and sky[0].mean() != sky[-1].mean()
    for bad in (np.full((2, 2, 3), -1.0), np.full((2, 2, 3), np.nan), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            io.write_hdr(str(path), bad)


def test_hdr_run_length_encoded_scanlines_decode(tmp_path):
    io = image_io()
    w = 8
    head = b"#?RADIANCE\n# a comment\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y 2 +X 8\n"
    # scanline 0: R a run of 8 x 128; G 3 literals, then a run of 5 x 64; B a run of 2 x 0, 6 literals; E a run of 8 x 129 (channel = (m + 0.5) * 2^(129 - 136))
    line0 = bytes([2, 2, 0, w]) + bytes([128 + 8, 128]) + bytes([3, 10, 20, 30, 128 + 5, 64]) + bytes([128 + 2, 0, 6, 1, 2, 3, 4, 5, 6]) + bytes([128 + 8, 129])
    # scanline 1: every channel as 8 literals, exponent 128
    lit = lambda vals: bytes([8]) + bytes(vals)
    line1 = bytes([2, 2, 0, w]) + lit(range(0, 8)) + lit(range(8, 16)) + lit(range(16, 24)) + lit([128] * 8)
    path = tmp_path / "rle.hdr"
    path.write_bytes(head + line0 + line1)
    got = io.read_hdr(str(path))
    m = np.zeros((2, w, 3), np.float64)
    m[0, :, 0] = 128
    m[0, :, 1] = [10, 20, 30, 64, 64, 64, 64, 64]
    m[0, :, 2] = [0, 0, 1, 2, 3, 4, 5, 6]
    m[1, :, 0], m[1, :, 1], m[1, :, 2] = np.arange(0, 8), np.arange(8, 16), np.arange(16, 24)
    want = (m + 0.5) * np.array([2.0 ** (129 - 136), 2.0 ** (128 - 136)])[:, None, None]
    assert bits_equal(got, want.astype(F)), mismatch_report(got, want.astype(F))
    flat = tmp_path / "flat.hdr"   # the same picture as flat scanlines
    rgbe = np.zeros((2, w, 4), np.uint8)
    rgbe[..., :3], rgbe[0, :, 3], rgbe[1, :, 3] = m, 129, 128
    flat.write_bytes(head + rgbe.tobytes())
    assert bits_equal(io.read_hdr(str(flat)), got)


@pytest.mark.parametrize("head", [b"P6\n2 2\n255\n", b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 2 +X 8\n", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+Y 2 +X 8\n",
                                  b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 -X 8\n", b"#?RADIANCE\n\n-Y 2 +X 8\n", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+X 8 -Y 2\n",
                                  b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n"],
                         ids=["no signature", "xyze", "+Y", "-X", "no format", "columns first", "no end"])
def test_hdr_wrong_headers_raise(tmp_path, head):
    path = tmp_path / "bad.hdr"
    path.write_bytes(head + bytes(64))
    with pytest.raises(ValueError, match="read_hdr"):
        image_io().read_hdr(str(path))


def test_hdr_bad_scanlines_raise(tmp_path):
    io = image_io()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 8\n"
    for name, body in (("short", bytes(31)), ("wrong length", bytes([2, 2, 0, 9]) + bytes(64)), ("run past the end", bytes([2, 2, 0, 8, 128 + 9, 1]) + bytes(64)),
                       ("zero count", bytes([2, 2, 0, 8, 0]) + bytes(64)), ("old run-length", bytes([9, 9, 9, 128, 1, 1, 1, 3]) + bytes(24))):
        path = tmp_path / "bad.hdr"
        path.write_bytes(head + body)
        with pytest.raises(ValueError, match="read_hdr"):
            io.read_hdr(str(path))


# ---- 5. the whole-sample twin is the old one plus one hook ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
@pytest.mark.parametrize("background", [None, (0.3, 1.5, 0.9)], ids=["gradient", "constant"])
def test_whole_sample_twin_is_tri_twin_with_the_miss_colour_as_a_parameter(p, background, as_list):
    w, h, spp, depth = 24, 16, 4, 6

    def more(s):
        if background is not None:
            s.set_background(background)
    scene = TW.tri_room(p, open_right=True, as_list=as_list, more=more)   # the room without its right wall: primary and scattered rays leave it
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(TW.camera(p, w, h))
    want, want_followed = TT.frame_samples(world, cam, w, h, spp, depth, TW.SEED)
    stats = {}
    got, followed = ET.frame_samples(world, cam, w, h, spp, depth, TW.SEED, ET.sky_gradient if background is None else ET.sky_constant(background), stats=stats)
    assert np.array_equal(followed, want_followed) and followed.all()   # Lambertian, metal, checker and lights: the followed rule is unchanged
    assert bits_equal(got, want), mismatch_report(got, want)
    assert stats["misses_by_bounce"][0] > 0 and stats["misses_by_bounce"][1:].sum() > 0   # the hook was exercised by primary and by scattered rays


# ---- GPU test 4's world meets its conditions by the twin alone ---------------------------------------------------------------------------------------------
def test_the_sky_rooms_twin_run_meets_the_conditions_of_the_gpu_test():
    run = EW.sky_room_run()
    assert run.followed.mean() >= 0.90, run.followed.mean()
    misses = run.stats["misses_by_bounce"]
    assert misses.sum() > 0 and misses[1:].sum() >= 0.25 * misses.sum(), misses
