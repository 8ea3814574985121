"""Environment maps on the GPU: the probe, an open sky, a constant map on every EXT 2 kernel key, a real map against the whole-sample twin,
sessions, ranks, feature buffers, refusals, and the worlds without a map.  Every comparison is bit for bit: against the host function, against the numpy twin
(tests/_env_twin.py, pinned by tests/test_environment_cpu.py), against the oracle where it knows the world, and between forms where nothing absolute does."""
import functools

import numpy as np
import pytest

import _env_twin as ET
import _env_worlds as EW
import _oracle as O
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = EW.W, EW.H, EW.SPP, EW.DEPTH, EW.SEED
EXT2 = EW.EXT2_FORMS
EXT2_IDS = [TW.form_id(f) for f in EXT2]
PLAIN_LDS = {"kernel": "stream", "exact": 0, "filter": 0, "world": 0, "ext": 2, "big": 0, "wide": 0, "tol": 0, "nee": 0}   # what variant 0 picks for a small BVH world


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def setenv(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def frame_of(r):
    r.Render()
    return r.DownloadRenderbuffer()


def renderer(p, scene, form=None, mode=0, tri=False, variant=None, w=W, h=H, spp=SPP, depth=DEPTH):
    """a renderer of `scene` that states the kernel it runs: form = a _tri_worlds.FORMS key (its variant; the caller has set its environment), or None = variant 0"""
    v = TW.FORMS[form][0] if form is not None else (variant or 0)
    r = p.Renderer.MakeRenderer(w, h, spp, depth, EW.camera(p, w, h), scene.getWorldPtr(), seed=SEED, variant=v)
    if mode:
        r.light_sampling(mode)
    if form is not None:
        assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
        assert r.kernel_triangles() == (tri or mode == 16) and r.kernel_light_tree() == (mode == 16)
    return r


# ---- 1. the probe ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u0", EW.ROTATIONS, ids=EW.ROTATION_IDS)
@pytest.mark.parametrize("size", EW.SIZES, ids=[f"{w}x{h}" for w, h in EW.SIZES])
def test_probe_equals_the_host_function(p, size, u0):
    env = EW.random_map(*size)
    dirs = EW.directions()
    rgb, texel = p.api.probe_environment(env, u0, dirs)
    want_rgb, want_texel = p.api.environment_batch(env, u0, dirs)
    assert np.array_equal(texel, want_texel), f"{int((texel != want_texel).sum())} texel indices differ"
    assert bits_equal(rgb, want_rgb), mismatch_report(rgb, want_rgb)


def test_probe_on_a_large_map(p):
    w, h = 2048, 1024   # pointer and index width: 32 MiB of texels, indices beyond 2^20
    rng = np.random.default_rng(77)
    env = (rng.random((h, w, 3), dtype=F) * F(50.0)).astype(F)
    dirs = np.concatenate([EW.random_directions(4096, seed=78), EW.crafted_directions()[1]])
    rgb, texel = p.api.probe_environment(env, 0.3, dirs)
    want_rgb, want_texel = ET.lookup(env, F(0.3), dirs)
    assert np.array_equal(texel, want_texel) and bits_equal(rgb, want_rgb), mismatch_report(rgb, want_rgb)
    assert texel.max() > (1 << 20) and len(np.unique(texel)) > 4000
    assert len(p.api.probe_environment(env[:2, :2], 0.0, np.zeros((0, 3), F))[1]) == 0


# ---- 2. open sky ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotate", [0.0, 108.0], ids=["u0=0", "u0=0.3"])
def test_open_sky_is_the_mean_of_the_twins_lookups(p, rotate):
    env = EW.random_map(16, 8, decades=(-1.5, 0.5))   # a few texels above 1, most below: the frame's clamp leaves them apart
    scene = EW.open_sky(p, env, rotate_y=rotate)
    r = renderer(p, scene)
    assert r.kernel_form() == PLAIN_LDS   # (the twin restates the pinhole camera only)
    info = r.environment_info()
    assert info["enabled"] and (info["width"], info["height"]) == (16, 8) and info["u0"] == scene.environment()[1]
    got = frame_of(r)
    r.close()
    want = EW.open_sky_frame(p, env, scene.environment()[1])
    assert bits_equal(got, want), mismatch_report(got, want)
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 20   # many texels in view


def test_a_one_texel_map_gives_its_colour_in_every_pixel(p):
    c = np.array([1.75, 0.5, 0.25], F)
    scene = EW.open_sky(p, c.reshape(1, 1, 3))
    r = renderer(p, scene)
    assert r.kernel_form() == PLAIN_LDS
    r.refine(SPP)
    sums = r.refine_sums()
    frame = r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(sums[..., 0:3], np.broadcast_to(c * F(SPP), (H, W, 3)))   # SPP = 8 copies of c, added in order: exact
    assert bits_equal(frame[..., 0:3], np.broadcast_to(np.sqrt(np.minimum(c, F(1))), (H, W, 3)))


# ---- 3. constant map == constant background == oracle, on every EXT 2 form ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_room_frame(tri, as_list, traversal=0):
    p = pkg()
    scene = EW.env_room(p, EW.C, tri, as_list=as_list, traversal=traversal)
    frame, _ = O.render(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(EW.camera(p)), W, H, SPP, DEPTH, SEED)
    frame.setflags(write=False)
    return frame


@pytest.mark.parametrize("form", EXT2, ids=EXT2_IDS)
@pytest.mark.parametrize("tri", [False, True], ids=["plain", "TRI"])
def test_constant_map_is_the_constant_background_is_the_oracle(p, monkeypatch, tri, form):
    """the 8 plain and the 8 TRI stack-walk and list keys"""
    as_list = form[0] == TW.LIST
    setenv(monkeypatch, TW.FORMS[form][1])
    scene = EW.env_room(p, ("map", EW.constant_map(), 40.0), tri, as_list=as_list)
    r = renderer(p, scene, form, tri=tri)
    assert r.environment_info()["enabled"]
    got = frame_of(r)
    r.close()
    want = oracle_room_frame(tri, as_list)
    assert bits_equal(got, want), mismatch_report(got, want)
    assert (got[..., 0] == 1.0).any()   # the sky is in view, its red above 1


@pytest.mark.parametrize("traversal", [1, 2], ids=["queue", "wide4"])
def test_constant_map_on_the_lane_walks(p, traversal):
    """the ninth plain key: RT_WORLD_BVH_QUEUE at EXT 2"""
    scene = EW.env_room(p, ("map", EW.constant_map(), 0.0), False, traversal=traversal)
    r = renderer(p, scene)
    assert r.kernel_form() == EW.QUEUE_FORM
    got = frame_of(r)
    r.close()
    want = oracle_room_frame(False, False, traversal)
    assert bits_equal(got, want), mismatch_report(got, want)


@pytest.mark.parametrize("form", EXT2, ids=EXT2_IDS)
@pytest.mark.parametrize("family", ["NEE", "TRI_NEE", "LTREE"])
def test_constant_map_is_the_constant_background_under_light_sampling(p, monkeypatch, family, form):
    """the 8 NEE, 8 TRI && NEE and 8 LTREE keys.  The oracle samples no lights, so the standard here is the same kernel on the same world with the constant
    background of colour c (held to the twins by the light-sampling tests).  An image material that nothing uses keeps the world EXT 2 under the constant
    background too, so the only difference between the two launches is the miss branch taken."""
    as_list = form[0] == TW.LIST
    setenv(monkeypatch, TW.FORMS[form][1])
    tri = family != "NEE"
    mode = {"NEE": 2, "TRI_NEE": 4, "LTREE": 16}[family]
    frames = []
    for background in (("map", EW.constant_map(3, 5), 250.0), EW.C):
        scene = EW.env_room(p, background, tri, as_list=as_list, image_material=True)
        r = renderer(p, scene, form, mode=mode, tri=tri)
        assert r.light_sampling_mode() == mode
        frames.append(frame_of(r))
        r.close()
    assert bits_equal(frames[0], frames[1]), mismatch_report(frames[0], frames[1])
    assert (frames[0][..., 0] == 1.0).any()


def test_light_table_normals_texture_coordinates_and_map_all_at_once(p, monkeypatch):
    """the header and offset arithmetic with every rider on: light table, vertex normals, texture coordinates, environment record"""
    for env_vars in (TW.LDS, TW.NARROW):
        setenv(monkeypatch, env_vars)
        frames = []
        for background in (("map", EW.constant_map(), 40.0), EW.C):
            scene = EW.env_room(p, background, True, tables=True)
            r = renderer(p, scene)
            r.light_sampling(16)
            k = r.kernel_form()
            assert k["ext"] == 2 and k["nee"] == 1 and k["big"] == (env_vars is TW.NARROW) and r.kernel_light_tree() and r.kernel_triangles()
            assert r.shading_normals_info()["smooth"] == 80 and r.texture_coords_info()["mapped"] == 81
            assert r.environment_info()["enabled"] == isinstance(background[0], str)
            frames.append(frame_of(r))
            if isinstance(background[0], str):   # the riders go and come one at a time; the map stays where the header says it is
                vn, uv = scene.vertex_normals(), scene.texture_coords()
                r.shading_normals(None)
                no_vn = frame_of(r)
                r.texture_coords(None)
                r.shading_normals(vn)
                no_uv = frame_of(r)
                r.texture_coords(uv)
                assert bits_equal(frame_of(r), frames[0]) and not bits_equal(no_vn, frames[0]) and not bits_equal(no_uv, frames[0])
                r.light_sampling(0)
                plain = frame_of(r)
                r.light_sampling(4)
                r.light_sampling(16)
                assert bits_equal(frame_of(r), frames[0]) and not bits_equal(plain, frames[0])
                frames.append(no_vn)
                frames.append(no_uv)
            else:
                r.shading_normals(None)
                frames.append(frame_of(r))
                r.texture_coords(None)
                r.shading_normals(scene.vertex_normals())
                frames.append(frame_of(r))
            r.close()
        for a, b in zip(frames[:3], frames[3:]):
            assert bits_equal(a, b), mismatch_report(a, b)


# ---- 4. a real map against the whole-sample twin -----------------------------------------------------------------------------------------------------------
def test_a_real_map_equals_the_whole_sample_twin_and_every_form_agrees(p, monkeypatch):
    run = EW.sky_room_run()
    assert run.followed.mean() >= 0.90
    misses = run.stats["misses_by_bounce"]
    assert misses[1:].sum() >= 0.25 * misses.sum()
    setenv(monkeypatch, TW.LDS)
    r = renderer(p, run.scene)
    assert r.kernel_form() == PLAIN_LDS and r.environment_info()["u0"] == F(0.3)
    r.refine(SPP)
    first = r.DownloadRenderbuffer()
    sums = r.refine_sums()
    r.close()
    whole = run.followed.all(axis=2)   # pixels whose every sample the twin followed: their sums are the twin's, bit for bit
    want = ET.in_order_sums(run.samples)
    assert bits_equal(sums[whole], want[whole]), mismatch_report(sums[whole], want[whole])
    assert bits_equal(first[whole], run.frame[whole])
    assert whole.all()   # this world holds only what the twin follows
    for form in EXT2:   # the other plain keys, and the TRI keys on the world with a triangle no ray reaches
        as_list = form[0] == TW.LIST
        setenv(monkeypatch, TW.FORMS[form][1])
        for tri in (False, True):
            scene = EW.sky_room(p, hidden_triangle=tri, as_list=as_list)
            r = renderer(p, scene, form, tri=tri)
            got = frame_of(r)
            r.close()
            assert bits_equal(got, first), (TW.form_id(form), tri, mismatch_report(got, first))
    setenv(monkeypatch, TW.LDS)
    for traversal in (1, 2):
        r = renderer(p, EW.sky_room(p, traversal=traversal))
        assert r.kernel_form() == EW.QUEUE_FORM
        got = frame_of(r)
        r.close()
        assert bits_equal(got, first), (traversal, mismatch_report(got, first))


# ---- 5. sessions ---------------------------------------------------------------------------------------------------------------------------------------------
def test_sessions_keep_restart_refuse_and_reproduce(p, monkeypatch):
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # cuts inside the frame
    scene = EW.sky_room(p)
    env, u0 = scene.environment()
    r = renderer(p, scene)
    assert r.kernel_form() == PLAIN_LDS
    first = frame_of(r)
    r.refine(3)
    r.refine(1)
    r.environment(env.copy(), u0=u0)   # the same map again: the refinement goes on
    assert r.refine_info()["samples"] == 4
    r.refine(SPP - 4)
    assert bits_equal(r.DownloadRenderbuffer(), first)   # steps == one render at the accumulated count
    r.environment(env, u0=0.5)         # another rotation restarts it, and the next frame is the new one's
    assert r.refine_info()["samples"] == 0 and r.environment_info()["u0"] == F(0.5)
    turned = frame_of(r)
    other = EW.random_map(16, 8)
    r.environment(other, u0=0.5)       # another map restarts it
    assert r.refine_info()["samples"] == 0 and (r.environment_info()["width"], r.environment_info()["height"]) == (16, 8)
    other_frame = frame_of(r)
    assert len({first.tobytes(), turned.tobytes(), other_frame.tobytes()}) == 3
    s2 = EW.sky_room(p)
    s2.set_environment(other, rotate_y=180.0)
    r2 = renderer(p, s2)
    assert bits_equal(frame_of(r2), other_frame)   # ... the frame a fresh renderer makes of that map
    r2.close()
    r.environment(None)                # off: a background-2 renderer without a map launches nothing
    assert not r.environment_info()["enabled"]
    for call in (r.Render, lambda: r.refine(1), r.render_async, lambda: r.refine_async(1)):
        with pytest.raises(p.capi.RtError, match="rt_renderer_environment") as e:
            call()
        assert e.value.code == 1
    assert r.refine_info()["samples"] == 0
    r.environment(None)                # off twice: nothing
    r.environment(env, u0=u0)          # on again: the first frame
    assert bits_equal(frame_of(r), first)
    r.close()


# ---- 6. ranks ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 3])
def test_ranks_through_the_memcpy_transport(p, monkeypatch, ranks):
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    scene = EW.sky_room(p)
    r = renderer(p, scene)
    one = frame_of(r)
    r.close()
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, EW.camera(p), scene.getWorldPtr(), ranks, seed=SEED)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), one)
    bad = scene.environment()[0].copy()
    bad[3, 3, 1] = -1.0
    with pytest.raises(p.capi.RtError, match="rt_renderer_environment.*negative"):
        m.environment(bad)   # refused before any rank changes
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), one)
    m.environment(None)
    with pytest.raises(p.capi.RtError, match="rt_renderer_environment"):
        m.Render()
    m.environment(*scene.environment())
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), one)
    m.close()


# ---- 7. feature buffers --------------------------------------------------------------------------------------------------------------------------------------
def test_feature_buffers_do_not_see_the_map(p):
    sums = []
    for background in (("map", EW.random_map(16, 8), 40.0), EW.C):
        scene = EW.env_room(p, background, True)
        r = renderer(p, scene)
        assert r.kernel_form()["ext"] == (2 if isinstance(background[0], str) else 1)
        r.enable_aov()
        r.refine(SPP)
        assert r.aov_info()["samples"] == SPP
        sums.append(r.aov_sums())
        r.close()
    assert bits_equal(sums[0], sums[1]), mismatch_report(sums[0], sums[1])   # normal, depth, albedo, coverage
    assert 0 < (sums[0][..., 7] > 0).mean() < 1   # hits and sky both in view


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_each_with_its_own_message(p):
    cam = EW.camera(p)
    spheres = p.Scene.book1_final(SEED)   # the reference's feature set: variants 5 and 6 take it, until its background is a map
    spheres.set_environment(EW.constant_map())
    for variant, word in ((1, "baseline kernel \\(variant 1\\)"), (5, "variant 5"), (6, "variant 6")):
        with pytest.raises(p.capi.RtError, match=word + ".*environment map") as e:
            p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, spheres.getWorldPtr(), seed=SEED, variant=variant)
        assert e.value.code == 1
    for background in (None, (0.2, 0.3, 0.4)):   # modes 0 and 1
        s = p.Scene.book1_final(SEED)
        s.set_background(background)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED)
        before = frame_of(r)
        with pytest.raises(p.capi.RtError, match="rt_renderer_environment.*background mode is " + ("0" if background is None else "1")) as e:
            r.environment(EW.constant_map())
        assert e.value.code == 1 and not r.environment_info()["enabled"] and bits_equal(frame_of(r), before)
        r.environment(None)   # off on a world without a map: nothing
        r.close()
    cfg = p.capi.RenderConfig(W, H, 1, DEPTH, SEED, 0, 0, 1, 0)
    with pytest.raises(p.capi.RtError, match="rt_probe_radiance.*environment map"):
        p.api.probe_radiance(cfg, cam, spheres.getWorldPtr(), np.zeros((1, 2), np.uint32))
    scene = EW.sky_room(p)
    env, u0 = scene.environment()
    r = renderer(p, scene)
    first = frame_of(r)
    nan, neg = env.copy(), env.copy()
    nan[2, 5, 0], neg[0, 0, 0] = np.nan, -0.5
    for bad, kw, why in ((nan, {}, "not finite"), (neg, {}, "negative"), (np.zeros((0, 3, 3), F), {}, "zero"), (env, {"u0": 1.0}, "u0"), (env, {"u0": -0.25}, "u0"),
                         (env, {"u0": float("nan")}, "u0")):
        with pytest.raises(p.capi.RtError, match="rt_renderer_environment.*" + why) as e:
            r.environment(bad, **kw)
        assert e.value.code == 1
    with pytest.raises(p.capi.RtError, match="rt_renderer_environment.*2\\^25"):
        p.capi.check(p.capi.lib().rt_renderer_environment(r.h, 8192, 4097, env.ctypes.data, 0.0))
    with pytest.raises(p.capi.RtError, match="rt_probe_environment.*negative"):
        p.api.probe_environment(neg, 0.0, np.ones((1, 3), F))
    assert r.environment_info()["enabled"] and r.environment_info()["u0"] == u0 and bits_equal(frame_of(r), first)   # the renderer is as it was
    for mode in (1, 2, 4, 16):   # a world lit only by its map has no light table: the modes refuse it as ever
        with pytest.raises(p.capi.RtError, match="rt_renderer_light_sampling_enable"):
            r.light_sampling(mode)
    r.close()


# ---- 9. nothing else moved -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("background", [None, (0.3, 1.5, 0.9)], ids=["gradient", "constant"])
def test_worlds_without_a_map_render_the_oracles_frames(p, background):
    cam = EW.camera(p)
    builds = {}
    if background is None:   # EXT 0: the reference's feature set under its gradient
        s = p.Scene.book1_final(SEED)
        builds[0] = (s, p.PinholeCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H))
    builds[1] = (EW.env_room(p, background, False), cam)                      # EXT 1: quads and lights
    builds[2] = (TW.tri_room(p, textured=True, open_right=True, more=lambda s: s.set_background(background)), cam)   # EXT 2: an image texture
    for ext, (scene, c) in builds.items():
        w = scene.getWorldPtr()
        assert w.background == (0 if background is None else 1)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, c, w, seed=SEED)
        assert r.kernel_form()["kernel"] == "stream" and r.kernel_form()["ext"] == ext and not r.environment_info()["enabled"]
        got = frame_of(r)
        r.close()
        want, _ = O.render(as_oracle_world(w), as_oracle_camera(c), W, H, SPP, DEPTH, SEED)
        assert bits_equal(got, want), (ext, mismatch_report(got, want))
