"""Lens cameras on the GPU: the probe against the host batch; the type-16 copies of the three reference cameras against the frames the CPU oracle
pins; every form of primary_rays_lens_kernel against the numpy twin (tests/_lens_twin.py feeding the whole-sample loop of tests/_path_twin.py, which
tests/test_path_twin_oracle_cpu.py holds to the oracle), bit for bit on every pixel; refinement in steps; the feature buffers; a panorama read back as the
environment map it was lit by; ranks; refusals and sessions; the C++ mirror.  Frames are 20 x 12 — no multiple of the 8 x 8 tile on either axis, so both edges have
padding pixels — at 5 samples (64 * 5 = 320 threads per block row: one full 256-thread block and a partial one) and depth 6."""
import os
import subprocess

import numpy as np
import pytest

import _aov_full_twin as FT
import _aov_full_worlds as FW
import _aov_tex_twin as AT
import _lens_twin as LT
import _oracle as O
import _path_twin as PT
import _tri_twin as TT
import test_lens_cameras_cpu as CPU
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, oracle_scene, pkg
from _nee_twin import in_order_sums, resolve

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = 20, 12, 5, 6, 1984
UP = (0, 1, 0)


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


# per world: the configuration's own eye, an oblique eye, an eye inside the scene for the wide views, an eye and a target on one axis, the orthographic window's
# height, and a focus distance that reaches the scene
WORLDS = {
    "three_spheres": dict(eye=(0, 0, 0), at=(0, 0, -1), oblique=(1.5, 1.0, 0.6), inside=(0, 0.1, 0.2), axis=((0, 0, 0), (0, 0, -1)), height=2.0, focus=1.0, aperture=0.2),
    "cornell_box": dict(eye=(278, 278, -800), at=(278, 278, 278), oblique=(100, 420, -700), inside=(278, 278, 60), axis=((278, 278, -800), (278, 278, 0)), height=560.0,
                        focus=1000.0, aperture=30.0),
    "book2_moving": dict(eye=(13, 2, 3), at=(0, 0, 0), oblique=(9, 4, 7), inside=(3, 1.2, 2), axis=((0, 1, 12), (0, 1, 0)), height=6.0, focus=10.0, aperture=0.3),
}
CAMERAS = ["ortho_oblique", "ortho_axis", "fisheye", "panorama", "perspective_lens_shutter", "ortho_lens_shutter", "fisheye_lens_shutter", "panorama_lens_shutter"]


def camera(p, world, kind):
    c, a = WORLDS[world], W / H
    blur = (c["aperture"], c["focus"], 0.0, 1.0)
    if kind == "ortho_oblique":
        return p.api.OrthographicCamera(c["oblique"], c["at"], UP, c["height"], a)
    if kind == "ortho_axis":   # every direction has two zero components
        return p.api.OrthographicCamera(c["axis"][0], c["axis"][1], UP, c["height"], a)
    if kind == "fisheye":
        return p.api.FisheyeCamera(c["inside"], c["at"], UP, 180.0, a)
    if kind == "panorama":
        return p.api.PanoramaCamera(c["inside"], c["at"], UP)
    if kind == "perspective_lens_shutter":
        return p.api.PerspectiveCamera(c["eye"], c["at"], UP, 40.0, a, *blur)
    if kind == "ortho_lens_shutter":
        return p.api.OrthographicCamera(c["oblique"], c["at"], UP, c["height"], a, *blur)
    if kind == "fisheye_lens_shutter":
        return p.api.FisheyeCamera(c["inside"], c["at"], UP, 180.0, a, *blur)
    if kind == "panorama_lens_shutter":
        return p.api.PanoramaCamera(c["inside"], c["at"], UP, 360.0, 180.0, *blur)
    base, one = kind.rsplit("_", 1)   # the forms with one of the two: "<projection>_lens", "<projection>_shutter"
    only = (c["aperture"], c["focus"], 0.0, 0.0) if one == "lens" else (0.0, c["focus"], 0.0, 1.0)
    assert one in ("lens", "shutter") and base in ("ortho", "fisheye", "panorama"), kind
    if base == "ortho":
        return p.api.OrthographicCamera(c["oblique"], c["at"], UP, c["height"], a, *only)
    if base == "fisheye":
        return p.api.FisheyeCamera(c["inside"], c["at"], UP, 180.0, a, *only)
    return p.api.PanoramaCamera(c["inside"], c["at"], UP, 360.0, 180.0, *only)


SCENES, TWINS = {}, {}


def scene_of(p, world):
    if world not in SCENES:
        SCENES[world] = config_scene(p, world, SEED)
    return SCENES[world]


def twin_samples(p, world, kind, spp=SPP, first_sample=0):
    """the whole-sample twin's (H, W, spp, 3) samples of `world` under camera `kind`, with the lens twin's primary rays; computed once and left unchanged"""
    key = (world, kind, spp, first_sample)
    if key not in TWINS:
        scene, cam = scene_of(p, world), camera(p, world, kind)
        primary, PT.primary_rays = PT.primary_rays, LT.primary_rays   # the loop looks the name up at call time
        try:
            radiance = lambda g, s: PT.radiance(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, DEPTH, SEED, g, s, TT.closest_intersection,  # noqa: E731
                                                glass=True, media=True)
            samples, followed = PT.frame_samples(radiance, W, H, spp, first_sample)
        finally:
            PT.primary_rays = primary
        assert followed.all(), f"{int((~followed).sum())} samples not followed"   # none is left out
        samples.setflags(write=False)
        TWINS[key] = samples
    return TWINS[key]


def renderer(p, world, cam, spp=SPP, **kw):
    return p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, scene_of(p, world).getWorldPtr(), seed=SEED, **kw)


def frame_of(p, world, cam, spp=SPP, **kw):
    r = renderer(p, world, cam, spp, **kw)
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.close()
    return frame


# ---- 1. the probe ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_probe_is_the_host_batch_bit_for_bit(p):
    st, tape, offsets = CPU.cases()
    for name, cam in CPU.forms(p):
        for n in (len(st), 1, 127, 129):
            rays, draws = p.api.probe_camera_lens(cam, st[:n], tape, offsets[:n])
            want, want_draws = p.api.camera_rays_batch(cam, st[:n], tape, offsets[:n])
            assert bits_equal(rays, want), (name, n, mismatch_report(rays, want))
            assert (draws == want_draws).all(), (name, n)
    with pytest.raises(p.capi.RtError, match="no lens camera"):
        p.api.probe_camera_lens(p.PinholeCamera((0, 0, 0), (0, 0, -1), UP, 90.0, 1.0), st[:1], tape, offsets[:1])


# ---- 2. frames the CPU oracle pins -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["three_spheres", "book1_final", "book2_moving"])
def test_a_type_16_copy_renders_the_reference_cameras_frame(p, which):
    """<PERSPECTIVE, 0, 0> is the pinhole, <.., 1, 0> the defocus and <.., 0, 1> the motion camera: the legacy frame, which is the CPU oracle's"""
    scene, cam = config_scene(p, which, SEED), config_cameras(p, which, W, H)
    copy = CPU.lens_copy(p, cam)
    assert copy.type == 16 and (copy.lens_radius > 0) == (which == "book1_final") and (copy.t0 != copy.t1) == (which == "book2_moving")
    frames = []
    for c in (cam, copy):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, c, scene.getWorldPtr(), seed=SEED)
        r.Render()
        frames.append(r.DownloadRenderbuffer())
        r.close()
    assert bits_equal(frames[1], frames[0]), mismatch_report(frames[1], frames[0])
    oscene = oracle_scene(which, SEED)   # (kept alive: its world borrows its arrays)
    ref, _ = O.render(oscene.world, as_oracle_camera(cam), W, H, SPP, DEPTH, SEED)
    assert bits_equal(frames[0], ref), mismatch_report(frames[0], ref)


# ---- 3. frames the twin holds ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CAMERAS)
@pytest.mark.parametrize("world", list(WORLDS))
def test_every_projection_is_the_twin_on_every_pixel(p, world, kind):
    """Without the feature this fails at the camera's constructor."""
    cam = camera(p, world, kind)
    samples = twin_samples(p, world, kind)
    want = in_order_sums(samples)
    r = renderer(p, world, cam)
    r.refine(SPP)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(sums, want), (world, kind, mismatch_report(sums, want))
    assert bits_equal(frame, resolve(want, SPP)), mismatch_report(frame, resolve(want, SPP))
    lit = (want[..., 0:3] > 0).any(axis=2).sum()
    assert lit >= (10 if world == "cornell_box" else (W * H) // 2), (world, kind, lit)   # the camera sees the scene (five samples find the Cornell lamp from few pixels)
    if kind == "ortho_axis":
        w = np.array(list(cam.w), F)
        assert (w == 0).sum() == 2
    plain = frame_of(p, world, config_cameras(p, world, W, H))
    assert not bits_equal(plain, frame)


@pytest.mark.parametrize("kind", [f"{b}_{o}" for b in ("ortho", "fisheye", "panorama") for o in ("lens", "shutter")])
def test_the_forms_with_a_lens_or_a_shutter_alone_are_the_twin_too(p, kind):
    """the six instantiations the cameras above leave out: with them, and the three type-16 copies, all sixteen forms have rendered a frame"""
    world = "book2_moving"
    cam = camera(p, world, kind)
    assert (cam.lens_radius > 0) != (cam.t0 != cam.t1)
    want = in_order_sums(twin_samples(p, world, kind))
    r = renderer(p, world, cam)
    r.refine(SPP)
    sums = r.refine_sums()
    r.close()
    assert bits_equal(sums, want), (kind, mismatch_report(sums, want))
    both = in_order_sums(twin_samples(p, world, kind.rsplit("_", 1)[0] + "_lens_shutter"))
    assert not bits_equal(want, both)


# ---- 4. steps --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refinement_in_steps_is_one_render(p):
    world, kind = "book2_moving", "fisheye_lens_shutter"
    cam = camera(p, world, kind)
    r = renderer(p, world, cam)
    r.refine(2)
    head = r.refine_sums()
    r.refine(3)
    stepped, stepped_frame = r.refine_sums(), r.DownloadRenderbuffer()
    r.close()
    want = in_order_sums(twin_samples(p, world, kind))
    assert bits_equal(head, in_order_sums(twin_samples(p, world, kind)[:, :, 0:2]))
    assert bits_equal(stepped, want), mismatch_report(stepped, want)
    tail = twin_samples(p, world, kind, spp=3, first_sample=2)   # pass_first_s: the second step's samples are samples 2 to 4 of their streams
    assert bits_equal(tail, twin_samples(p, world, kind)[:, :, 2:5])
    once = frame_of(p, world, cam)
    assert bits_equal(stepped_frame, once), mismatch_report(stepped_frame, once)


# ---- 5. feature buffers ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["panorama", "ortho_oblique"])
def test_the_feature_buffers_follow_the_cameras_rays(p, monkeypatch, kind):
    world = "cornell_box"
    cam = camera(p, world, kind)
    LT.use(monkeypatch)
    want, hit_share = AT.sums(as_oracle_world(scene_of(p, world).getWorldPtr()), as_oracle_camera(cam), W, H, SPP, SEED, False)
    r = renderer(p, world, cam)
    r.enable_aov()
    r.refine(SPP)
    got, sums = r.aov_sums(), r.refine_sums()
    r.close()
    assert bits_equal(got, want), (kind, mismatch_report(got, want))
    assert hit_share > 0.5 and bits_equal(sums, in_order_sums(twin_samples(p, world, kind)))   # the colour frame beside the features is the twin's


def test_the_full_feature_pass_follows_a_lens_camera_through_fog(p, monkeypatch):
    scene = FW.room(p, masks=False, fog=True)
    cam = p.api.FisheyeCamera(FW.EYE, (0, 1, 0), UP, 150.0, W / H, 0.3, 8.0, 0.0, 1.0)
    LT.use(monkeypatch)
    stats = FT.new_stats()
    want = FT.sums(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, SPP, SEED, stats=stats, **FW.tables(scene))
    assert stats["fog_hits"] > 0 and stats["through_fog"] > 0, stats
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
    r.enable_aov(full=True)
    r.refine(SPP)
    got = r.aov_sums()
    r.close()
    assert bits_equal(got, want), mismatch_report(got, want)


# ---- 6. a panorama is the environment map it was lit by ------------------------------------------------------------------------------------------------------------------
def test_a_full_panorama_reads_the_environment_map_back(p):
    MW, MH = 64, 32
    rng = np.random.default_rng(23)
    image = (rng.random((MH, MW, 3)) * 4).astype(F)
    s = p.Scene()
    s.MakeSphere((3.0, 0.4, 0.5), 0.3, s.Lambertian((0.7, 0.6, 0.5)))
    s.MakeSphere((-2.0, -1.0, 1.5), 0.25, s.Lambertian((0.2, 0.6, 0.5)))
    s.set_environment(image)
    s.BuildBVH_SAH()
    cam = p.api.PanoramaCamera((0, 0, 0), (1, 0, 0), UP)
    gids, smp = PT.keys(MW, MH, 1)
    _, rays = LT.primary_rays(as_oracle_camera(cam), MW, MH, SEED, gids, smp, timed=True)
    hit = TT.closest_intersection(as_oracle_world(s.getWorldPtr()), rays)[0].reshape(MH, MW) != 0
    assert 0 < hit.sum() <= 0.05 * MW * MH, hit.sum()   # the miss share is at least 95 %, and the spheres are seen
    r = p.Renderer.MakeRenderer(MW, MH, 1, DEPTH, cam, s.getWorldPtr(), seed=SEED)
    r.refine(1)
    sums = r.refine_sums()
    r.close()
    own = image[::-1]   # the frame's row 0 is the bottom, the map's row 0 the top
    assert bits_equal(sums[..., 0:3][~hit], own[~hit]), mismatch_report(sums[..., 0:3][~hit], own[~hit])
    assert not bits_equal(sums[..., 0:3][hit], own[hit])


# ---- 7. ranks ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    world, kind = "book2_moving", "fisheye_lens_shutter"
    cam = camera(p, world, kind)
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene_of(p, world).getWorldPtr(), 2, seed=SEED)
    m.Render()
    frame = m.DownloadRenderbuffer()
    bad = type(cam).from_buffer_copy(bytes(cam))
    bad.viewport_height = 4.0
    with pytest.raises(p.capi.RtError, match="rt_multi_renderer_set_camera.*pi"):
        m.set_camera(bad)
    m.Render()
    again = m.DownloadRenderbuffer()
    m.close()
    one = frame_of(p, world, cam)
    assert bits_equal(frame, one), mismatch_report(frame, one)
    assert bits_equal(again, one)


# ---- 8. refusals and sessions --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(p):
    world = "three_spheres"
    lens = camera(p, world, "perspective_lens_shutter")
    with pytest.raises(p.capi.RtError, match="baseline kernel"):
        renderer(p, world, lens, variant=1)
    baseline = renderer(p, world, config_cameras(p, world, W, H), variant=1)
    baseline.Render()
    before = baseline.DownloadRenderbuffer()
    with pytest.raises(p.capi.RtError, match="rt_renderer_set_camera.*baseline kernel"):
        baseline.set_camera(lens)
    baseline.Render()
    assert bits_equal(baseline.DownloadRenderbuffer(), before)
    baseline.close()
    foggy = FW.fog_tree(p)   # a bvh_node tree with a medium renders on the baseline kernel alone
    with pytest.raises(p.capi.RtError, match="baseline kernel"):
        p.Renderer.MakeRenderer(W, H, SPP, DEPTH, lens, foggy.getWorldPtr(), seed=SEED)
    for t in (3, 15, 20):
        c = type(lens).from_buffer_copy(bytes(lens))
        c.type = t
        with pytest.raises(p.capi.RtError, match="unknown camera type"):
            renderer(p, world, c)
    st, tape, offsets = CPU.cases(n_random=2)
    with pytest.raises(p.capi.RtError, match="rt_probe_camera_tape: unknown camera type"):
        p.api.probe_camera_tape(lens, st, tape, offsets.reshape(-1))
    with pytest.raises(p.capi.RtError, match="rt_probe_camera: unknown camera type"):
        p.api.probe_camera(SEED, lens, st, np.zeros((len(st), 2), np.uint32))
    cfg = p.capi.RenderConfig(W, H, SPP, DEPTH, SEED, 0, 0, 1, 0)
    with pytest.raises(p.capi.RtError, match="rt_probe_radiance: unknown camera type"):
        p.api.probe_radiance(cfg, lens, scene_of(p, world).getWorldPtr(), np.zeros((1, 2), np.uint32))


def test_a_refused_set_camera_leaves_the_next_frame_unchanged(p):
    world = "cornell_box"
    good = camera(p, world, "fisheye")
    r = renderer(p, world, good)
    r.Render()
    before = r.DownloadRenderbuffer()
    bad = type(good).from_buffer_copy(bytes(good))
    bad.viewport_width = float("nan")
    with pytest.raises(p.capi.RtError, match="rt_renderer_set_camera.*viewport_width"):
        r.set_camera(bad)
    bad.viewport_width = 3.0   # corner sqrt(9 + (pi/2)^2) = 3.39 >= pi
    with pytest.raises(p.capi.RtError, match="pi"):
        r.set_camera(bad)
    r.Render()
    after = r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(after, before)


def test_switching_cameras_on_one_renderer_gives_each_time_the_fresh_frame(p):
    world = "cornell_box"
    pinhole, pano = config_cameras(p, world, W, H), camera(p, world, "panorama_lens_shutter")
    fresh = {id(c): frame_of(p, world, c) for c in (pinhole, pano)}
    assert not bits_equal(fresh[id(pinhole)], fresh[id(pano)])
    r = renderer(p, world, pinhole)
    for c in (pinhole, pano, pinhole, pano):
        r.set_camera(c)
        r.Render()
        got = r.DownloadRenderbuffer()
        assert bits_equal(got, fresh[id(c)]), mismatch_report(got, fresh[id(c)])
    r.close()


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_app_renders_pythons_frames(p, tmp_path):
    d = os.path.join(ROOT, "tests", "cpp_lens_cameras")
    subprocess.check_call(["make", "-s", "-C", d])
    prefix = str(tmp_path / "cpp")
    res = subprocess.run([os.path.join(d, "lens_cameras_app"), str(W), str(H), str(SPP), str(DEPTH), prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip().splitlines() == ["perspective: type=16", "orthographic: type=17", "fisheye: type=18", "panorama: type=19",
                                               "fisheye 300: refused (names the bound)", "variant 1: refused (names the baseline kernel)"]
    s = p.Scene()
    floor, ball = s.Lambertian((0.5, 0.5, 0.5)), s.Metal((0.8, 0.8, 0.9), 0.1)
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), floor)
    s.MakeSphere((0.0, 1.0, 0.0), 1.0, ball)
    s.set_background((0.6, 0.7, 0.9))
    s.BuildBVH_TopDown()
    eye, at, a = (0.5, 2.0, 7.0), (0, 1.0, 0), W / H
    cams = {"perspective": p.api.PerspectiveCamera(eye, at, UP, 50.0, a, 0.4, 7.0, 0.0, 1.0), "orthographic": p.api.OrthographicCamera(eye, at, UP, 6.0, a),
            "fisheye": p.api.FisheyeCamera(eye, at, UP, 180.0, a, 0.4, 7.0, 0.0, 1.0), "panorama": p.api.PanoramaCamera(eye, at, UP)}
    for name, cam in cams.items():
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=1984)
        r.Render()
        want = r.DownloadRenderbuffer()
        r.close()
        got = np.fromfile(f"{prefix}_{name}.f32", dtype=np.float32).reshape(H, W, 4)
        assert bits_equal(got, want), (name, mismatch_report(got, want))
