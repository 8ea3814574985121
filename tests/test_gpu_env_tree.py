"""The map and the light tree together on the GPU (mode 48): the mode accepted where no other samples both lights, all eight kernel forms against
the whole-sample twin, empty and large tables, the silhouette rule, a sun, cuts, sessions and ranks, switching, refusals and the C++ program.  Every comparison
is bit for bit against the numpy twin (tests/_env_tree_twin.py, pinned by tests/test_env_tree_cpu.py), which follows EVERY sample of these worlds, image-textured
hits included.  Frames are 24 x 16 at 8 spp and depth 6; every render states its kernel_form(), kernel_env_light() and kernel_light_tree()."""
import os
import subprocess

import numpy as np
import pytest

import _env_light_worlds as LW
import _env_tree_twin as VT
import _env_tree_worlds as VW
import _env_worlds as EW
import _tri_worlds as TW
from _common import ROOT, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = VW.W, VW.H, VW.SPP, VW.DEPTH, VW.SEED
FORMS = list(VW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
LDS_FAST = (TW.BVH, 0, 2, 0, 0)     # what variant 0 picks for a small BVH world
NARROW_FAST = (TW.BVH, 0, 2, 1, 0)  # ... and with the image left in global memory
MEMORY = [("lds", TW.LDS, LDS_FAST), ("global", TW.NARROW, NARROW_FAST)]


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def setenv(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def frame_of(r):
    r.Render()
    return r.DownloadRenderbuffer()


def renderer(p, scene, form=LDS_FAST, mode=VW.ENV_TREE, spp=SPP, view="room"):
    """a renderer of `scene` on the recipe of `form` (the caller has set its environment) that states the kernel it runs"""
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, VW.camera(p, view), scene.getWorldPtr(), seed=SEED, variant=TW.FORMS[form][0])
    if mode:
        r.light_sampling(mode)
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1 if mode else 0), r.kernel_form()
    assert r.kernel_env_light() == (mode in (32, 48)) and r.kernel_light_tree() == (mode in (16, 48)) and r.light_sampling_mode() == mode
    return r


def sums_of(p, run, form=LDS_FAST, mode=VW.ENV_TREE):
    r = renderer(p, run.scene, form, mode, view=run.view)
    if mode == VW.ENV_TREE:
        assert r.kernel_triangles() and r.light_sampling_info() == {"enabled": True, "lights": run.tree.n_l}
    r.refine(SPP)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(frame, VT.resolve(sums, SPP))
    return sums


# ---- 1. what no other mode does -------------------------------------------------------------------------------------------------------------------------
def test_mode_48_samples_a_triangle_lamp_under_the_sky(p, monkeypatch):
    """A sky room with one triangle lamp.  Mode 32 leaves the lamp to be hit and mode 16 leaves the sky to be missed into; mode 48 samples both, and its frame is
    the twin's on every pixel.  Without the mode the value 48 is refused."""
    setenv(monkeypatch, TW.LDS)
    run = VW.run("triangle_lamp")
    assert run.followed.all() and run.tree.n_l == 1 and run.stats["map_draws"] > 100 and run.stats["table_draws"] > 100
    r = renderer(p, run.scene)
    assert r.light_sampling_info() == {"enabled": True, "lights": 1}
    r.refine(SPP)
    sums = r.refine_sums()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    frames = {48: r.DownloadRenderbuffer()}
    for mode in (32, 16, 0):
        r.light_sampling(mode)
        frames[mode] = frame_of(r)
    r.close()
    assert bits_equal(frames[48], run.frame) and len({f.tobytes() for f in frames.values()}) == 4


# ---- 2. the forms -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_frames():
    """world name -> the sums of the first form rendered of it: what every later form of that world must repeat on EVERY pixel"""
    return {}


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_instantiation_is_the_twin(p, monkeypatch, first_frames, form):
    """All 8 RT_KERNEL_ENV_TREE keys, each reached by its recipe on the room with a checker floor, a Lambertian and a metal sphere, an image-textured mesh with
    per-vertex coordinates and an image-textured parallelogram under a two-image table, a quad light, a sphere lamp and a triangle light: the sums equal the
    whole-sample twin's on every pixel."""
    as_list = form[0] == TW.LIST
    run = VW.run("forms", as_list=as_list)
    setenv(monkeypatch, TW.FORMS[form][1])
    sums = sums_of(p, run, form)
    assert run.followed.all()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    first = first_frames.setdefault("forms", sums)
    assert bits_equal(sums, first), mismatch_report(sums, first)


# ---- 3. the table's sizes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", MEMORY, ids=[m[0] for m in MEMORY])
@pytest.mark.parametrize("n_l", [0, 1, 2, 65])
def test_empty_small_and_large_tables(p, monkeypatch, n_l, memory):
    """n_l = 0: a header alone, no second draw, no walk — the textured room under the sky with no lamp; 1: no index draw; 2; 65: more than mode 4 takes"""
    run = VW.run(f"n_l={n_l}")
    setenv(monkeypatch, memory[1])
    sums = sums_of(p, run, memory[2])
    assert run.followed.all() and run.tree.n_l == n_l
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)


def test_a_world_without_lights_is_the_map_alone_and_still_samples_image_hits(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = VW.run("n_l=0")
    with_48 = sums_of(p, run)
    with_32 = sums_of(p, run, mode=32)
    assert bits_equal(with_48, run.sums) and not bits_equal(with_48, with_32)   # mode 32 does not sample at the image-textured hits
    r = renderer(p, run.scene, mode=0)
    with pytest.raises(p.capi.RtError, match="no light to sample"):
        r.light_sampling(16)
    r.close()


# ---- 4. the silhouette, a sun -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", MEMORY, ids=[m[0] for m in MEMORY])
def test_a_drawn_sphere_light_lost_on_its_silhouette(p, monkeypatch, memory):
    run = VW.run("silhouette")
    assert run.stats["sphere_uncredited"] > 0
    setenv(monkeypatch, memory[1])
    form = (TW.BVH, 0, 2, memory[2][3], 0)
    sums = sums_of(p, run, form)
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)


def test_a_map_with_one_texel_at_1e4(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = VW.run("sun")
    sums = sums_of(p, run)
    assert run.followed.all() and bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert not bits_equal(sums, VW.run("forms").sums)


# ---- 5. cuts, sessions and ranks ----------------------------------------------------------------------------------------------------------------------------
def test_cuts_steps_and_a_replaced_map(p, monkeypatch):
    setenv(monkeypatch, {"RT06_PASS_SPP": "3"})   # cuts inside the frame
    run = VW.run("forms")
    r = renderer(p, run.scene)
    assert r.pass_info()["n_passes"] == 3
    first = frame_of(r)
    assert bits_equal(first, run.frame), mismatch_report(first, run.frame)
    r.refine(3)
    r.refine(1)
    r.environment(run.env.copy(), u0=run.u0)   # the same map again: the refinement goes on
    r.light_sampling("env+tree")               # 48 -> 48 keeps it
    assert r.refine_info()["samples"] == 4
    r.refine(SPP - 4)
    assert bits_equal(r.refine_sums(), run.sums) and bits_equal(r.DownloadRenderbuffer(), first)
    replaced = VW.run("replaced")
    r.environment(replaced.env, u0=run.u0)    # another map while the mode is on: its distribution comes with it, and the refinement restarts
    assert r.refine_info()["samples"] == 0 and r.kernel_env_light() and r.kernel_light_tree() and r.light_sampling_info() == {"enabled": True, "lights": 3}
    r.refine(SPP)
    assert bits_equal(r.refine_sums(), replaced.sums), mismatch_report(r.refine_sums(), replaced.sums)
    r.light_sampling(0)                        # off, another map, on again: the distribution is the new map's
    r.environment(run.env, u0=run.u0)
    r.light_sampling(48)
    assert r.refine_info()["samples"] == 0 and bits_equal(frame_of(r), first)
    r.refine(2)
    r.light_sampling(32)                       # any other mode discards the refinement
    assert r.refine_info()["samples"] == 0
    r.close()


def test_two_ranks_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, {})
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    run = VW.run("forms")
    m = p.MultiRenderer.MakeRenderer(W, H, SPP, DEPTH, VW.camera(p), run.scene.getWorldPtr(), 2, seed=SEED)
    m.Render()
    plain = m.DownloadRenderbuffer()
    m.light_sampling("env+tree")
    m.Render()
    got = m.DownloadRenderbuffer()
    assert bits_equal(got, run.frame), mismatch_report(got, run.frame)
    with pytest.raises(p.capi.RtError, match="switch light sampling off"):
        m.environment(None)
    m.light_sampling("off")
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), plain) and not bits_equal(plain, got)
    m.close()


# ---- 6. switching -------------------------------------------------------------------------------------------------------------------------------------------
def test_modes_0_16_and_32_keep_their_frames_before_and_after_48(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    run = VW.run("forms")
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, VW.camera(p), run.scene.getWorldPtr(), seed=SEED)
    before = {}
    for mode in (0, 16, 32):
        r.light_sampling(mode)
        assert r.kernel_env_light() == (mode == 32) and r.kernel_light_tree() == (mode == 16)
        before[mode] = frame_of(r)
    r.light_sampling(48)
    assert r.kernel_env_light() and r.kernel_light_tree() and r.light_sampling_info() == {"enabled": True, "lights": 3}
    on = frame_of(r)
    assert bits_equal(on, run.frame), mismatch_report(on, run.frame)
    for mode in (32, 16, 0):
        r.light_sampling(mode)
        assert bits_equal(frame_of(r), before[mode]), mode
    r.light_sampling("env+tree")
    assert bits_equal(frame_of(r), on)
    assert len({on.tobytes()} | {f.tobytes() for f in before.values()}) == 4
    r.close()
    # mode 48 first, on a fresh renderer: the table's image is built by it, and mode 16 then finds it
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, VW.camera(p), run.scene.getWorldPtr(), seed=SEED)
    r.light_sampling(48)
    assert bits_equal(frame_of(r), on)
    for mode in (16, 32, 0):
        r.light_sampling(mode)
        assert bits_equal(frame_of(r), before[mode]), mode
    r.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_each_with_its_own_message(p, monkeypatch):
    setenv(monkeypatch, TW.LDS)
    cam = VW.camera(p)

    def refused(r, pattern, mode_before=0):
        with pytest.raises(p.capi.RtError, match="rt_renderer_light_sampling_enable.*" + pattern) as e:
            r.light_sampling(48)
        assert e.value.code == 1 and r.light_sampling_mode() == mode_before and not r.kernel_env_light() and r.kernel_light_tree() == (mode_before == 16)

    # the world's background is not 2
    for background, mode in ((None, 0), ((0.2, 0.3, 0.4), 1)):
        scene = EW.env_room(p, background, False)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
        refused(r, f"mode 48.*background mode 2.*this world's is {mode}")
        r.light_sampling(16)
        refused(r, "background mode 2", mode_before=16)
        r.close()
    # variants 1, 5 and 6: a background-2 world is refused at creation; any other world's renderer says that its kernel has no light-sampling form
    spheres = p.Scene.book1_final(SEED)
    for variant in (1, 5, 6):
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, spheres.getWorldPtr(), seed=SEED, variant=variant)
        refused(r, f"kernel variant {variant} has no light-sampling form")
        r.close()
    # a queue or wide4 traversal
    for traversal in (1, 2):
        scene = EW.sky_room(p, traversal=traversal)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
        refused(r, "mode 48.*queue or wide4 traversal")
        r.close()
    # a constant medium
    s2 = p.Scene()
    s2.MakeQuad((-15, 0, -15), (40, 0, 0), (0, 0, 40), s2.Lambertian((0.5, 0.5, 0.5)))
    s2.MakeSphere((5, 2, 6), 1.5, s2.Isotropic((0.9, 0.9, 0.9), 0.4))
    s2.MakeQuad((3.5, 6, 3.5), (3, 0, 0), (0, 0, 3), s2.DiffuseLight((8, 8, 8)))
    s2.set_environment(EW.sky_map())
    s2.BuildBVH_SAH()
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s2.getWorldPtr(), seed=SEED)
    refused(r, "mode 48.*constant medium")
    r.close()
    # more than RT_MAX_LIGHTS_TREE lights; a light whose area is lost in the running sum; a table that does not fit beside an LDS-resident image
    def lit_sky(lights, as_list=True):
        s = p.Scene()
        s.MakeQuad((-15, -1, -15), (40, 0, 0), (0, 0, 40), s.Lambertian((0.5, 0.5, 0.5)))
        lights(s, s.DiffuseLight((1, 1, 1)))
        s.set_environment(EW.sky_map())
        s.MakeHittableList() if as_list else s.BuildBVH_SAH()
        return s

    def grid(n):
        def lights(s, emit):
            for i in range(n):
                x, z = 0.1 * (i % 64), 0.1 * (i // 64)
                s.MakeTriangle((x, 0, z), (x + 0.05, 0, z), (x, 0, z + 0.05), emit)
        return lights

    def lost(s, emit):
        s.MakeQuad((-5000, 0, -5000), (10000, 0, 0), (0, 0, 10000), emit)
        s.MakeTriangle((-9000, 0, 0), (-9000, 0, 2), (-9001, 0, 0), emit)
        s.MakeTriangle((9000, 0, 0), (9000, 0, 2), (9001, 0, 0), emit)

    for lights, pattern in ((grid(4097), "mode 48.*more than 4096 lights"), (lost, "mode 48.*lost in the fp32 running sum")):
        scene = lit_sky(lights)   # (kept: the flat world borrows the scene's arrays)
        r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
        refused(r, pattern)
        r.close()
    scene = lit_sky(grid(1000))   # 80 KiB of image, 94 KiB of table
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, scene.getWorldPtr(), seed=SEED)
    assert r.kernel_info()["lds_resident"]
    refused(r, "does not fit beside the scene image in the LDS")
    r.close()
    # no map; an all-black map
    s = VW.run("forms").scene
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, cam, s.getWorldPtr(), seed=SEED)
    first = frame_of(r)
    r.environment(None)
    refused(r, "mode 48.*rt_renderer_environment")
    r.environment(np.zeros((4, 8, 3), F))
    refused(r, "mode 48.*all black")
    # while the mode is on: the map cannot leave, and an all-black successor is refused with the old map left in place
    env, u0 = s.environment()
    r.environment(env, u0=u0)
    r.light_sampling(48)
    on = frame_of(r)
    with pytest.raises(p.capi.RtError, match="rt_renderer_environment.*mode 48.*switch light sampling off") as e:
        r.environment(None)
    assert e.value.code == 1
    with pytest.raises(p.capi.RtError, match="rt_renderer_environment.*mode 48.*all black") as e:
        r.environment(np.zeros((4, 8, 3), F))
    assert e.value.code == 1 and r.environment_info()["width"] == 32 and r.kernel_env_light() and r.kernel_light_tree()
    assert bits_equal(frame_of(r), on) and bits_equal(on, VW.run("forms").frame)
    for bad in (3, 5, 8, 17, 33, 49, 64):
        with pytest.raises(p.capi.RtError, match="on must be 0 \\(off\\), 1 .* or 32 \\(the environment map\\), or 48"):
            r.light_sampling(bad)
    assert r.light_sampling_mode() == 48
    r.light_sampling(0)
    assert bits_equal(frame_of(r), first)
    r.close()


# ---- 8. the C++ program ---------------------------------------------------------------------------------------------------------------------------------------
def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_cpp_app_renders_the_frames_python_renders(p, monkeypatch):
    setenv(monkeypatch, {})
    d = os.path.join(ROOT, "tests", "cpp_env_tree")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", d])
    out = subprocess.check_output([os.path.join(d, "env_tree_app"), str(W), str(H), str(SPP), str(DEPTH)], text=True, timeout=120)
    yy, xx = np.mgrid[0:8, 0:16]
    env = np.stack([0.0625 * xx, 0.125 * yy, np.where((xx == 5) & (yy == 1), 40.0, 0.25)], axis=2).astype(F)   # the map the program computes
    s = p.Scene()
    s.set_environment(env, rotate_y=45.0)
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), s.Lambertian((0.73, 0.73, 0.73)))
    red, steel = s.Lambertian((0.7, 0.3, 0.3)), s.Metal((0.8, 0.8, 0.9), 0.1)
    warm, cold = s.DiffuseLight((8, 7, 5)), s.DiffuseLight((4, 8, 12))
    s.MakeSphere((-2.2, 1.0, 0.0), 1.0, red)
    s.MakeSphere((0.0, 1.0, 0.0), 1.0, steel)
    s.MakeSphere((2.2, 1.0, 0.0), 1.0, red)
    s.MakeQuad((-1, 4, -1), (2, 0, 0), (0, 0, 2), warm)
    s.MakeTriangle((3.5, 1.0, -2.0), (3.5, 3.0, -1.0), (3.6, 1.5, 1.0), cold)
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, p.PinholeCamera((0.5, 2.5, 7), (0, 1.0, 0), (0, 1, 0), 50.0, W / H), s.getWorldPtr(), seed=1984)
    r.light_sampling("env+tree")
    assert r.kernel_env_light() and r.kernel_light_tree() and r.light_sampling_info()["lights"] == 2
    on = frame_of(r)
    r.light_sampling("env")
    env_only = frame_of(r)
    r.close()
    lines = out.strip().splitlines()
    assert lines[0] == f"env tree {W}x{H} spp={SPP} depth={DEPTH} fnv={fnv1a(on.tobytes()):016x}"
    assert lines[1] == "map off: refused (says to switch light sampling off)"
    assert lines[2] == f"env fnv={fnv1a(env_only.tobytes()):016x}"
    assert lines[0].split("fnv=")[1] != lines[2].split("fnv=")[1]
