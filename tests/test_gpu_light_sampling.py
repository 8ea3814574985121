"""Light sampling on the GPU: the NEE instantiations of render_kernel_stream against the numpy twin of a whole sample
(tests/_nee_twin.py, pinned to the oracle by tests/test_light_sampling_cpu.py), bit for bit — every one of the 16 forms of tests/_nee_worlds.py's
matrix, each identified by Renderer.kernel_form(), and the estimator's edges (16 lights, two lights on one ray, lights behind surfaces, several
passes, moving spheres); what switching it on and off does to a renderer's state; and that it leaves every other path — materials that do not
sample, feature buffers, the multi-GPU driver — with the bits it had."""
import numpy as np
import pytest

import _nee_twin as T
import _nee_worlds as NW
import _oracle as O
from _common import as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, pkg

pytestmark = pytest.mark.gpu

SEED = 1984


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def twin_samples(scene, cam, W, H, spp, depth, on=True):
    return T.frame_samples(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, spp, depth, SEED, light_sampling=on)


@pytest.fixture(scope="module")
def cornell(p):
    """the Cornell box at 32x32, depth 6, and the twin's four samples per pixel with sampling on (computed once, never modified)"""
    W = H = 32
    scene = config_scene(p, "cornell_box")
    cam = config_cameras(p, "cornell_box", W, H)
    samples, followed = twin_samples(scene, cam, W, H, 4, 6)
    assert followed.all()
    samples.setflags(write=False)
    return scene, cam, W, H, 6, samples


def make(p, scene, cam, W, H, spp, depth, on=True, variant=0, seed=SEED):
    r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, scene.getWorldPtr(), seed=seed, variant=variant)
    if on:
        r.light_sampling(True)
    return r


@pytest.mark.parametrize("spp", [1, 4])
def test_cornell_box_is_the_twin_bit_for_bit_however_the_samples_are_cut(p, cornell, spp):
    scene, cam, W, H, depth, samples = cornell
    sums = T.in_order_sums(samples[:, :, :spp])
    frame = T.resolve(sums, spp)
    r = make(p, scene, cam, W, H, spp, depth)
    assert r.light_sampling_info() == {"enabled": True, "lights": 1}
    r.Render()
    img = r.DownloadRenderbuffer()
    assert bits_equal(img, frame), mismatch_report(img, frame)
    r.refine(spp)
    assert bits_equal(r.DownloadRenderbuffer(), frame) and bits_equal(r.refine_sums(), sums), mismatch_report(r.refine_sums(), sums)
    r.refine_reset()
    for _ in range(spp):
        r.refine(1)
    assert bits_equal(r.DownloadRenderbuffer(), frame) and bits_equal(r.refine_sums(), sums), mismatch_report(r.refine_sums(), sums)
    r.close()
    assert (samples[:, :, :spp].sum(axis=(2, 3)) > 0).mean() > 0.5   # a sampled light reaches most pixels, even at this sample count


two_light_room = NW.two_light_room


def test_two_light_room_is_the_twin_in_the_lds_and_the_global_memory_form(p, monkeypatch):
    W = H = 32
    spp, depth = 4, 8
    scene = two_light_room(p)
    cam = p.PinholeCamera((5, 5, 0.5), (5, 4, 10), (0, 1, 0), 80.0, W / H)
    samples, followed = twin_samples(scene, cam, W, H, spp, depth)
    pixel_followed = followed.all(axis=2)
    assert 0.5 < pixel_followed.mean() < 1.0   # the dielectric sphere is in view: there the twin stops, elsewhere it goes all the way
    sums = T.in_order_sums(np.where(followed[..., None], samples, 0))
    got = {}
    for form in ("lds", "global"):
        if form == "global":
            monkeypatch.setenv("RT06_FORCE_BIG", "1")   # as tests/test_gpu_parity.py forces the global-memory path
        r = make(p, scene, cam, W, H, spp, depth)
        assert r.kernel_info()["lds_resident"] == (form == "lds") and r.light_sampling_info() == {"enabled": True, "lights": 2}
        r.refine(spp)
        got[form] = (r.refine_sums(), r.DownloadRenderbuffer())
        r.close()
        assert bits_equal(got[form][0][pixel_followed], sums[pixel_followed]), form + ": " + mismatch_report(got[form][0][pixel_followed], sums[pixel_followed])
    assert bits_equal(got["lds"][0], got["global"][0]) and bits_equal(got["lds"][1], got["global"][1])
    assert np.isfinite(got["lds"][0][pixel_followed]).all()


def test_a_world_without_lambertian_hits_draws_nothing_more(p):
    """metal, dielectric and one quad light only: no hit ever samples, so every per-pixel sum keeps the bits it has with sampling off"""
    s = p.Scene()
    mirror, glass, light = s.Metal((0.8, 0.7, 0.6), 0.2), s.Dielectric((1, 1, 1), 1.5), s.DiffuseLight((6, 6, 6))
    s.MakeQuad((-6, -0.5, -8), (12, 0, 0), (0, 0, 12), mirror)
    s.MakeQuad((-1, 3, -3), (2, 0, 0), (0, 0, 2), light)
    s.MakeSphere((-1, 0.5, -2), 1.0, glass)
    s.MakeSphere((1.2, 0.5, -2.5), 1.0, mirror)
    s.BuildBVH_TopDown()
    W, H, spp, depth = 40, 24, 4, 12
    cam = p.PinholeCamera((0, 1.5, 2), (0, 0.5, -2), (0, 1, 0), 70.0, W / H)
    sums = []
    for on in (False, True):
        r = make(p, s, cam, W, H, spp, depth, on=on)
        r.refine(spp)
        sums.append(r.refine_sums())
        r.close()
    assert bits_equal(sums[0], sums[1]), mismatch_report(sums[1], sums[0])
    assert (sums[0][..., :3] > 0).any(axis=2).mean() > 0.5


def test_enable_discards_the_refinement_and_disable_restores_the_plain_renderer(p, cornell):
    scene, cam, W, H, depth, samples = cornell
    plain = make(p, scene, cam, W, H, 4, depth, on=False)
    plain.Render()
    plain_frame = plain.DownloadRenderbuffer()
    plain.refine(4)
    plain_sums = plain.refine_sums()
    plain.close()
    r = make(p, scene, cam, W, H, 4, depth, on=False)
    assert r.light_sampling_info() == {"enabled": False, "lights": 1}
    r.refine(3)
    assert r.refine_info()["samples"] == 3
    r.light_sampling(False)                       # nothing changes: the refinement goes on
    assert r.refine_info()["samples"] == 3
    r.light_sampling(True)                        # another estimator: what was accumulated belongs to another sequence
    assert r.refine_info()["samples"] == 0 and r.light_sampling_info()["enabled"]
    r.refine(4)
    assert bits_equal(r.refine_sums(), T.in_order_sums(samples)) and not bits_equal(r.refine_sums(), plain_sums)
    r.light_sampling(False)
    assert r.refine_info()["samples"] == 0 and not r.light_sampling_info()["enabled"]
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), plain_frame)
    r.refine(4)
    assert bits_equal(r.refine_sums(), plain_sums)
    r.close()


def test_variants_without_a_light_sampling_form_are_refused(p, cornell):
    scene, cam, W, H, depth, _ = cornell
    r = make(p, scene, cam, W, H, 1, depth, on=False, variant=1)
    with pytest.raises(p.capi.RtError, match="variant 1") as e:
        r.light_sampling(True)
    assert e.value.code == 1
    r.close()
    plain = config_scene(p, "book1_final")   # a BVH world of the reference's feature set: variants 5 and 6 take it
    for variant in (5, 6):
        r = make(p, plain, config_cameras(p, "book1_final", W, H), W, H, 1, depth, on=False, variant=variant)
        with pytest.raises(p.capi.RtError, match=f"variant {variant}"):
            r.light_sampling(True)
        assert r.light_sampling_info() == {"enabled": False, "lights": 0}
        r.close()
    r = make(p, plain, config_cameras(p, "book1_final", W, H), W, H, 1, depth, on=False)
    with pytest.raises(p.capi.RtError, match="no quad light"):
        r.light_sampling(True)
    r.Render()   # a refused enable leaves the renderer as it was
    r.close()


def test_feature_buffers_keep_their_bits_and_the_denoiser_runs(p, cornell):
    scene, cam, W, H, depth, samples = cornell
    aov = []
    for on in (False, True):
        r = make(p, scene, cam, W, H, 4, depth, on=on)
        r.enable_aov()
        r.refine(4)
        aov.append(r.aov_sums())
        if on:
            assert bits_equal(r.refine_sums(), T.in_order_sums(samples))
            den = r.denoise()
            assert den.shape == (H, W, 4) and np.isfinite(den).all() and den[..., :3].max() > 0
        r.close()
    assert bits_equal(aov[0], aov[1])


def test_two_ranks_render_the_single_renderers_frame(p, cornell, monkeypatch):
    scene, cam, W, H, depth, samples = cornell
    frame = T.resolve(T.in_order_sums(samples), 4)
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    m = p.MultiRenderer.MakeRenderer(W, H, 4, depth, cam, scene.getWorldPtr(), 2, seed=SEED)
    m.light_sampling(True)
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), frame)
    m.refine(4)
    assert bits_equal(m.DownloadRenderbuffer(), frame)
    m.close()
    r = make(p, scene, cam, W, H, 4, depth)
    r.Render()
    assert bits_equal(r.DownloadRenderbuffer(), frame)
    r.close()


def test_noise_figure_falls_on_the_cornell_box(p):
    """64x64, 16 spp, depth 50: the relative standard error of the frame's mean luminance, strictly lower with sampling on (measured: EXPERIMENTS.md E7)"""
    W = H = 64
    scene = config_scene(p, "cornell_box")
    cam = config_cameras(p, "cornell_box", W, H)
    noise = {}
    for on in (False, True):
        r = make(p, scene, cam, W, H, 16, 50, on=on)
        r.refine(16)
        noise[on] = r.noise()
        r.close()
    print(f"noise figure at 64x64x16, depth 50: off {noise[False]:.4f}, on {noise[True]:.4f}, ratio {noise[True] / noise[False]:.3f}")
    assert np.isfinite(noise[True]) and noise[True] < noise[False]


# ------------------------------------------------------------------------------------------------
# every light-sampling instantiation (tests/_nee_worlds.py: FORMS), identified by kernel_form()
# ------------------------------------------------------------------------------------------------
def set_form_env(monkeypatch, env):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read when the renderer is made


def render_run(p, run, variant, expect_form):
    """(sums, frame) of a renderer on `run`'s world with sampling on, after it is shown to launch `expect_form` on the world's lights"""
    r = make(p, run.scene, run.cam, run.W, run.H, run.spp, run.depth, variant=variant, seed=run.seed)
    reached = r.kernel_form()
    print(f"{run.name}, variant {variant}: kernel_form {reached}")
    assert reached == expect_form, (reached, expect_form)
    assert r.light_sampling_info() == {"enabled": True, "lights": run.lights}
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.refine(run.spp)
    sums = r.refine_sums()
    r.close()
    assert bits_equal(frame, T.resolve(sums, run.spp)), mismatch_report(frame, T.resolve(sums, run.spp))
    return sums, frame


@pytest.fixture(scope="module")
def first_of_world():
    """world name -> (form id, sums, frame) of the first form of the matrix rendered on it: what every later form of that world must repeat"""
    return {}


@pytest.mark.parametrize("form", list(NW.FORMS), ids=NW.form_id)
def test_every_light_sampling_form_is_reached_and_is_the_twin(p, monkeypatch, first_of_world, form):
    """Reached: kernel_form() is the tuple, with nee = 1.  Correct: the sums are the twin's on every pixel the twin followed.  Consistent: the frame
    is the resolve of the sums (render_run).  Pixels the twin does not follow (dielectric, noise, image): the same bits in every form of the world."""
    name, variant, env = NW.FORMS[form]
    run = NW.run(name)
    set_form_env(monkeypatch, env)
    sums, frame = render_run(p, run, variant, NW.kernel_form_of(form))
    f = run.followed
    assert bits_equal(sums[f], run.sums[f]), mismatch_report(sums[f], run.sums[f])
    assert np.isfinite(sums[f]).all()
    first_id, first_sums, first_frame = first_of_world.setdefault(name, (NW.form_id(form), sums, frame))
    assert bits_equal(sums, first_sums), f"against {first_id}: " + mismatch_report(sums, first_sums)
    assert bits_equal(frame, first_frame), f"against {first_id}: " + mismatch_report(frame, first_frame)


def test_irregular_box_coordinates_take_the_verbatim_light_sampling_form(p, monkeypatch):
    """the room with a box coordinate outside the fast-division class (tests/test_gpu_parity.py's 1e-15): variant 0 falls back to EXACT, sampling on"""
    run = NW.run("irregular_room")
    nodes, _, _ = run.scene.arrays()
    assert np.any((np.abs(nodes["min"]) > 0) & (np.abs(nodes["min"]) < 2.0 ** -40))
    set_form_env(monkeypatch, NW.LDS)
    sums, _ = render_run(p, run, 0, NW.kernel_form_of((NW.BVH, 1, 1, 0, 0)))
    f = run.followed
    assert bits_equal(sums[f], run.sums[f]), mismatch_report(sums[f], run.sums[f])
    assert np.isfinite(sums[f]).all()


# ------------------------------------------------------------------------------------------------
# the estimator's edges (what each world exercises: tests/test_light_sampling_cpu.py holds the twin's counts to it)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("name", NW.EDGE_WORLDS)
def test_estimator_edges_are_the_twin_bit_for_bit(p, monkeypatch, name, big):
    """16 lights (the index draw), and under a seed that draws a uniform of 1 for the index (its clamp); two lights on one ray (two terms in pdf_light); lights below and in the plane of the surface that
    samples them (pdf_cos == 0, quad::hit's |denom| < 1e-8): every pixel is followed, so every sum is compared"""
    run = NW.run(name)
    assert run.followed.all()
    set_form_env(monkeypatch, NW.NARROW if big else NW.LDS)
    sums, _ = render_run(p, run, 0, NW.kernel_form_of((NW.BVH, 0, 1, big, 0)))
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert np.isfinite(sums).all() and (sums[..., :3] > 0).any(axis=2).mean() > 0.5


@pytest.mark.parametrize("pass_spp", [1, 3])
def test_several_passes_with_sampling_on_are_the_one_pass_frame(p, cornell, monkeypatch, pass_spp):
    scene, cam, W, H, depth, samples = cornell
    set_form_env(monkeypatch, {})
    one = make(p, scene, cam, W, H, 4, depth)
    assert one.pass_info()["n_passes"] == 1
    one.Render()
    one_frame = one.DownloadRenderbuffer()
    one.refine(4)
    one_sums = one.refine_sums()
    one.close()
    assert bits_equal(one_sums, T.in_order_sums(samples))
    monkeypatch.setenv("RT06_PASS_SPP", str(pass_spp))
    r = make(p, scene, cam, W, H, 4, depth)
    info = r.pass_info()
    assert info["pass_spp"] == pass_spp and info["n_passes"] == -(-4 // pass_spp) > 1   # the passes really were cut
    r.Render()
    frame = r.DownloadRenderbuffer()
    assert bits_equal(frame, one_frame), mismatch_report(frame, one_frame)
    r.refine(4)
    assert bits_equal(r.refine_sums(), one_sums), mismatch_report(r.refine_sums(), one_sums)
    assert bits_equal(r.DownloadRenderbuffer(), one_frame)
    r.close()


def test_moving_spheres_under_a_quad_light_agree_across_forms_and_variants(p, monkeypatch):
    """a motion-blur camera is outside the twin's scope: the three memory forms and variants 2 and 3 must give the same sums, sampling must change
    them, and switching it off must restore the plain oracle frame"""
    W = H = 32
    spp, depth = 4, 8
    scene = NW.moving_world(p)
    cam = p.MotionBlurCamera((0, 1.2, 2.5), (0, 0.2, -1.2), (0, 1, 0), 60.0, W / H, 0.0, 1.0)
    plain, _ = O.render(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, spp, depth)
    first = None
    for env, (big, wide) in ((NW.LDS, (0, 0)), (NW.NARROW, (1, 0)), (NW.WIDE, (1, 1))):
        set_form_env(monkeypatch, env)
        for variant in (3, 2):
            r = make(p, scene, cam, W, H, spp, depth, variant=variant)
            assert r.kernel_form() == NW.kernel_form_of((NW.BVH, int(variant == 2), 1, big, wide)) and r.light_sampling_info() == {"enabled": True, "lights": 1}
            r.refine(spp)
            sums = r.refine_sums()
            if first is None:
                first = sums
                assert np.isfinite(sums).all() and (sums[..., :3] > 0).any(axis=2).mean() > 0.5
            assert bits_equal(sums, first), f"variant {variant}, big {big}, wide {wide}: " + mismatch_report(sums, first)
            r.light_sampling(False)
            assert r.kernel_form() == NW.kernel_form_of((NW.BVH, int(variant == 2), 1, big, wide), nee=0)
            r.Render()
            frame = r.DownloadRenderbuffer()
            assert bits_equal(frame, plain), f"variant {variant}, big {big}, wide {wide}, sampling off: " + mismatch_report(frame, plain)
            r.refine(spp)
            assert not bits_equal(r.refine_sums(), first)
            r.close()


def test_kernel_form_names_the_baseline_and_the_exchange_kernel(p, cornell):
    scene, cam, W, H, depth, _ = cornell
    r = make(p, scene, cam, W, H, 1, depth, on=False, variant=1)
    assert r.kernel_form() == dict(NW.kernel_form_of((NW.BVH, 0, 0, 0, 0), nee=0), kernel="baseline")
    r.close()
    plain = config_scene(p, "book1_final")
    r = make(p, plain, config_cameras(p, "book1_final", W, H), W, H, 1, depth, on=False, variant=5)
    assert r.kernel_form() == dict(NW.kernel_form_of((NW.BVH, 0, 0, 0, 0), nee=0), kernel="xchg")
    r.close()
    r = make(p, plain, config_cameras(p, "book1_final", W, H), W, H, 1, depth, on=False, variant=6)
    assert r.kernel_form() == dict(NW.kernel_form_of((NW.BVH, 0, 0, 0, 0), nee=0), tol=1)
    r.close()
