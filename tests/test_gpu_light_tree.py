"""The light tree and the choice by area on the GPU (mode 16): the 16 LTREE instantiations against the numpy twin of a whole sample
(tests/_light_tree_twin.py, pinned by tests/test_light_tree_cpu.py), bit for bit — every key of _tri_worlds.FORMS on a room with a quad, a sphere and a triangle
light; the shapes where the walk or the search can go wrong, each in an LDS and a global-memory form; a world without triangles; that modes 0, 1, 2 and 4 are
what they were; what switching does; two ranks; the feature buffers; and the expectation against plain path tracing."""
import ctypes as C

import numpy as np
import pytest

import _light_tree_worlds as LW
import _mesh_light_worlds as MW
import _tri_twin as TT
import _tri_worlds as TW
from _common import as_oracle_camera, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu

ENV_KEYS = ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP")


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read when the renderer is made


def make(p, run, mode=16, variant=0):
    r = p.Renderer.MakeRenderer(run.W, run.H, run.spp, run.depth, run.cam, run.scene.getWorldPtr(), seed=run.seed, variant=variant)
    if mode:
        r.light_sampling(mode)
    return r


def test_mode_16_is_accepted_on_a_room_lit_by_65_triangle_lights(p, monkeypatch):
    """fails without the feature: enable(16) is RT_ERR_INVALID there (16 is no mode), and mode 4 refuses this world for having more than 64 lights"""
    set_env(monkeypatch, {})
    run = LW.run("sixty_five")
    r = make(p, run, mode=0)
    with pytest.raises(p.capi.RtError, match="more than 64 lights"):
        r.light_sampling(4)
    assert r.light_sampling_mode() == 0 and not r.kernel_light_tree()
    r.light_sampling(16)
    out = (C.c_uint32 * 2)()
    assert p.lib().rt_renderer_light_sampling_info(r.h, out) == 0 and list(out) == [16, 65]
    assert r.light_sampling_mode() == 16 and r.light_sampling_info() == {"enabled": True, "lights": 65}
    assert r.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 1, 0, 0), nee=1) and r.kernel_triangles() and r.kernel_light_tree()
    for bad in (3, 5, 8, 17, 32):
        with pytest.raises(p.capi.RtError, match="on must be 0 \\(off\\), 1 "):
            r.light_sampling(bad)
    assert r.light_sampling_mode() == 16
    r.refine(run.spp)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling("off")
    assert r.light_sampling_mode() == 0 and not r.kernel_light_tree()
    r.light_sampling("tree")
    assert r.light_sampling_mode() == 16
    r.close()


def test_switching_4_16_4_restarts_the_refinement_and_16_16_does_not(p, monkeypatch):
    set_env(monkeypatch, {})
    run = LW.run("three_kinds")
    four = MW.run("three_kinds")
    r = make(p, run, mode=4)
    r.refine(3)
    assert not r.kernel_light_tree()
    r.light_sampling(16)                      # 4 -> 16: another table, another kernel, another sequence
    assert r.refine_info()["samples"] == 0 and r.light_sampling_info() == {"enabled": True, "lights": 3} and r.kernel_light_tree()
    r.refine(3)
    r.light_sampling(16)                      # 16 -> 16 keeps it
    r.light_sampling("tree")
    assert r.refine_info()["samples"] == 3
    r.refine(1)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling(4)                       # 16 -> 4 discards, and mode 4's kernel and table are still its own
    assert r.refine_info()["samples"] == 0 and not r.kernel_light_tree() and r.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 1, 0, 0), nee=1)
    r.refine(run.spp)
    assert bits_equal(r.refine_sums(), four.sums), mismatch_report(r.refine_sums(), four.sums)
    r.close()


@pytest.fixture(scope="module")
def first_of_world():
    """world name -> (form, sums, frame) of the first form rendered on it: what every later form of that world must repeat on EVERY pixel"""
    return {}


@pytest.mark.parametrize("form", list(TW.FORMS), ids=[TW.form_id(f) for f in TW.FORMS])
def test_every_light_tree_instantiation_is_the_twin(p, monkeypatch, first_of_world, form):
    """All 16 RT_KERNEL_LIGHT_TREE keys, each reached by its recipe of _tri_worlds.FORMS on the room with a quad light, a sphere lamp and a triangle light: frame and
    refinement sums against the twin, two passes, uneven steps.  An EXT = 2 room holds an image-textured triangle: the twin follows every other pixel, and on the
    rest every form of the room gives the bits of the first one rendered."""
    world, exact, ext, big, wide = form
    variant, env = TW.FORMS[form]
    name = "three_kinds" + ("_textured" if ext == 2 else "") + ("_list" if world == TW.LIST else "")
    run = LW.run(name)
    keep = run.pixel_followed
    assert run.followed if ext == 1 else 0.8 < keep.mean() < 1.0
    set_env(monkeypatch, env)
    monkeypatch.setenv("RT06_PASS_SPP", "3")   # a cut inside the frame: two passes
    r = make(p, run, variant=variant)
    assert r.light_sampling_info() == {"enabled": True, "lights": 3} and r.light_sampling_mode() == 16
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1) and r.kernel_triangles() and r.kernel_light_tree()
    r.Render()
    img = r.DownloadRenderbuffer()
    assert bits_equal(img[keep], run.frame[keep]), mismatch_report(img[keep], run.frame[keep])
    r.refine(1)
    r.refine(3)   # uneven steps
    sums = r.refine_sums()
    r.close()
    assert bits_equal(sums[keep], run.sums[keep]), mismatch_report(sums[keep], run.sums[keep])
    assert np.isfinite(sums[keep]).all()
    if ext == 2:
        first_id, first_sums, first_img = first_of_world.setdefault(name, (TW.form_id(form), sums, img))
        assert bits_equal(sums, first_sums) and bits_equal(img, first_img), f"against {first_id}: " + mismatch_report(sums, first_sums)


@pytest.mark.parametrize("big", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("name", LW.SHAPE_WORLDS)
def test_the_shapes_where_the_walk_or_the_search_can_go_wrong_are_the_twin_bit_for_bit(p, monkeypatch, name, big):
    """n_l = 1 (the root is a leaf, no draw), 2, 3 (unbalanced), 20 (a closed mesh: both crossings), 64, 65, 320; the centroid tie; a drawn sphere lost on its
    silhouette; the clamped last index; areas 1 : 10^4 (tests/test_light_tree_cpu.py holds each world to what it is there for)"""
    run = LW.run(name)
    assert run.followed
    if name == "silhouette":
        assert run.stats["tree_sphere_uncredited"] > 0
    if name == "clamped_last_index":
        assert run.stats["index_clamped"] > 0
    set_env(monkeypatch, TW.NARROW if big else TW.LDS)
    r = make(p, run)
    assert r.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 1, big, 0), nee=1) and r.kernel_triangles() and r.kernel_light_tree()
    assert r.light_sampling_info() == {"enabled": True, "lights": run.lights}
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.refine(run.spp)
    sums = r.refine_sums()
    r.close()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(frame, run.frame) and np.isfinite(sums).all() and (sums[..., :3] > 0).any(axis=2).mean() > 0.5


@pytest.mark.parametrize("big", [0, 1], ids=["lds", "global"])
def test_a_world_without_triangles_runs_the_light_tree_family(p, monkeypatch, big):
    """quad and sphere lamps only: n_plain_quads == n_quads is a valid world of the triangle family, which mode 16 alone puts it in"""
    run = LW.run("no_triangles")
    set_env(monkeypatch, TW.NARROW if big else TW.LDS)
    r = make(p, run, mode=0)
    assert not r.kernel_triangles()
    r.light_sampling(2)
    assert not r.kernel_triangles() and not r.kernel_light_tree()
    r.light_sampling(16)
    assert r.kernel_triangles() and r.kernel_light_tree() and r.light_sampling_info() == {"enabled": True, "lights": 2}
    r.refine(run.spp)
    assert bits_equal(r.refine_sums(), run.sums), mismatch_report(r.refine_sums(), run.sums)
    r.light_sampling(0)
    assert not r.kernel_triangles()
    r.close()


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_modes_0_1_2_4_are_what_mesh_light_twin_says(p, monkeypatch, mode):
    set_env(monkeypatch, {})
    old = MW.run("three_kinds", mode)
    run = LW.run("three_kinds")
    r = make(p, run, mode=16)     # through mode 16 and back: its table and kernel change nothing of the others
    r.refine(1)
    r.light_sampling(mode)
    assert r.light_sampling_info()["lights"] == {0: 1, 1: 1, 2: 2, 4: 3}[mode] and r.refine_info()["samples"] == 0 and not r.kernel_light_tree()
    r.refine(run.spp)
    assert bits_equal(r.refine_sums(), old.sums), mismatch_report(r.refine_sums(), old.sums)
    r.close()


def test_two_ranks_in_mode_16_render_the_single_renderers_frame(p, monkeypatch):
    set_env(monkeypatch, {})
    run = LW.run("mesh_lamp")
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    m = p.MultiRenderer.MakeRenderer(run.W, run.H, run.spp, run.depth, run.cam, run.scene.getWorldPtr(), 2, seed=run.seed)
    with pytest.raises(p.capi.RtError, match="must be 0"):
        m.light_sampling(8)
    m.light_sampling("tree")
    m.Render()
    assert bits_equal(m.DownloadRenderbuffer(), run.frame), mismatch_report(m.DownloadRenderbuffer(), run.frame)
    m.refine(run.spp)
    assert bits_equal(m.DownloadRenderbuffer(), run.frame)
    m.close()


def test_feature_buffers_are_unchanged_by_the_mode(p, monkeypatch):
    set_env(monkeypatch, {})
    run = LW.run("three_kinds")
    exp = TT.first_hit_sums(run.world, as_oracle_camera(run.cam), run.W, run.H, run.spp, run.seed)
    got = {}
    for mode in (0, 16):
        r = make(p, run, mode=mode)
        r.enable_aov()
        r.refine(1)
        r.refine(run.spp - 1)
        got[mode] = r.aov_sums()
        r.close()
    assert bits_equal(got[16], got[0]), mismatch_report(got[16], got[0])
    assert bits_equal(got[16][..., 0:4], exp[..., 0:4]) and bits_equal(got[16][..., 7], exp[..., 4])


def test_mode_16_and_plain_path_tracing_agree_in_expectation_on_the_icosphere_lamp(p, monkeypatch):
    """16 seeds x 256 spp per mode, 32 x 32, depth 8, a room lit by an emissive icosphere(1) (80 lights): the frame-mean radiance per channel of mode 0 and of
    mode 16 differ by at most 5 sqrt(SE0^2 + SE16^2), the standard errors taken from the spread over the 16 seeds (§19's rule and sizes).  Measured on one
    MI355X: MEASURED below."""
    set_env(monkeypatch, {})
    scene = LW.scene("icosphere1")
    cam = TW.camera(p)
    means = {0: [], 16: []}
    for mode in (0, 16):
        for seed in range(16):
            r = p.Renderer.MakeRenderer(32, 32, 256, 8, cam, scene.getWorldPtr(), seed=1000 + seed)
            if mode:
                r.light_sampling(mode)
                assert r.light_sampling_info()["lights"] == 80
            r.refine(256)   # the linear sums: the framebuffer is clamped and square-rooted, and its mean is not the mean radiance
            means[mode].append(r.refine_sums()[..., :3].astype(np.float64).mean(axis=(0, 1)) / 256.0)
            r.close()
    m0, m16 = np.mean(means[0], axis=0), np.mean(means[16], axis=0)
    se0, se16 = np.std(means[0], axis=0, ddof=1) / 4.0, np.std(means[16], axis=0, ddof=1) / 4.0
    bound = 5 * np.sqrt(se0 ** 2 + se16 ** 2)
    print(f"icosphere1 16 x 256 spp: mode 0 mean {m0} se {se0}; mode 16 mean {m16} se {se16}; |diff| / bound {np.abs(m0 - m16) / bound}")
    assert (se0 < 0.01 * m0).all()   # plain path tracing knows the mean well: the check is sharp
    assert (np.abs(m0 - m16) <= bound).all()


MEASURED = """one MI355X, seeds 1000..1015, frame-mean radiance (R, G, B) from the linear refinement sums (EXPERIMENTS.md E11):
mode 0: mean 0.90721172 0.7085352 0.53541116, SE 0.00056209 0.00039747 0.00029774 (0.06 % of the mean)
mode 16: mean 0.90730727 0.7079538 0.53516978, SE 0.00035077 0.00027738 0.00021502
|difference| / (5 sqrt(SE0^2 + SE16^2)): 0.029 0.240 0.131"""
