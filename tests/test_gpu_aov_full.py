"""The feature pass's third mode on the GPU (RT_AOV_FULL): the feature sums against the numpy twin (tests/_aov_full_twin.py, whose first trace is
the walk-with-tape that tests/test_path_twin_oracle_cpu.py holds to the CPU oracle) on the cutout room, the fog room and the room with both
(tests/_aov_full_worlds.py; tests/test_aov_full_cpu.py shows that they reach what the mode is for), on every walk a medium streams on, on LDS and global-memory
forms, with and without texture coordinates and vertex normals; the contract of the refinement, the table coming and going, ranks, the neutral cases, the
untouched colour path, the filter and the refusals.  Frames are 24 x 16 at 8 samples; every comparison is bit for bit."""
import numpy as np
import pytest

import _aov_full_twin as FT
import _aov_full_worlds as FW
import _aov_tex_twin as AT
import _tex_worlds as XW
from _common import as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = FW.W, FW.H, FW.SPP, FW.DEPTH, FW.SEED
MEMORY = {"lds": {}, "global": {"RT06_FORCE_BIG": "1"}}
TWINS = {}


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


def twin(p, spp=SPP, cutouts="scene", **room):
    """the twin's sums of FW.room(**room), computed once per room and left unchanged; cutouts=None: the same world without its table"""
    key = (spp, cutouts is None) + tuple(sorted(room.items()))
    if key not in TWINS:
        scene = FW.room(p, **room)
        tb = FW.tables(scene)
        if cutouts is None:
            tb["cutouts"] = None
        TWINS[key] = FT.sums(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(FW.camera(p)), W, H, spp, SEED, **tb)
        TWINS[key].setflags(write=False)
    return TWINS[key]


def renderer(p, scene, spp=SPP, cam=None, w=W, h=H, **kw):
    return p.Renderer.MakeRenderer(w, h, spp, DEPTH, cam or FW.camera(p), scene.getWorldPtr(), seed=SEED, **kw)


def full_sums(p, scene, steps=(SPP,), max_samples=0, **kw):
    r = renderer(p, scene, **kw)
    r.enable_aov(max_samples, full=True)
    assert r.aov_mode() == "full" and p.capi.AOV_FULL == 2
    for n in steps:
        r.refine(n)
    assert r.aov_info()["samples"] == (max_samples or sum(steps))
    got = r.aov_sums()
    r.close()
    return got


# ---- 1. mode 2 against the twin, every pixel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [False, True], ids=["flat", "smooth"])
@pytest.mark.parametrize("uvs", [True, False], ids=["uv", "planar"])
@pytest.mark.parametrize("memory", list(MEMORY))
@pytest.mark.parametrize("walk", ["stack", "list"])
def test_the_cutout_room_is_the_twin(p, monkeypatch, walk, memory, uvs, normals):
    """Without the feature this fails at the enable: mode 2 is an unknown mode."""
    setenv(monkeypatch, MEMORY[memory])
    scene = FW.room(p, walk=walk, uvs=uvs, normals=normals)
    r = renderer(p, scene)
    assert r.kernel_cutout() and r.cutouts_info()["enabled"] and r.kernel_form()["big"] == (1 if memory == "global" else 0)
    assert r.texture_coords_info()["enabled"] == uvs and r.shading_normals_info()["enabled"] == normals
    r.close()
    got, want = full_sums(p, scene), twin(p, walk=walk, uvs=uvs, normals=normals)
    assert bits_equal(got, want), mismatch_report(got, want)
    solid = twin(p, walk=walk, uvs=uvs, normals=normals, opaque=True)
    assert ((got.view(np.uint32) != solid.view(np.uint32)).any(axis=2)).sum() > 100   # the holes are seen through


@pytest.mark.parametrize("memory", list(MEMORY))
@pytest.mark.parametrize("walk", ["stack", "list", "queue", "wide4"])
def test_the_fog_room_is_the_twin_on_every_walk_a_medium_streams_on(p, monkeypatch, walk, memory):
    """The queue and the four-wide walk, which no numpy twin restates, are held to the sums of the stack walk's twin: one medium draws one uniform whatever the
    order of the tests (tests/test_aov_full_cpu.py: the list's order and the tree's agree on every sample of this room)."""
    setenv(monkeypatch, MEMORY[memory])
    scene = FW.room(p, walk=walk, masks=False, fog=True)
    wf = scene.getWorldPtr()
    assert wf.traversal == FW.WALKS[walk] and wf.kind == (1 if walk == "list" else 0)
    got, want = full_sums(p, scene), twin(p, walk="list" if walk == "list" else "stack", masks=False, fog=True)
    assert bits_equal(got, want), mismatch_report(got, want)


def test_the_tree_walk_streams_no_medium_and_is_mode_1_there(p):
    """A bvh_node tree streams only within the reference's feature set: with a medium it renders on the baseline kernel, which keeps no records (refused, in the
    words of variant 1).  On a tree that streams the TREE form carries an RNG nothing draws from, and gives mode 1's bits and the twin's."""
    import test_gpu_aov_textured as T1
    foggy = FW.fog_tree(p)   # (the flat world borrows the scene's arrays: the scene stays alive)
    r = p.Renderer.MakeRenderer(W, H, SPP, DEPTH, p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, W / H), foggy.getWorldPtr(), seed=SEED)
    with pytest.raises(p.capi.RtError, match="rt_renderer_aov_enable_mode.*variant 1"):
        r.enable_aov(full=True)
    r.close()
    scene, cam = T1.sphere_tree(p), p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, W / H)
    assert scene.getWorldPtr().kind == 2
    got = full_sums(p, scene, cam=cam)
    r = renderer(p, scene, cam=cam)
    r.enable_aov(textured=True)
    r.refine(SPP)
    mode1 = r.aov_sums()
    r.close()
    want = AT.sums(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, SPP, SEED, True)[0]
    assert bits_equal(got, mode1) and bits_equal(got, want), mismatch_report(got, want)


@pytest.mark.parametrize("memory", list(MEMORY))
@pytest.mark.parametrize("walk", ["stack", "list"])
def test_a_room_with_a_mask_and_a_medium_is_the_twin(p, monkeypatch, walk, memory):
    setenv(monkeypatch, MEMORY[memory])
    got, want = full_sums(p, FW.room(p, walk=walk, fog=True)), twin(p, walk=walk, fog=True)
    assert bits_equal(got, want), mismatch_report(got, want)
    assert not bits_equal(got, twin(p, walk=walk)) and not bits_equal(got, twin(p, walk=walk, masks=False, fog=True))


# ---- 2. sessions ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_uneven_steps_a_limit_inside_a_pass_and_the_table_off_on_off(p, monkeypatch):
    setenv(monkeypatch, {"RT06_PASS_SPP": "2"})   # read at creation: steps span several passes; 5 ends inside one
    scene = FW.room(p, fog=True)
    one = twin(p, fog=True)
    stepped = full_sums(p, scene, steps=(2, 3, 3), spp=2)
    assert bits_equal(stepped, one), mismatch_report(stepped, one)
    limited = full_sums(p, scene, steps=(3, 5), max_samples=5, spp=2)
    five = twin(p, spp=5, fog=True)
    assert bits_equal(limited, five), mismatch_report(limited, five)
    table = scene.cutouts()
    r = renderer(p, scene, spp=2)
    r.enable_aov(full=True)
    r.refine(3)
    for k, cut in enumerate((None, table, None)):   # off, on, off: accepted under mode 2, and colour and features restart together
        r.cutouts(cut)
        assert r.aov_info()["samples"] == 0 and r.refine_info()["samples"] == 0 and r.aov_mode() == "full" and r.kernel_cutout() == (cut is not None)
        r.refine(3)
        r.refine(5)
        got, want = r.aov_sums(), twin(p, fog=True, cutouts=None) if cut is None else one
        assert bits_equal(got, want), (k, mismatch_report(got, want))
    r.cutouts(None)   # unchanged: the refinement goes on
    assert r.aov_info()["samples"] == SPP
    r.close()
    assert not bits_equal(one, twin(p, fog=True, cutouts=None))


def test_two_rank_shards_accumulate_their_own_pixels(p):
    """As in tests/test_gpu_aov_textured.py: each rank of two accumulates its own pixels and says so; a shard's buffers are not a frame"""
    scene = FW.room(p, fog=True)
    for rank in (0, 1):
        shard = renderer(p, scene, spp=4, rank=rank, world_size=2)
        shard.enable_aov(full=True)
        shard.refine(4)
        assert shard.aov_info()["samples"] == 4 and shard.aov_mode() == "full" and shard.aov_info()["bytes"] > 0
        with pytest.raises(p.capi.RtError, match="shard"):
            shard.aov_sums()
        with pytest.raises(p.capi.RtError, match="shard"):
            shard.denoise()
        shard.close()


# ---- 3. neutral cases ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", ["routing", "riders-stack", "riders-list", "marble", "lane-queue"])
def test_on_a_world_mode_1_accepts_mode_2_gives_mode_1s_bits(p, world):
    import test_gpu_aov_textured as T1
    w, h = T1.W, T1.H
    if world == "routing":
        scene, cam = XW.routing_room(p), XW.camera(p)
    elif world.startswith("riders"):   # vertex normals, texture coordinates and the table together
        scene, cam = XW.riders_room(p, as_list=world.endswith("list"), env=False), XW.camera(p)
    elif world == "marble":
        scene, cam = T1.marble_world(p), p.PinholeCamera((0.5, 2.5, 7), (0, 1.0, 0), (0, 1, 0), 50.0, w / h)
    else:
        scene, cam = T1.lane_walk_world(p, 1), p.PinholeCamera((0.5, 2.5, 7), (0, 1.0, 0), (0, 1, 0), 50.0, w / h)
    sums = {}
    for mode in ("textured", "full"):
        r = renderer(p, scene, spp=4, cam=cam, w=w, h=h)
        r.enable_aov(**{mode: True})
        r.refine(4)
        sums[mode] = r.aov_sums()
        r.close()
    assert bits_equal(sums["full"], sums["textured"]), mismatch_report(sums["full"], sums["textured"])
    assert T1.n_albedos(sums["full"]) > 6


@pytest.mark.parametrize("walk", ["stack", "list"])
def test_a_table_of_opaque_masks_gives_the_bits_of_the_world_without_a_table(p, walk):
    scene = FW.room(p, walk=walk, opaque=True)
    r = renderer(p, scene)
    r.enable_aov(full=True)
    r.refine(SPP)
    opaque = r.aov_sums()
    assert r.kernel_cutout()
    r.cutouts(None)
    r.refine(SPP)
    bare = r.aov_sums()
    r.close()
    assert bits_equal(opaque, bare), mismatch_report(opaque, bare)
    want = twin(p, walk=walk, opaque=True)
    assert bits_equal(opaque, want), mismatch_report(opaque, want)


# ---- 4. the colour path and the filter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", ["cutout", "fog"])
def test_the_colour_frame_is_untouched_and_denoise_is_the_numpy_filter(p, room):
    import test_gpu_denoise as DN
    scene = FW.room(p) if room == "cutout" else FW.room(p, masks=False, fog=True)
    off = renderer(p, scene)
    off.refine(SPP)
    colour, frame = off.refine_sums(), off.DownloadRenderbuffer()
    off.close()
    r = renderer(p, scene)
    r.enable_aov(full=True)
    r.refine(SPP)
    sums, aov = r.refine_sums(), r.aov_sums()
    assert bits_equal(sums, colour) and bits_equal(r.DownloadRenderbuffer(), frame)
    want_aov = twin(p) if room == "cutout" else twin(p, masks=False, fog=True)
    assert bits_equal(aov, want_aov), mismatch_report(aov, want_aov)
    dp = p.Renderer.denoise_params()
    for params, demodulate in (({}, dp.demodulate), ({"demodulate": 0}, 0)):
        got = r.denoise(**params)
        want = DN.twin_denoise(sums, aov, SPP, SPP, dp.iterations, dp.sigma_depth, dp.sigma_lum, demodulate)
        assert bits_equal(got, want), mismatch_report(got, want)
        assert not bits_equal(got, frame)
    r.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(p):
    cam = p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, 1.0)
    spheres = p.Scene.book1_final(SEED)   # (the flat world borrows the scene's arrays: the scene stays alive)
    base = p.Renderer.MakeRenderer(32, 32, 4, 8, cam, spheres.getWorldPtr(), variant=1)
    with pytest.raises(p.capi.RtError, match="rt_renderer_aov_enable_mode.*variant 1"):
        base.enable_aov(full=True)
    base.close()
    L = p.capi.lib()
    # a cutout room: modes 0 and 1 refuse it in the words they had, on a new renderer; an unknown mode is still unknown
    scene = FW.room(p)
    r = renderer(p, scene)
    for who, enable in (("rt_renderer_aov_enable", lambda: r.enable_aov()), ("rt_renderer_aov_enable_mode", lambda: r.enable_aov(textured=True))):
        with pytest.raises(p.capi.RtError, match=who + ": the renderer has a cutout table, and the feature pass does not know the cutout rule") as e:
            enable()
        assert e.value.code == 1 and r.aov_info()["enabled"] is False
    assert L.rt_renderer_aov_enable_mode(r.h, 0, 3) == 1 and "unknown mode 3" in L.rt_last_error().decode()
    assert L.rt_renderer_aov_enable_mode(r.h, 0, 7) == 1 and "unknown mode 7" in L.rt_last_error().decode() and r.aov_mode() == "plain"
    # a record that names an image the table has lost: refused at the launch, before any kernel, the feature pass included
    r.enable_aov(full=True)
    records, texels = scene.textures()
    r.textures((records[:2].copy(), texels[:int(records[2]["first"])].copy()))
    with pytest.raises(p.capi.RtError, match="a cutout record of the world names image 2.*rt_renderer_textures"):
        r.refine(2)
    assert r.aov_info()["samples"] == 0 and r.refine_info()["samples"] == 0
    r.textures((records, texels))
    r.refine(2)
    assert r.aov_info()["samples"] == 2 and r.aov_mode() == "full"
    r.close()
    # rt_renderer_cutouts still refuses while mode 0 or 1 buffers are on
    bare = FW.room(p, masks=False)
    table = scene.cutouts()
    for kw in ({}, {"textured": True}):
        r = renderer(p, bare)
        r.enable_aov(**kw)
        with pytest.raises(p.capi.RtError, match="rt_renderer_cutouts: feature buffers are on, and the feature pass does not know the cutout rule"):
            r.cutouts(table)
        assert not r.cutouts_info()["enabled"]
        r.close()
    # a fog room: mode 0 names the medium, mode 1 refuses it in its own words
    r = renderer(p, FW.room(p, masks=False, fog=True))
    with pytest.raises(p.capi.RtError, match="rt_renderer_aov_enable: the world has a constant medium .RT_MAT_ISOTROPIC.: the feature pass covers"):
        r.enable_aov()
    with pytest.raises(p.capi.RtError, match="rt_renderer_aov_enable_mode: the world has a constant medium .RT_MAT_ISOTROPIC.: the textured feature pass covers"):
        r.enable_aov(textured=True)
    assert r.aov_info()["enabled"] is False
    r.enable_aov(full=True)
    r.close()
