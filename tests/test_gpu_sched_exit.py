"""The streaming kernel's node loop is left relative to the lane count it was entered with (inner_drop, inner_floor beside inner_keep).
That is scheduling only: which lane takes which step of which trace does not depend on it, so every frame must stay the CPU oracle's, bit for bit,
under any setting of the knobs — here at their extremes, on the hot loop (variant 3: Book-1, moving spheres) and on the generic loop of an EXT
instantiation (variant 2 on the Cornell box, a world with quads).

RT06_TUNE=keep,shade,leaf[,drop,floor] is read when a renderer is created; 0 for keep, shade, leaf or floor leaves the planned default.
"""
import numpy as np
import pytest

import _oracle as O
from _common import as_oracle_camera, as_oracle_world, bits_equal, config_cameras, config_scene, mismatch_report, pkg

pytestmark = pytest.mark.gpu

DEPTH = 8
SIZES = [(61, 37, 4), (240, 160, 8)]
WORLDS = {"book1_final": 0, "book2_moving": 0, "cornell_box": 2}   # scene -> variant (0 = the default, variant 3 on these BVH worlds)
# (keep, drop, floor); 0 = the shipped default.  The threshold of a loop entered with n lanes is min(keep, max(floor, n - drop)).
KNOBS = {
    "every_step": (64, 0, 64),   # threshold 64: the loop is left after a step unless all 64 lanes want another
    "never_early": (0, 64, 1),   # threshold 1: the loop runs until no lane is at an inner node
    "defaults": None,
    "odd_pair": (0, 7, 3),
}


def _tune(knob, leaf):
    if KNOBS[knob] is None:
        return f"0,0,{leaf}"
    keep, drop, floor = KNOBS[knob]
    return f"{keep},0,{leaf},{drop},{floor}"


@pytest.fixture(scope="module")
def p():
    m = pkg()
    assert m.api.device_count() >= 1, "no HIP device: the gpu tests need an MI355X"
    return m


_refs = {}


def _world(p, which, W, H):
    """The product's scene and camera, and the oracle's frame of them (computed once per world and size, shared, never written to)."""
    s = config_scene(p, which)
    cam = config_cameras(p, which, W, H)
    return s, cam


def _reference(which, w, cam, W, H, spp):
    key = (which, W, H, spp)
    if key not in _refs:
        ref, _ = O.render(as_oracle_world(w), as_oracle_camera(cam), W, H, spp, DEPTH)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


@pytest.mark.parametrize("leaf", [1, 64])
@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("W,H,spp", SIZES)
@pytest.mark.parametrize("which", list(WORLDS))
def test_frame_is_the_oracles_under_every_exit_rule(p, monkeypatch, which, W, H, spp, knob, leaf):
    s, cam = _world(p, which, W, H)
    w = s.getWorldPtr()
    ref = _reference(which, w, cam, W, H, spp)
    monkeypatch.setenv("RT06_TUNE", _tune(knob, leaf))
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w, variant=WORLDS[which])
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(img, ref), f"{which} {W}x{H}x{spp} {knob} leaf {leaf}: " + mismatch_report(img, ref)


def test_defaults_without_an_override_are_the_oracles(p, monkeypatch):
    """No RT06_TUNE at all: what a caller gets."""
    monkeypatch.delenv("RT06_TUNE", raising=False)
    W, H, spp = SIZES[0]
    for which, variant in WORLDS.items():
        s, cam = _world(p, which, W, H)
        w = s.getWorldPtr()
        r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w, variant=variant)
        r.Render()
        img = r.DownloadRenderbuffer()
        r.close()
        ref = _reference(which, w, cam, W, H, spp)
        assert bits_equal(img, ref), f"{which}: " + mismatch_report(img, ref)


@pytest.mark.parametrize("knob", ["every_step", "never_early", "odd_pair"])
def test_forced_pass_cut(p, monkeypatch, knob):
    """8 spp in passes of 3, 3 and 2: each pass drains its own queue, and the last lanes of each run under the dry-queue threshold."""
    W, H, spp = SIZES[1]
    s, cam = _world(p, "book1_final", W, H)
    w = s.getWorldPtr()
    ref = _reference("book1_final", w, cam, W, H, spp)
    monkeypatch.setenv("RT06_PASS_SPP", "3")
    monkeypatch.setenv("RT06_TUNE", _tune(knob, 4))
    r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w)
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(img, ref), f"{knob}: " + mismatch_report(img, ref)


@pytest.mark.parametrize("knob", ["every_step", "never_early", "odd_pair"])
def test_one_eighth_shards(p, monkeypatch, knob):
    """Each of 8 ranks traces every eighth tile: little work per wave, so most of a shard's life is the drain, where the threshold is 1 whatever
    the knobs say.  The assembled frame is the oracle's."""
    import torch
    W, H, spp = SIZES[1]
    s, cam = _world(p, "book1_final", W, H)
    w = s.getWorldPtr()
    ref = _reference("book1_final", w, cam, W, H, spp)
    monkeypatch.setenv("RT06_TUNE", _tune(knob, 4))
    stream = torch.cuda.current_stream().cuda_stream
    shards = []
    for rank in range(8):
        r = p.Renderer.MakeRenderer(W, H, spp, DEPTH, cam, w, rank=rank, world_size=8)
        buf = torch.zeros(r.shard_floats(), dtype=torch.float32, device="cuda:0")
        r.render_async(stream, buf.data_ptr())
        torch.cuda.synchronize()
        shards.append(buf)
        last = r
    image = torch.empty(H * W * 4, dtype=torch.float32, device="cuda:0")
    last.assemble(torch.cat(shards).data_ptr(), image.data_ptr(), stream)
    torch.cuda.synchronize()
    got = image.cpu().numpy().reshape(H, W, 4)
    assert bits_equal(got, ref), f"{knob}: " + mismatch_report(got, ref)
