"""The textured feature mode without a GPU: the ABI, the marble's host batch pinned to the CPU oracle, and the twin against itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _aov_tex_twin as AT
import _oracle as O
import _tex_twin as XT
import _tri_twin as TT
import _tri_worlds as TW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg

F = np.float32
W, H, SEED = 48, 32, 1984
NEW = ("rt_renderer_aov_enable_mode", "rt_renderer_aov_mode", "rt_noise_value_batch", "rt_probe_noise_value")


@pytest.fixture(scope="module")
def p():
    return pkg()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_prototyped_and_wrapped(p):
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    L = p.capi.lib()
    for name in NEW:
        assert name in p.capi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert re.search(r"^#define RT_AOV_PLAIN\s+0u", header, re.M) and re.search(r"^#define RT_AOV_TEXTURED\s+1u", header, re.M)
    assert (p.capi.AOV_PLAIN, p.capi.AOV_TEXTURED) == (0, 1)
    import inspect
    assert "textured" in inspect.signature(p.Renderer.enable_aov).parameters and inspect.signature(p.Renderer.enable_aov).parameters["textured"].default is False
    assert callable(p.Renderer.aov_mode) and callable(p.api.noise_value_batch) and callable(p.api.probe_noise_value)
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    assert re.search(r"enum class AovMode\s*\{\s*Plain,\s*Textured\s*\}", hpp) and "EnableAOV(uint32_t max_samples, AovMode mode)" in hpp


def test_every_null_argument_is_invalid(p):
    L = p.capi.lib()
    s = p.Scene().set_perlin(SEED)
    s.MakeSphere((0, 0, -3), 1.0, s.NoiseTexture(4.0))
    s.BuildBVH_TopDown()
    perlin = s.getWorldPtr().perlin
    albedo, pts, out, mode = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.1, 0.2, 0.3), (C.c_float * 3)(), C.c_uint32(9)
    assert L.rt_renderer_aov_enable_mode(None, 0, 0) == 1 and "rt_renderer_aov_enable_mode" in L.rt_last_error().decode()
    assert L.rt_renderer_aov_enable_mode(None, 0, 1) == 1
    assert L.rt_renderer_aov_mode(None, C.byref(mode)) == 1 and mode.value == 9
    good = [perlin, albedo, 4.0, pts, 1, out]
    assert L.rt_noise_value_batch(*good) == 0 and any(v != 0 for v in out)
    for k in (0, 1, 3, 5):
        args = list(good)
        args[k] = None
        assert L.rt_noise_value_batch(*args) == 1 and "rt_noise_value_batch: null" in L.rt_last_error().decode(), k
        assert L.rt_probe_noise_value(0, *args) == 1 and "rt_probe_noise_value: null" in L.rt_last_error().decode(), k   # refused before any device is touched
    assert p.api.noise_value_batch(s.getWorldPtr(), (0.5, 0.5, 0.5), 4.0, np.zeros((0, 3), F)).shape == (0, 3)
    with pytest.raises(ValueError):
        p.api.noise_value_batch(p.Scene.book1_final(SEED).getWorldPtr(), (0.5, 0.5, 0.5), 4.0, np.zeros((1, 3), F))


# ---- the marble's host batch is the oracle's marble ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perlin_seed", [1984, 7])
@pytest.mark.parametrize("scale", [4.0, 0.75])
def test_noise_batch_is_the_oracles_marble_bit_for_bit(p, scale, perlin_seed):
    """One marble sphere (centre (0.3, -0.2, -3.5), radius 1.25, albedo (0.5, 0.4, 0.3)) under a constant background (1, 1, 1), depth 2, 1 spp, pinhole, 48 x 32.
    A Lambertian scatter off a lone convex sphere escapes, so a hit pixel of the oracle is clamp01_sqrt(noise_value(hit point)) and has the bits of the batch's
    value at the twin's hit point.  A pixel is left out only when the oracle's is exactly 0 and the batch's is not (the scattered ray met the sphere again, or
    the scatter failed); at most 1 % of the hit pixels may be.  Observed on the four cases (scale, Perlin seed) = (4, 1984), (4, 7), (0.75, 1984), (0.75, 7):
    1 of 359 hit pixels left out in each (0.28 %)."""
    albedo = (0.5, 0.4, 0.3)
    s = p.Scene().set_perlin(perlin_seed)
    s.set_background((1, 1, 1))
    s.MakeSphere((0.3, -0.2, -3.5), 1.25, s.NoiseTexture(scale, albedo))
    s.BuildBVH_TopDown()
    wf = s.getWorldPtr()
    world, cam = as_oracle_world(wf), as_oracle_camera(p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, W / H))
    frame, _ = O.render(world, cam, W, H, 1, 2, SEED)
    rays = AT.primary_rays(cam, W, H, 1, SEED)
    hit, t, _, _ = TT.closest_intersection(world, rays)
    h = hit != 0
    assert 300 < h.sum() < W * H
    with np.errstate(all="ignore"):
        pos = (rays[h, 0:3] + rays[h, 3:6] * t[h][:, None]).astype(F)
    value = p.api.noise_value_batch(wf, albedo, scale, pos)
    samples = np.ones((W * H, 1, 3), F)   # a miss: the background
    samples[h, 0] = value * np.ones(3, F) + np.zeros(3, F)
    want = XT.resolve(XT.in_order_sums(samples.reshape(H, W, 1, 3)), 1)[..., 0:3].reshape(-1, 3)
    got = frame[..., 0:3].reshape(-1, 3)
    left_out = h & (got == 0).all(axis=1) & ~(want == 0).all(axis=1)
    print(f"scale {scale}, perlin seed {perlin_seed}: {int(left_out.sum())} of {int(h.sum())} hit pixels left out")
    assert left_out.sum() <= 0.01 * h.sum()
    keep = ~left_out
    assert bits_equal(got[keep], want[keep]), mismatch_report(got[keep], want[keep])
    assert len(np.unique(got[h & keep], axis=0)) > 100   # a marble, not a constant


# ---- the twin agrees with itself -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_without_textured_materials_both_modes_of_the_twin_are_one(p, as_list):
    scene = TW.tri_room(p, as_list=as_list)   # Lambertian, metal, checker and light: no noise, no image
    world, cam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(TW.camera(p, 24, 16))
    plain, rate = AT.sums(world, cam, 24, 16, 3, SEED, textured=False)
    tex, _ = AT.sums(world, cam, 24, 16, 3, SEED, textured=True)
    assert rate == 1.0 and bits_equal(plain, tex)
    assert len(np.unique(plain[..., 4:7].reshape(-1, 3), axis=0)) > 4   # several albedos, the checker's two among them
    five = TT.first_hit_sums(world, cam, 24, 16, 3, SEED)   # the older twin of the normal, depth and hit sums
    assert bits_equal(plain[..., 0:4], five[..., 0:4]) and bits_equal(plain[..., 7], five[..., 4])
    textured = TW.tri_room(p, as_list=as_list, textured=True)   # (the flat world borrows the scene's arrays: the scene stays alive)
    with pytest.raises(AssertionError, match="RT_AOV_PLAIN refuses"):
        AT.sums(as_oracle_world(textured.getWorldPtr()), as_oracle_camera(TW.camera(p, 48, 32)), 48, 32, 1, SEED, textured=False)
