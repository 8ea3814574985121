"""The full feature mode from C and C++ (tests/cpp_aov_full): the C11 ABI check runs without a GPU; the C++ program written against
include/rt06/rt06.hpp accumulates the feature sums and filters the frame the C ABI path gives through Python, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from _common import ROOT, bits_equal, mismatch_report, pkg

DIR = os.path.join(ROOT, "tests", "cpp_aov_full")


def build_programs():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", DIR])


def test_c_abi_check():
    build_programs()
    out = subprocess.check_output([os.path.join(DIR, "aov_full_abi_check")], text=True)
    assert out.strip() == "full feature ABI ok"


@pytest.mark.gpu
def test_the_cpp_app_gives_pythons_feature_sums(tmp_path):
    build_programs()
    w, h, depth, n = 24, 16, 6, 4
    prefix = str(tmp_path / "cpp")
    res = subprocess.run([os.path.join(DIR, "aov_full_app"), str(w), str(h), str(depth), str(n), prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip().splitlines() == ["plain: refused (names the cutout table)", "textured: refused (names the cutout table)", "mode=full", f"samples={n}",
                                               "after the table: samples=0 mode=full"]
    p = pkg()
    s = p.Scene()
    floor, fence, ball = s.Lambertian((0.5, 0.5, 0.5)), s.Lambertian((0.7, 0.5, 0.3)), s.Metal((0.8, 0.8, 0.9), 0.1)
    fog = s.add_material(p.capi.MAT_ISOTROPIC, (0.8, 0.85, 0.9), 0.3)
    i, j = np.meshgrid(np.arange(8), np.arange(4))
    image = s.add_image(np.repeat((((i + j) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2))
    s.set_cutout(fence, image)
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), floor)
    s.MakeQuad((-3, 0, 2), (6, 0, 0), (0, 3, 0), fence)
    s.MakeSphere((0.0, 1.0, 0.0), 1.0, ball)
    s.MakeSphere((1.0, 1.5, 3.5), 1.4, fog)
    s.set_background((0.6, 0.7, 0.9))
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(w, h, n, depth, p.PinholeCamera((0.5, 2.0, 7), (0, 1.0, 0), (0, 1, 0), 50.0, w / h), s.getWorldPtr(), seed=1984)
    assert r.kernel_cutout() and r.cutouts_info() == {"enabled": True, "records": 1}
    r.enable_aov(full=True)
    r.refine(n)
    den, holed = r.denoise(), r.aov_sums()
    load = lambda name, c: np.fromfile(prefix + name, dtype=np.float32).reshape(h, w, c)   # noqa: E731
    assert bits_equal(load("_aov.f32", 8), holed), mismatch_report(load("_aov.f32", 8), holed)
    assert bits_equal(load("_denoised.f32", 4), den)
    r.cutouts(None)
    r.refine(n)
    solid = r.aov_sums()
    r.close()
    assert bits_equal(load("_solid_aov.f32", 8), solid), mismatch_report(load("_solid_aov.f32", 8), solid)
    assert not bits_equal(holed, solid)
