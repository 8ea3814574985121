"""The texture-table surface from C and C++ (tests/cpp_textures): the C11 ABI check runs without a GPU; the C++ program written against
include/rt06/rt06.hpp renders the frame the C ABI path renders, bit for bit, and is refused once its table is off."""
import os
import subprocess

import numpy as np
import pytest

from _common import ROOT, pkg

DIR = os.path.join(ROOT, "tests", "cpp_textures")


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def build_programs():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", DIR])


def image(w, h, salt):
    """the image the program computes"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([40 + 200 * x // w, 30 + 180 * y // h, np.where((x + y + salt) & 1, 220, 60)], axis=2).astype(np.uint8)


def test_c_abi_check():
    build_programs()
    out = subprocess.check_output([os.path.join(DIR, "textures_abi_check")], text=True)
    assert out.strip() == "textures ABI ok"


@pytest.mark.gpu
def test_the_cpp_app_renders_the_frame_python_renders():
    build_programs()
    w, h, spp, depth = 24, 16, 8, 6
    out = subprocess.check_output([os.path.join(DIR, "textures_app"), str(w), str(h), str(spp), str(depth)], text=True, timeout=120)
    p = pkg()
    s = p.Scene()
    s.set_image(image(8, 4, 0))
    tiles = s.add_image(image(2, 2, 1), "repeat", "nearest")
    atlas = s.add_image(image(5, 3, 0))
    s.image_sampling(atlas, "clamp", "bilinear")
    m_globe, m_tiles, m_atlas = s.ImageTexture(), s.ImageTexture(tiles), s.ImageTexture(atlas)
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), m_tiles)
    s.MakeSphere((-1.2, 1.0, 0.0), 1.0, m_globe)
    s.MakeTriangle((0.5, 0.1, 0.5), (3.0, 0.1, 0.0), (1.5, 2.6, 0.2), m_atlas, uvs=[(-0.5, 0.0), (1.5, 0.25), (0.5, 1.5)])
    s.set_background((0.6, 0.7, 0.9))
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(w, h, spp, depth, p.PinholeCamera((0.5, 2.5, 7), (0, 1.0, 0), (0, 1, 0), 50.0, w / h), s.getWorldPtr(), seed=1984)
    assert r.kernel_form()["ext"] == 2 and r.textures_info() == {"enabled": True, "entries": 3}
    r.Render()
    frame = r.DownloadRenderbuffer()
    r.close()
    lines = out.strip().splitlines()
    assert lines[0] == f"textures {w}x{h} spp={spp} depth={depth} fnv={fnv1a(frame.tobytes()):016x}"
    assert lines[1] == "off: refused (names rt_renderer_textures)"
