"""Solid glass from C and C++ (tests/cpp_interiors): the tail's layout check and the C11 ABI check run without a GPU; the C++ program written
against include/rt06/rt06.hpp renders the frames the C ABI path renders, solid and thin, bit for bit."""
import os
import subprocess

import pytest

from _common import ROOT, pkg

DIR = os.path.join(ROOT, "tests", "cpp_interiors")


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def build_programs():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", DIR])


def test_the_tail_with_and_without_the_table():
    """a host program with its own main, under the address and undefined-behaviour sanitizers: the sub-header and both tables word for word"""
    build_programs()
    out = subprocess.check_output([os.path.join(DIR, "interiors_tail_check")], text=True)
    assert out.strip() == "ok"


def test_c_abi_check():
    build_programs()
    out = subprocess.check_output([os.path.join(DIR, "interiors_abi_check")], text=True)
    assert out.strip() == "interiors ABI ok"


@pytest.mark.gpu
def test_the_cpp_app_renders_the_frames_python_renders():
    build_programs()
    w, h, spp, depth = 24, 16, 8, 8
    out = subprocess.check_output([os.path.join(DIR, "interiors_app"), str(w), str(h), str(spp), str(depth)], text=True, timeout=120)
    p = pkg()
    s = p.Scene()
    floor, box, ball = s.Lambertian((0.5, 0.5, 0.5)), s.Dielectric((1, 1, 1), 1.5), s.Dielectric((1, 1, 1), 1.33)
    s.set_interior(box, sigma=(1.0, 0.25, 0.5)).set_interior(ball, sigma=(0.125, 0.5, 1.0))
    s.MakeQuad((-6, 0, -6), (12, 0, 0), (0, 0, 12), floor)
    s.MakeBox((0.2, 0.1, -0.8), (2.0, 1.9, 1.0), box, rotate_y=20.0)
    s.MakeSphere((-1.4, 1.0, 0.2), 1.0, ball)
    s.set_background((0.6, 0.7, 0.9))
    s.BuildBVH_TopDown()
    r = p.Renderer.MakeRenderer(w, h, spp, depth, p.PinholeCamera((0.5, 2.5, 7), (0, 1.0, 0), (0, 1, 0), 50.0, w / h), s.getWorldPtr(), seed=1984)
    assert r.kernel_interior() and r.interiors_info() == {"enabled": True, "records": 2} and not r.microfacets_info()["enabled"]
    r.Render()
    on = r.DownloadRenderbuffer()
    r.interiors(None)
    assert not r.kernel_interior() and not r.kernel_microfacet()
    r.Render()
    off = r.DownloadRenderbuffer()
    r.close()
    lines = out.strip().splitlines()
    assert lines[0] == f"interiors {w}x{h} spp={spp} depth={depth} fnv={fnv1a(on.tobytes()):016x}"
    assert lines[1] == f"off: fnv={fnv1a(off.tobytes()):016x}" and lines[0].split("fnv=")[1] != lines[1].split("fnv=")[1]
