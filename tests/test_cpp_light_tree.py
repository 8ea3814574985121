"""The light-tree surface from C and from C++: tests/cpp_light_tree/ holds a C11 -pedantic translation unit that checks the new declarations of
include/rt06.h on the host, and a program written against include/rt06/rt06.hpp that renders a room lit by two triangles with LightSampling::Tree."""
import os
import re
import subprocess

import pytest

from _common import ROOT, pkg
from test_cpp_api import fnv1a

DIR = os.path.join(ROOT, "tests", "cpp_light_tree")


def build_callers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])   # as the other ABI tests do: built where it is missing
    subprocess.check_call(["make", "-s", "-C", DIR])


def test_the_new_declarations_compile_as_c11_and_the_host_table_is_what_the_header_says():
    build_callers()
    mk = open(os.path.join(DIR, "Makefile")).read()
    assert "-std=c11" in mk and "-pedantic" in mk
    src = open(os.path.join(DIR, "light_tree_abi_check.c")).read()
    for name in ("rt_world_light_tree", "rt_renderer_kernel_light_tree", "RT_LIGHT_SAMPLING_TREE", "RT_MAX_LIGHTS_TREE", "RT_LIGHT_TREE_K"):
        assert name in src
    assert subprocess.check_output([os.path.join(DIR, "light_tree_abi_check")], text=True).strip() == "light tree ABI ok"
    r = subprocess.run([os.path.join(DIR, "light_tree_app")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: light_tree_app" in r.stderr


def room(p):
    """tests/cpp_light_tree/light_tree_app.cpp's room, call for call"""
    s = p.Scene()
    white, red, lamp = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.DiffuseLight((14, 12, 9))
    s.MakeQuad((0, 0, 0), (10, 0, 0), (0, 0, 10), white)
    s.MakeQuad((0, 10, 0), (10, 0, 0), (0, 0, 10), white)
    s.MakeQuad((0, 0, 0), (0, 10, 0), (0, 0, 10), red)
    s.MakeQuad((0, 0, 10), (10, 0, 0), (0, 10, 0), white)
    s.MakeTriangle((3.5, 9.5, 4), (6.5, 9.7, 4.5), (5, 9.2, 7), lamp)
    s.MakeTriangle((0.3, 5, 3), (0.3, 7, 4), (0.4, 5.5, 6), lamp)
    s.MakeTriangle((2, 0, 5), (5, 0, 4), (3.5, 3, 6), red)
    s.set_background((0, 0, 0))
    s.BuildBVH_TopDown()
    return s


@pytest.mark.gpu
def test_the_cpp_mirror_renders_with_the_light_tree_what_the_c_abi_renders():
    build_callers()
    W, H, spp, depth = 32, 32, 4, 8
    out = subprocess.check_output([os.path.join(DIR, "light_tree_app"), str(W), str(H), str(spp), str(depth)], text=True, timeout=120)
    m = re.search(r"fnv=([0-9a-f]+)", out)
    assert m, out
    p = pkg()
    s = room(p)
    r = p.Renderer.MakeRenderer(W, H, spp, depth, p.PinholeCamera((5, 5, 0.5), (5, 4, 10), (0, 1, 0), 80.0, W / H), s.getWorldPtr())
    r.Render()
    plain = r.DownloadRenderbuffer()
    r.light_sampling("mesh")
    r.Render()
    by_count = r.DownloadRenderbuffer()
    r.light_sampling("tree")
    assert r.light_sampling_info() == {"enabled": True, "lights": 2} and r.light_sampling_mode() == 16 and r.kernel_light_tree()
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    assert int(m[1], 16) == fnv1a([img.tobytes()]) and int(m[1], 16) not in (fnv1a([plain.tobytes()]), fnv1a([by_count.tobytes()]))
