"""The session surface without a GPU: a renderer that lives across frames (camera per Render(), progressive refinement).

Every new entry point is declared in include/rt06.h (plain C), exported by librt06.so and mirrored in capi.py / api.py / rt06.hpp;
tests/cpp_session/ holds a C11 -pedantic translation unit that takes the address of each one and a C++ caller written against rt06.hpp.
What the entry points compute is tests/test_gpu_session.py's subject."""
import ctypes as C
import os
import re
import subprocess

import pytest

from _common import ROOT, pkg

SESSION_DIR = os.path.join(ROOT, "tests", "cpp_session")
SESSION_SYMBOLS = ["rt_renderer_set_camera", "rt_multi_renderer_set_camera", "rt_renderer_refine", "rt_renderer_refine_async",
                   "rt_renderer_refine_reset", "rt_renderer_refine_info", "rt_renderer_refine_download_sums", "rt_renderer_refine_noise",
                   "rt_multi_renderer_refine"]


def build_session_apps():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", SESSION_DIR])


def test_every_session_symbol_is_declared_exported_and_bound():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in SESSION_SYMBOLS:
        assert name in declared, f"include/rt06.h does not declare {name}"
        assert name in p.capi.SYMBOLS
        assert hasattr(L, name), f"librt06.so does not export {name}"
        assert getattr(L, name).argtypes, f"capi.py gives {name} no signature"


def test_the_session_entry_points_compile_and_link_from_pedantic_c11():
    build_session_apps()
    src = open(os.path.join(SESSION_DIR, "session_abi_check.c")).read()
    for name in SESSION_SYMBOLS:
        assert re.search(r"=\s*" + name + r"\s*;", src), f"session_abi_check.c does not take the address of {name}"
    assert "-std=c11" in open(os.path.join(SESSION_DIR, "Makefile")).read() and "-pedantic" in open(os.path.join(SESSION_DIR, "Makefile")).read()
    out = subprocess.check_output([os.path.join(SESSION_DIR, "session_abi_check")], text=True)
    assert "session ABI ok" in out


def test_session_app_compiles_against_the_cpp_mirror():
    build_session_apps()
    r = subprocess.run([os.path.join(SESSION_DIR, "session_app")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: session_app camera" in r.stderr
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("void Refine(uint32_t n)", "void ResetRefinement()", "SamplesAccumulated()", "double Noise()", "const rt_camera* cam{}"):
        assert name in hpp, name


def test_python_mirror_has_the_session_methods():
    p = pkg()
    for name in ("set_camera", "refine", "refine_async", "refine_reset", "refine_info", "refine_sums", "noise"):
        assert callable(getattr(p.Renderer, name)), name
    for name in ("set_camera", "refine"):
        assert callable(getattr(p.MultiRenderer, name)), name


def test_null_handles_and_null_arguments_are_refused_before_any_device_is_touched():
    p = pkg()
    L = p.lib()
    cam = p.PinholeCamera((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, 1.5)
    out3, d = (C.c_uint64 * 3)(), C.c_double()
    calls = [lambda: L.rt_renderer_set_camera(None, C.byref(cam)), lambda: L.rt_multi_renderer_set_camera(None, C.byref(cam)),
             lambda: L.rt_renderer_refine(None, 1), lambda: L.rt_renderer_refine_async(None, None, None, 1), lambda: L.rt_renderer_refine_reset(None),
             lambda: L.rt_renderer_refine_info(None, out3), lambda: L.rt_renderer_refine_noise(None, C.byref(d)), lambda: L.rt_multi_renderer_refine(None, 1)]
    for call in calls:
        assert call() == 1   # RT_ERR_INVALID
        assert b"null" in L.rt_last_error()
    with pytest.raises(p.capi.RtError):
        p.Renderer(None, None).refine(1)
