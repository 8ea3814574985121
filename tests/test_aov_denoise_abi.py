"""The feature-buffer and denoiser surface without a GPU: declared in include/rt06.h (plain C), exported by librt06.so, mirrored in
capi.py / api.py / rt06.hpp; tests/cpp_denoise/ holds a C11 -pedantic translation unit that takes the address of each entry point and a
C++ caller written against rt06.hpp.  What the entry points compute is the subject of tests/test_gpu_aov.py and tests/test_gpu_denoise.py."""
import ctypes as C
import os
import re
import subprocess

from _common import ROOT, pkg

DENOISE_DIR = os.path.join(ROOT, "tests", "cpp_denoise")
SYMBOLS = ["rt_renderer_aov_enable", "rt_renderer_aov_info", "rt_renderer_aov_download", "rt_denoise_params_default", "rt_renderer_denoise",
           "rt_renderer_denoise_async", "rt_renderer_denoise_download"]


def build_apps():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", DENOISE_DIR])


def test_every_symbol_is_declared_exported_and_bound():
    p = pkg()
    L = p.lib()
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, f"include/rt06.h does not declare {name}"
        assert name in p.capi.SYMBOLS
        assert hasattr(L, name), f"librt06.so does not export {name}"
        assert getattr(L, name).argtypes, f"capi.py gives {name} no signature"
    section = header.index("Feature buffers and denoiser")
    assert header.index("Progressive refinement") < section < header.index("Multi-GPU renderer")
    assert "not in the reference" in header[section:section + 200]


def test_denoise_params_default_fills_the_documented_defaults():
    p = pkg()
    dp = p.capi.DenoiseParams(99, -1.0, -1.0, 99)
    assert p.lib().rt_denoise_params_default(C.byref(dp)) == 0
    assert dp.iterations == 5 and dp.demodulate == 1
    header = open(os.path.join(ROOT, "include", "rt06.h")).read()
    doc = {k: float(re.search(r"float " + k + r";\s*/\* default ([0-9.]+)", header).group(1)) for k in ("sigma_depth", "sigma_lum")}
    assert dp.sigma_depth == C.c_float(doc["sigma_depth"]).value and dp.sigma_lum == C.c_float(doc["sigma_lum"]).value
    assert p.Renderer.denoise_params(iterations=3, demodulate=0).iterations == 3


def test_null_arguments_are_refused_with_a_message_before_any_device_is_touched():
    p = pkg()
    L = p.lib()
    dp = p.Renderer.denoise_params()
    out3 = (C.c_uint64 * 3)()
    import numpy as np
    buf = np.zeros(8, np.float32)
    calls = [lambda: L.rt_renderer_aov_enable(None, 0), lambda: L.rt_renderer_aov_info(None, out3), lambda: L.rt_renderer_aov_download(None, buf, 8),
             lambda: L.rt_denoise_params_default(None), lambda: L.rt_renderer_denoise(None, C.byref(dp)), lambda: L.rt_renderer_denoise_async(None, None, C.byref(dp)),
             lambda: L.rt_renderer_denoise_download(None, buf[:4].copy(), 4)]
    for call in calls:
        assert call() == 1   # RT_ERR_INVALID
        assert b"null" in L.rt_last_error()


def test_the_entry_points_compile_and_link_from_pedantic_c11():
    build_apps()
    src = open(os.path.join(DENOISE_DIR, "denoise_abi_check.c")).read()
    for name in SYMBOLS:
        assert re.search(r"=\s*" + name + r"\s*;", src), f"denoise_abi_check.c does not take the address of {name}"
    mk = open(os.path.join(DENOISE_DIR, "Makefile")).read()
    assert "-std=c11" in mk and "-pedantic" in mk
    out = subprocess.check_output([os.path.join(DENOISE_DIR, "denoise_abi_check")], text=True)
    assert "denoise ABI ok" in out


def test_denoise_app_compiles_against_the_cpp_mirror_and_python_has_the_methods():
    build_apps()
    r = subprocess.run([os.path.join(DENOISE_DIR, "denoise_app")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: denoise_app" in r.stderr
    hpp = open(os.path.join(ROOT, "include", "rt06", "rt06.hpp")).read()
    for name in ("void EnableAOV(", "void DownloadAOV(", "void Denoise(", "void DownloadDenoised("):
        assert name in hpp, name
    p = pkg()
    for name in ("enable_aov", "aov", "aov_info", "aov_sums", "denoise", "denoise_async"):
        assert callable(getattr(p.Renderer, name)), name
