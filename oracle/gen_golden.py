#!/usr/bin/env python3
"""Generate tests/golden/glm_*.f32 from the reference's vendored GLM, tests/golden/ref_* from the reference's own
aabb / HittableList / bvh_node / checker_texture headers, and tests/golden/ref_core_* from its spheres, flat BVH and builders,
materials and cameras (dev container only).

Builds oracle/_ref/glm_probe (oracle/Makefile `ref`: g++ on ref_glm_probe.cpp with
-I/root/reference/Libraries/include -I/root/reference/main/src — the reference sources are
compiled where they lie, never copied) and runs it.  The fixtures are data (inputs + expected
outputs); commit them together with this script.
"""
import ctypes as C
import os, subprocess, sys

import numpy as np
here = os.path.dirname(os.path.abspath(__file__))
out = os.path.join(here, "..", "tests", "golden")
os.makedirs(out, exist_ok=True)
subprocess.check_call(["make", "-C", here, "ref"])
subprocess.check_call([os.path.join(here, "_ref", "glm_probe"), out])
# the reference's headers above the vocabulary (oracle/ref_path_probe.cpp; <cuda_runtime.h> = NVIDIA's own, from the triton wheel)
subprocess.check_call([os.path.join(here, "_ref", "path_probe"), out])

# the reference's spheres, BVH, Scatter and cameras (oracle/ref_core_probe.cpp), served uniforms from tapes.  The natural tapes are
# the product's own uniforms for (seed 1984, pixel, sample), from the oracle's orc_rng_uniforms: rows [pixel, sample, k_0..k_95]
# with u = k * 2^-24.  The probe runs under a time limit (BVH.cu's rec2 recursion is guarded in the probe; this bounds the rest).
subprocess.check_call(["make", "-C", here, "liboracle.so"])
orc = C.CDLL(os.path.join(here, "liboracle.so"))
orc.orc_rng_uniforms.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
NATURAL_LEN, N_TAPES = 96, 8192
rows = np.zeros((N_TAPES, 2 + NATURAL_LEN), np.uint32)
u = np.zeros(NATURAL_LEN, np.float32)
for i in range(N_TAPES):
    pixel, sample = (i * 7919) % 1048576, i % 16
    orc.orc_rng_uniforms(1984, pixel, sample, 0, NATURAL_LEN, u.ctypes.data_as(C.POINTER(C.c_float)))
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.all(k == np.round(k)) and k.min() >= 1 and k.max() <= 2 ** 24
    rows[i, 0], rows[i, 1], rows[i, 2:] = pixel, sample, k.astype(np.uint32)
tapes = os.path.join(here, "_ref", "natural_tapes.u32")
rows.tofile(tapes)
subprocess.check_call(["timeout", "-k", "10", "600", os.path.join(here, "_ref", "core_probe"), out, tapes])
