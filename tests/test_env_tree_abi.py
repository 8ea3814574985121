"""The C and C++ callers of light-sampling mode 48 without a GPU: tests/cpp_env_tree/ builds against include/rt06.h and rt06.hpp, and the C11
translation unit's checks pass.  tests/test_gpu_env_tree.py runs the C++ program."""
import os
import subprocess

from _common import ROOT


def test_c_and_cpp_checks():
    d = os.path.join(ROOT, "tests", "cpp_env_tree")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ray-tracing-v06_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", d])
    assert subprocess.check_output([os.path.join(d, "env_tree_abi_check")], text=True).strip() == "env tree ABI ok"
    assert os.access(os.path.join(d, "env_tree_app"), os.X_OK)   # the program written against rt06.hpp compiles and links
