"""The launch images' layouts (csrc/rt_launch_image.hpp) without a GPU: tests/cpp_launch_image compares the light table of every mode and the
tail of the riders, word for word, with arrays written out by hand, built with -fsanitize=address,undefined."""
import os
import subprocess

from _common import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_launch_image")


def test_both_layouts_word_for_word_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", DIR])
    done = subprocess.run([os.path.join(DIR, "launch_image_check")], text=True, capture_output=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip().splitlines() == ["ok"]
