"""The whole-sample twins against tests/golden/frozen_twins.npz ("One loop for a whole sample") — no GPU.

The fixture was written by oracle/gen_frozen_twins.py from the ten radiance() loops that tests/_path_twin.py replaced; every case of it — each accepted mode or
argument shape of every twin module, on that module's own room — is recomputed here and compared for equality: the samples bit for bit (the NaNs of unfollowed
samples included), `followed`, and every counter the call filled.
"""
import functools
import os
import sys

import numpy as np
import pytest

from _common import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_frozen_twins as G  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "frozen_twins.npz"))
NAMES = sorted(k[: -len("/bits")] for k in GOLD.files if k.endswith("/bits"))


@functools.lru_cache(maxsize=None)
def cases():
    return G.cases(pkg())


def test_the_fixture_holds_every_case_of_the_generator():
    assert set(cases()) == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_a_twin_computes_what_the_fixture_recorded(name):
    got = G.compute_case(name, cases()[name])
    want = {k: GOLD[k] for k in GOLD.files if k in (name + "/bits", name + "/followed") or k.startswith(name + "/stats/")}
    assert set(got) == set(want)
    bits, gold = got[name + "/bits"], want[name + "/bits"]
    assert bits.shape == gold.shape
    differ = np.argwhere((bits != gold).any(axis=-1))
    assert len(differ) == 0, f"{len(differ)} samples differ; the first (y, x, sample): {differ[0].tolist()}: {bits[tuple(differ[0])]} for {gold[tuple(differ[0])]}"
    for key in sorted(want):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), f"{key}: {got[key]} for {want[key]}"
