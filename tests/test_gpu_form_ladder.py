"""The ladder of the four per-material tables on the GPU: which kernel form a renderer holds under every subset of the tables, plain and under
mode 48, however the subset was reached; a table that changes only in what no kernel reads keeps the refinement; two ranks answer the _info queries as one
renderer does.  Nothing is rendered but the four 16 x 16 refine steps of the second test."""
import itertools

import numpy as np
import pytest

import _cutout_worlds as CW
import _nmap_worlds as NW
from _common import pkg

pytestmark = pytest.mark.gpu
TABLES = ("normal_maps", "microfacets", "interiors", "cutouts")   # the rungs, lowest first
SUBSETS = [frozenset(s) for k in range(5) for s in itertools.combinations(TABLES, k)]


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def dtypes(p):
    c = p.capi
    return dict(normal_maps=c.NORMAL_MAP_DT, microfacets=c.MICROFACET_DT, interiors=c.INTERIOR_DT, cutouts=c.CUTOUT_DT)


def queries(r):
    return (r.kernel_normal_map(), r.kernel_microfacet(), r.kernel_interior(), r.kernel_cutout())


def expected(on):
    """the form of the highest rung that is on; its key carries the bits of the rungs it reads, and RT_KEY_NMAP only on the lowest"""
    if "cutouts" in on:
        return (False, True, True, True)
    if "interiors" in on:
        return (False, True, True, False)
    if "microfacets" in on:
        return (False, True, False, False)
    return ("normal_maps" in on, False, False, False)


@pytest.mark.parametrize("mode", ["plain", "mode 48 first", "mode 48 last"])
def test_every_subset_of_the_tables_runs_the_form_of_its_highest_rung(p, mode):
    """the cutout room as an EXT 2 list world under the sky map, on the default variant with its texture table and no record: all 16 subsets of the four tables,
    each table with every record off, reached by switching tables on from none and by switching tables off from all four; mode 48 comes on before the tables
    or after them"""
    n_mats = len(CW.room(p, env=True, as_list=True).cutouts())
    scene = CW.room(p, env=True, as_list=True, records=False)
    r = p.Renderer.MakeRenderer(CW.W, CW.H, CW.SPP, CW.DEPTH, CW.camera(p), scene.getWorldPtr(), seed=CW.SEED)
    assert r.textures_info()["enabled"] and queries(r) == (False,) * 4 and r.kernel_form()["ext"] == 2
    off = {name: np.zeros(n_mats, dt) for name, dt in dtypes(p).items()}
    held = set()

    def check():
        if mode == "mode 48 last":
            r.light_sampling(48)
        assert queries(r) == expected(held), (sorted(held), queries(r))
        form = r.kernel_form()   # (refuses when the key does not name the kernel the renderer holds)
        assert form["kernel"] == "stream" and form["ext"] == 2 and form["nee"] == (mode != "plain")
        assert r.kernel_env_light() == r.kernel_light_tree() == (mode != "plain")
        if mode == "mode 48 last":
            r.light_sampling(0)

    if mode == "mode 48 first":
        r.light_sampling(48)
    for subset in SUBSETS:
        for start, step in ((set(), "on"), (set(TABLES), "off")):
            for name in TABLES:   # to the start: none, or all four
                if (name in start) != (name in held):
                    getattr(r, name)(off[name] if name in start else None)
            held = set(start)
            for name in (TABLES if step == "on" else reversed(TABLES)):
                if (name in subset) != (name in held):
                    getattr(r, name)(off[name] if name in subset else None)
                    held ^= {name}
                    check()   # every subset on the way is one of the sixteen too
            assert held == subset
            check()
            for name in TABLES:
                assert getattr(r, name + "_info")()["enabled"] == (name in subset)
    r.close()


def test_a_table_that_differs_in_what_no_kernel_reads_keeps_the_refinement(p):
    """the normal-map room at 16 x 16 and 2 samples: after refine(2), each of the four tables given again with other values in the fields no kernel reads — the
    fields of an off record, pad, reserved, the image of a constant record, a negative zero — leaves 2 samples done, and a further refine(2) gives 4"""
    scene = NW.room(p)
    r = p.Renderer.MakeRenderer(16, 16, 2, NW.DEPTH, NW.camera(p, 16, 16), scene.getWorldPtr(), seed=NW.SEED)
    nmaps = scene.normal_maps().copy()
    n, dt = len(nmaps), dtypes(p)
    assert r.normal_maps_info() == {"enabled": True, "mapped": 4} and 0 < (nmaps["on"] == 0).sum() < n
    mfac, intr, cut = np.zeros(n, dt["microfacets"]), np.zeros(n, dt["interiors"]), np.zeros(n, dt["cutouts"])
    mapped = int(np.nonzero(nmaps["on"])[0][0])           # a Lambertian with a map takes a constant microfacet record and a cutout too
    mfac[mapped] = (p.capi.MICROFACET_CONSTANT, 0, 0.3, 0.04)
    cut[mapped] = (p.capi.CUTOUT_MASKED, 1, 0.0, 0)
    r.microfacets(mfac), r.interiors(intr), r.cutouts(cut)
    done = r.refine(2)
    assert done == 2
    again = nmaps.copy()
    again["pad"] = 7
    again["image"][nmaps["on"] == 0], again["strength"][nmaps["on"] == 0] = 2, 2.5
    mfac2, intr2, cut2 = mfac.copy(), intr.copy(), cut.copy()
    mfac2["image"][mapped] = 2                              # a constant record reads no image
    others = np.arange(n) != mapped
    mfac2["image"][others], mfac2["roughness"][others], mfac2["specular"][others] = 1, 0.5, 0.5
    intr2["sigma"] = (0.25, -0.0, 3.0)                      # every record is off
    cut2["reserved"] = 9
    cut2["cutoff"][mapped] = -0.0
    cut2["image"][others], cut2["cutoff"][others] = 2, 0.75
    for name, table in (("normal_maps", again), ("microfacets", mfac2), ("interiors", intr2), ("cutouts", cut2)):
        getattr(r, name)(table)
        assert r.refine_info()["samples"] == done, name
        done = r.refine(2)
        assert done == r.refine_info()["samples"], name
    assert done == 2 + 4 * 2
    again["strength"][mapped] += 0.5                        # a field a kernel reads: the refinement starts anew
    r.normal_maps(again)
    assert r.refine_info()["samples"] == 0 and r.refine(2) == 2
    r.close()


def test_two_ranks_answer_the_info_queries_as_one_renderer_does(p, monkeypatch):
    monkeypatch.setenv("RT06_MULTI_TRANSPORT", "memcpy")
    scene = CW.room(p, live=True)
    one = p.Renderer.MakeRenderer(CW.W, CW.H, CW.SPP, CW.DEPTH, CW.camera(p), scene.getWorldPtr(), seed=CW.SEED)
    m = p.MultiRenderer.MakeRenderer(CW.W, CW.H, CW.SPP, CW.DEPTH, CW.camera(p), scene.getWorldPtr(), 2, seed=CW.SEED)
    assert m.cutouts_info() == one.cutouts_info() == {"enabled": True, "records": CW.RECORDS}
    assert m.microfacets_info() == one.microfacets_info() == {"enabled": True, "records": 2}
    assert m.textures_info() == one.textures_info() and m.textures_info()["enabled"]
    assert m.normal_maps_info() == one.normal_maps_info() == {"enabled": False, "mapped": 0}
    m.cutouts(None)
    assert m.cutouts_info() == {"enabled": False, "records": 0}
    m.close(), one.close()
