"""The 32 NMAP and MFAC instantiations of render_kernel_stream on the GPU against the CPU oracle, through inert tables, bit for bit on every pixel.

The oracle knows no normal map and no microfacet record, and the twins of §28 to §30 follow no medium, no noise material, no moving sphere and only the pinhole
camera.  An inert table (tests/_surface_worlds.py: flat maps and bending maps at strength 0 on every material that takes one; records that are all off on the
materials in use, live ones on materials nothing uses) runs the new kernels on worlds whose frame the oracle gives: _tri_worlds' wide room with its medium, noise
triangle, image triangle, glass icosphere, moving sphere and fuzzy tetrahedron under three cameras, the worlds around the group boundary, twelve random worlds;
mode 48's forms take _env_tree_worlds' room and its twin's sums.  Every test names the kernel it ran through kernel_form(), kernel_normal_map() and
kernel_microfacet(): a microfacet table makes the MFAC family answer, which reads the normal-map table too, so MFAC runs with both tables on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _env_tree_twin as VT
import _env_tree_worlds as VW
import _oracle as O
import _surface_worlds as SW
import _tri_worlds as TW
from _common import ROOT, as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg
from test_gpu_triangles_oracle import BOUNDARY, WALKS, boundary_expected, check_frame, wide_room_expected

pytestmark = pytest.mark.gpu
FORMS = list(SW.FORMS)
FORM_IDS = [TW.form_id(f) for f in FORMS]
FAMILIES = ("NMAP", "MFAC")


@pytest.fixture(scope="module")
def p():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return pkg()


def setenv(monkeypatch, env, **more):
    for k in ("RT06_FORCE_BIG", "RT06_FORCE_WIDE", "RT06_PASS_SPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in {**env, **more}.items():
        monkeypatch.setenv(k, v)


def states_its_family(r, family, counts, why=""):
    """the renderer runs the family's kernel and holds the inert tables as they were built"""
    assert r.kernel_normal_map() == (family == "NMAP") and r.kernel_microfacet() == (family == "MFAC") and r.kernel_triangles(), (why, r.kernel_form())
    assert r.normal_maps_info() == {"enabled": True, "mapped": counts["mapped"]}, why
    assert r.microfacets_info() == {"enabled": family == "MFAC", "records": counts["records"]}, why
    assert r.textures_info()["enabled"]


# ---- a: the wide room, every plain form of both families, three cameras ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_kind", TW.CAMERAS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_plain_form_renders_the_wide_room_under_inert_tables_as_the_oracle_does(p, monkeypatch, form, family, cam_kind):
    """The eight plain RT_KERNEL_NORMAL_MAP keys and the eight plain RT_KERNEL_MICROFACET keys on the EXT 2 room: a sphere of medium, a Perlin-noise and an
    image-textured triangle, a glass icosphere, a moving sphere, a fuzzy-metal tetrahedron, a background behind an opening, under the pinhole, the defocus and
    the motion-blur camera.  Frame and refinement sums, every pixel, two passes and uneven refine steps."""
    as_list = form[0] == TW.LIST
    variant, env = SW.FORMS[form]
    exp = wide_room_expected(2, as_list, cam_kind)
    setenv(monkeypatch, env, RT06_PASS_SPP="3")
    scene = TW.wide_room(p, ext=2, as_list=as_list)
    counts = SW.inert_tables(scene, microfacets=family == "MFAC")
    assert counts["mapped"] >= 8 and counts["records"] == (SW.LIVE_RECORDS if family == "MFAC" else 0)
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, scene.getWorldPtr(), seed=TW.SEED, variant=variant)
    assert r.kernel_form() == TW.kernel_form_of(form), r.kernel_form()
    states_its_family(r, family, counts)
    r.Render()
    img = r.DownloadRenderbuffer()
    check_frame(img, exp.frame)
    r.refine(1)
    r.refine(3)
    check_frame(r.refine_sums(), exp.sums)
    assert bits_equal(r.DownloadRenderbuffer(), img)
    r.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_the_inert_records_are_in_view(p, monkeypatch, family):
    """the proof that the comparison above judges something: with the first flat map replaced by a bending one (NMAP), or with a record switched on on the
    materials in use (MFAC), the same room on the same kernel is no longer the oracle's frame"""
    setenv(monkeypatch, TW.LDS)
    exp = wide_room_expected(2, False, "pinhole")
    scene = TW.wide_room(p, ext=2)
    counts = SW.inert_tables(scene, microfacets=family == "MFAC", bend=family == "NMAP", live=family == "MFAC")
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, scene.getWorldPtr(), seed=TW.SEED)
    states_its_family(r, family, counts)
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    differ = (img.view(np.uint32) != exp.frame.view(np.uint32)).any(axis=2)
    print(f"{family}: {int(differ.sum())} of {differ.size} pixels differ once the records act")
    assert differ.any()


# ---- b: random triangle worlds -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed", list(range(12)))
def test_random_triangle_worlds_render_bit_exact_under_inert_tables(p, monkeypatch, seed, family):
    """_tri_worlds.random_tri_world's twelve worlds — moving spheres, media, noise and image textures, glass, every builder, three cameras — on the form the
    renderer picks; the EXT 1 worlds among them (seeds 3, 4, 5, 9, 10, 11) are moved to the EXT 2 kernel by the table.  A world in which no material in use takes
    a record would be skipped: every one of the twelve has three or five such materials, so 0 of 12 skip (tests/_surface_worlds.takes_a_record, counted without a
    GPU).  Frames wider than 32 pixels are rendered 32 wide, by the oracle too."""
    setenv(monkeypatch, TW.LDS)
    scene, cam, W, H, spp, depth, recipe = TW.random_tri_world(p, seed)
    if not SW.takes_a_record(scene):
        pytest.skip("no material in use takes a normal map or a microfacet record")
    W, H = min(W, 32), min(H, 32)
    ref, _ = O.render(as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam), W, H, spp, depth, TW.SEED)   # before the tables: they add materials
    counts = SW.inert_tables(scene, microfacets=family == "MFAC")
    w = scene.getWorldPtr()
    r = p.Renderer.MakeRenderer(W, H, spp, depth, cam, w, seed=TW.SEED)
    form = r.kernel_form()
    recipe.update(kernel=form, family=family, tables=counts)
    assert form["kernel"] == "stream" and form["ext"] == 2 and form["world"] == w.kind, recipe
    states_its_family(r, family, counts, recipe)
    r.Render()
    img = r.DownloadRenderbuffer()
    r.close()
    assert np.array_equal(np.isnan(img), np.isnan(ref)), recipe
    assert bits_equal(img, ref), f"{recipe}: " + mismatch_report(img, ref)


# ---- c: the group boundary -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("walk", ["stack-exact", "stack-fast", "list"])
@pytest.mark.parametrize("which", BOUNDARY)
def test_worlds_around_the_group_boundary_render_as_the_oracle_does_under_inert_tables(p, monkeypatch, which, walk, family):
    """no parallelogram at all (and no sphere), exactly one, one triangle behind many, the last parallelogram and the first triangle under one inner node: EXT 1
    worlds without an image, which the tables move to the families' EXT 2 forms, where the planar (u, v) of a quad and of a triangle are computed for the flat map"""
    setenv(monkeypatch, TW.LDS)
    as_list, variant, traversal = WALKS[walk]
    assert traversal == 0
    exp = boundary_expected(which, as_list, 0)
    builder = "MakeHittableList" if as_list else ("BuildBVH_SAH" if which == "siblings" else "BuildBVH_TopDown")
    scene = TW.boundary_world(p, which, builder, 0)
    counts = SW.inert_tables(scene, microfacets=family == "MFAC")
    r = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, scene.getWorldPtr(), seed=TW.SEED, variant=variant)
    assert r.kernel_form() == TW.kernel_form_of((TW.LIST if as_list else TW.BVH, int(variant != 3), 2, 0, 0)), r.kernel_form()
    states_its_family(r, family, counts)
    r.Render()
    check_frame(r.DownloadRenderbuffer(), exp.frame)
    r.refine(TW.SPP)
    check_frame(r.refine_sums(), exp.sums)
    r.close()


# ---- d: mode 48 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_mode_48_form_renders_the_sky_room_under_inert_tables_as_the_twin_does(p, monkeypatch, form, family):
    """The eight RT_KERNEL_NORMAL_MAP_ENV_TREE keys and the eight RT_KERNEL_MICROFACET_ENV_TREE keys.  The oracle does not know mode 48, and the mode refuses
    media: the judge is §26's whole-sample twin on §26's room (tests/test_gpu_env_tree.py's `forms` world and sums, computed without any table), never another
    kernel's output."""
    as_list = form[0] == TW.LIST
    run = VW.run("forms", as_list=as_list)
    assert run.followed.all()
    setenv(monkeypatch, SW.FORMS[form][1])
    scene = VW.sky_lamp_room(p, as_list=as_list)
    counts = SW.inert_tables(scene, microfacets=family == "MFAC")
    r = p.Renderer.MakeRenderer(VW.W, VW.H, VW.SPP, VW.DEPTH, VW.camera(p, run.view), scene.getWorldPtr(), seed=VW.SEED, variant=SW.FORMS[form][0])
    r.light_sampling(VW.ENV_TREE)
    assert r.kernel_form() == TW.kernel_form_of(form, nee=1), r.kernel_form()
    assert r.kernel_env_light() and r.kernel_light_tree() and r.light_sampling_info() == {"enabled": True, "lights": run.tree.n_l}
    states_its_family(r, family, counts)
    r.refine(VW.SPP)
    sums, frame = r.refine_sums(), r.DownloadRenderbuffer()
    r.close()
    assert bits_equal(sums, run.sums), mismatch_report(sums, run.sums)
    assert bits_equal(frame, VT.resolve(sums, VW.SPP))


# ---- e: two ranks ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_render_the_wide_room_under_both_inert_tables_through_the_memcpy_transport(p, monkeypatch):
    setenv(monkeypatch, TW.LDS, RT06_MULTI_TRANSPORT="memcpy")
    exp = wide_room_expected(2, False, "motion")
    scene = TW.wide_room(p, ext=2)
    counts = SW.inert_tables(scene)
    one = p.Renderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, scene.getWorldPtr(), seed=TW.SEED)
    assert one.kernel_form() == TW.kernel_form_of((TW.BVH, 0, 2, 0, 0))   # what every rank runs on its share
    states_its_family(one, "MFAC", counts)
    one.close()
    m = p.MultiRenderer.MakeRenderer(TW.W, TW.H, TW.SPP, TW.DEPTH, exp.cam, scene.getWorldPtr(), 2, seed=TW.SEED)
    assert m.normal_maps_info() == {"enabled": True, "mapped": counts["mapped"]} and m.microfacets_info() == {"enabled": True, "records": counts["records"]}
    m.Render()
    check_frame(m.DownloadRenderbuffer(), exp.frame)
    m.close()


# ---- the fuzzer ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_fuzz_campaign_runs_twenty_worlds_under_inert_surface_tables(p):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_campaign.py"), "--seeds", "20", "--surfaces"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    done = [line for line in res.stdout.splitlines() if line.startswith("DONE: 20 worlds, 0 failures")]
    assert done and "'surface_worlds':" in done[0] and "'surface_kernels':" in done[0], res.stdout[-2000:]
    print(done[0])
