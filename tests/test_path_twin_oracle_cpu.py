"""The extended whole-sample twin against the CPU oracle, without a GPU.

Without tables the numpy loop of tests/_path_twin.py and the oracle's sample_world state the same path: cameras that draw a lens point or a time, moving spheres,
constant media that draw inside the walk, isotropic and noise hits, glass.  Every comparison is bit for bit with NaN equal to NaN, and the twin follows every
sample.  The twin is judged here by an independent C restatement before it judges a kernel (tests/test_gpu_live_surfaces.py).
"""
import ctypes as C

import numpy as np
import pytest

import _aov_tex_twin as AT
import _noise_twin as NZ
import _oracle as O
import _path_twin as PT
import _tex_twin as XT
import _tri_twin as TT
import _tri_worlds as TW
from _common import as_oracle_camera, as_oracle_world, bits_equal, mismatch_report, pkg, random_mixed_scene

F = np.float32
COUNTERS = ("medium_draws", "medium_hits", "medium_scatters", "noise_hits", "moving_hits")


@pytest.fixture(scope="module")
def p():
    return pkg()


def oracle_samples(world, cam, w, h, spp, depth, seed):
    gids, smp = PT.keys(w, h, spp)
    keys = np.ascontiguousarray(np.stack([gids, smp], axis=1), np.uint32)
    out = np.zeros((len(keys), 3), F)
    assert O.lib().orc_radiance_batch(C.byref(world), C.byref(cam), w, h, depth, seed, len(keys), keys, out) == 0
    return out


def twin_samples(scene, world, cam, w, h, spp, depth, seed, stats, trace=TT.closest_intersection):
    image = AT.world_image(scene.getWorldPtr())
    tex = (None, [(image, XT.CLAMP, XT.NEAREST)]) if image is not None else None   # the world's one image, as image_texel reads it
    return PT.radiance(world, cam, w, h, depth, seed, *PT.keys(w, h, spp), trace, glass=True, media=True, tex=tex, stats=stats)


def compare(scene, cam, w, h, spp, depth, seed, stats, trace=TT.closest_intersection):
    world, ocam = as_oracle_world(scene.getWorldPtr()), as_oracle_camera(cam)
    got, followed = twin_samples(scene, world, ocam, w, h, spp, depth, seed, stats, trace)
    exp = oracle_samples(world, ocam, w, h, spp, depth, seed)
    assert followed.all(), f"{int((~followed).sum())} samples not followed"
    assert bits_equal(got, exp), mismatch_report(got, exp)


def test_the_noise_twin_is_rt_noise_value_batch_bit_for_bit(p):
    s = p.Scene()
    s.set_perlin(TW.SEED)
    s.MakeSphere((0, 0, 0), 1.0, s.NoiseTexture(2.0, (0.6, 0.6, 0.6)))
    s.BuildBVH_SAH()
    world = as_oracle_world(s.getWorldPtr())
    rng = np.random.default_rng(33)
    lattice = np.stack(np.meshgrid(*[np.arange(-3, 4, dtype=F)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    points = np.concatenate([
        (rng.random((4096, 3), dtype=F) * 40 - 20).astype(F),             # random, both signs
        lattice, lattice + F(0.5), lattice * F(256),                       # on the lattice, between it, at the permutation's period
        -(rng.random((512, 3), dtype=F) * 300).astype(F),                  # negative throughout: floor and & 255 below zero
        np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [255, 255, 255], [256, -256, 1e-30], [-1e-30, 1e-30, -1], [1000.25, -1000.75, 3.5]], F)])
    tab = NZ.tables(world)
    for albedo, scale in (((0.6, 0.6, 0.6), 2.0), ((1.0, 0.25, 0.0), 0.5), ((0.3, 0.9, 0.7), 7.0)):
        exp = p.api.noise_value_batch(s.getWorldPtr(), albedo, scale, points)
        got = NZ.value(tab, np.array(albedo, F), F(scale), points)
        assert bits_equal(got, exp), mismatch_report(got, exp)
    assert len(points) >= 4096 and np.unique(exp, axis=0).shape[0] > 4000


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
@pytest.mark.parametrize("kind", TW.CAMERAS)
def test_the_wide_room_with_its_medium_under_every_camera(p, kind, as_list):
    scene = TW.wide_room(p, ext=2, medium=True, as_list=as_list)
    stats = {}
    compare(scene, TW.camera(p, TW.W, TW.H, kind), TW.W, TW.H, TW.SPP, TW.DEPTH, TW.SEED, stats)
    counts = {k: int(stats.get(k, 0)) for k in COUNTERS + ("lens_draws", "time_draws")}
    print(f"wide_room {kind} {'list' if as_list else 'bvh'}: {counts}")
    for name in ("medium_draws", "medium_hits", "medium_scatters", "noise_hits"):
        assert counts[name] > 0, name
    assert counts["lens_draws"] > 0 if kind == "defocus" else counts["lens_draws"] == 0
    assert counts["moving_hits"] > 0 if kind == "motion" else counts["moving_hits"] == 0


@pytest.mark.parametrize("i", range(8))
def test_random_mixed_worlds_with_media_under_the_motion_camera(p, i):
    rng = np.random.default_rng(3300 + i)
    scene, oracle_scene = random_mixed_scene(p, rng, 24, 8, i % 4, background=(0.5, 0.6, 0.8) if i % 2 else None, media=True)   # three flat builders and the list
    prims = scene.arrays()[1]
    assert (prims["mat"] & np.uint32(0x80000000)).any()
    w, h = 24, 16
    cam = p.MotionBlurCamera((9, 3, 9), (0, 0, 0), (0, 1, 0), 55.0, w / h, 0.0, 1.0)
    stats = {}
    compare(scene, cam, w, h, 4, 8, 1984 + i, stats)
    print(f"random mixed {i}: { {k: int(stats.get(k, 0)) for k in COUNTERS} }")
    assert stats["medium_draws"] > 0 and stats["moving_hits"] > 0 and stats["time_draws"] == w * h * 4
    assert oracle_scene is not None


def nested_media_world(p, as_list=False):
    """a medium sphere inside a glass sphere, another medium overlapping a moving sphere, and a thin haze about them all: one walk tests two media and more"""
    s = p.Scene()
    s.MakeQuad((-8, 0, -8), (16, 0, 0), (0, 0, 16), s.Lambertian((0.6, 0.6, 0.55)))
    s.MakeQuad((-2, 6, -2), (4, 0, 0), (0, 0, 4), s.DiffuseLight((6, 6, 6)))
    s.MakeSphere((-1.6, 1.5, 0), 1.5, s.Dielectric((1, 1, 1), 1.5))
    s.MakeSphere((-1.6, 1.5, 0), 1.1, s.Isotropic((0.2, 0.4, 0.9), 0.9))
    s.MakeMovingSphere((1.8, 1.0, 0.2), (1.8, 1.9, 0.2), 0.9, s.Lambertian((0.8, 0.3, 0.2)))
    s.MakeSphere((2.3, 1.6, 0.6), 1.2, s.Isotropic((0.9, 0.9, 0.9), 0.6))
    s.MakeMovingSphere((0, 2.5, 1), (0.4, 2.5, 1), 7.0, s.Isotropic((0.8, 0.8, 0.8), 0.03))
    s.set_background((0.4, 0.5, 0.7))
    s.MakeHittableList() if as_list else s.BuildBVH_SAH()
    return s


@pytest.mark.parametrize("as_list", [False, True], ids=["bvh", "list"])
def test_a_medium_inside_glass_and_a_medium_over_a_moving_sphere(p, as_list):
    scene = nested_media_world(p, as_list)
    w, h = 24, 16
    cam = p.MotionBlurCamera((0, 2.2, 7.5), (0, 1.4, 0), (0, 1, 0), 50.0, w / h, 0.0, 1.0)
    stats, two = {"glass": 0}, [0, 0]

    def trace(world, rays, **draws):   # counts the walks in which two or more medium tests drew
        tape, rows = draws["tape"], draws["rows"]
        before = tape.cur[rows].copy()
        out = TT.closest_intersection(world, rays, **draws)
        two[0] += int(((tape.cur[rows] - before) >= 2).sum())
        two[1] += int(((tape.cur[rows] - before) >= 3).sum())
        return out

    compare(scene, cam, w, h, 4, 8, 1984, stats, trace)
    print(f"nested media {'list' if as_list else 'bvh'}: { {k: int(stats.get(k, 0)) for k in COUNTERS} }, walks with >= 2 draws {two[0]}, >= 3 draws {two[1]}, "
          f"glass hits {stats.get('glass', 0)}")
    for name in COUNTERS[:3] + ("moving_hits",):
        assert stats[name] > 0, name
    assert two[0] > 0
