"""The probes' plumbing (csrc/rt_probes.hip: uploads, strides, grids, downloads, refusals) — not their arithmetic, which
tests/test_gpu_parity.py and tests/test_reference_pins.py hold to the oracle and to the reference.

Every probe runs on one fixed random batch of 129 cases and on its prefixes of 1, 127 and 128 cases: each output array of a
prefix run must equal, bit for bit, the prefix of the 129-case run.  127 / 128 / 129 straddle the 128-thread block, 1 is the
smallest launch, and the last case of each run sits at the end of every buffer, so an array uploaded or downloaded with the
wrong stride shows up there.
"""
import numpy as np
import pytest

from _common import config_scene, pkg, random_rays

pytestmark = pytest.mark.gpu

N = 129
PREFIXES = (1, 127, 128)
PER_TAPE = 64         # tape entries per case: a rejection loop that has not accepted after 21 tries (0.48^21 ~ 2e-7) would run off them
FLT_MAX = np.float32(3.402823466e38)
RT_ERR_INVALID = 1   # include/rt06.h


@pytest.fixture(scope="module")
def p():
    m = pkg()
    assert m.api.device_count() >= 1, "no HIP device: the gpu tests need an MI355X"
    return m


@pytest.fixture(scope="module")
def batch(p):
    """The 129 cases of every probe, as {probe: run(k) -> tuple of output arrays for the first k cases}."""
    rng = np.random.default_rng(129)
    api = p.api
    lo = ((rng.random((N, 3), dtype=np.float32) * 2 - 1) * 10).astype(np.float32)
    ext = (rng.random((N, 3), dtype=np.float32) * 4 + 0.01).astype(np.float32)
    boxes = np.concatenate([lo, lo + ext], axis=1)
    rlo = (lo + ext * (rng.random((N, 3), dtype=np.float32) - 0.5)).astype(np.float32)
    pairs = np.ascontiguousarray(np.concatenate([boxes, rlo, rlo + ext], axis=1), dtype=np.float32)
    rays6 = random_rays(rng, N, with_time=False)
    k = np.arange(N) % 3 != 0                                # two thirds aim at a point of the left box; the rest mostly miss
    rays6[k, 3:6] = (lo + ext * rng.random((N, 3), dtype=np.float32) - rays6[:, 0:3])[k]
    rays7 = random_rays(rng, N, spread=5.0)
    maxd = np.where(rng.random(N) < 0.5, FLT_MAX, rng.random(N, dtype=np.float32) * 30).astype(np.float32)
    spheres = np.concatenate([(rng.random((N, 3), dtype=np.float32) * 2 - 1) * 8, rng.random((N, 1), dtype=np.float32) * 2 + 0.05], axis=1)
    prims = np.zeros(N, dtype=p.capi.PRIM_DT)
    prims["c0"] = spheres[:, 0:3]; prims["c1"] = spheres[:, 0:3] + 0.25; prims["radius"] = spheres[:, 3]
    prims["mat"] = np.where(np.arange(N) % 3 == 0, 0x80000000, 0)
    aimed = rays7.copy()
    aimed[:, 3:6] = spheres[:, 0:3] - aimed[:, 0:3]
    mats = np.zeros(N, dtype=p.capi.MAT_DT)
    mats["albedo"] = rng.random((N, 3), dtype=np.float32); mats["albedo2"] = rng.random((N, 3), dtype=np.float32)
    mats["type"] = np.arange(N) % 4
    mats["param"] = np.float32([0.0, 0.3, 1.5, 3.125])[np.arange(N) % 4]
    normals = rng.standard_normal((N, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True).astype(np.float32)
    dist = (rng.random(N, dtype=np.float32) * 20).astype(np.float32)
    keys = rng.integers(0, 2**31, size=(N, 2), dtype=np.uint32)
    tape = rng.integers(1, (1 << 24) + 1, size=N * PER_TAPE, dtype=np.uint32)
    offsets = np.stack([np.arange(N) * PER_TAPE, np.full(N, PER_TAPE)], axis=1).astype(np.uint32)
    st = (rng.random((N, 2), dtype=np.float32) * 2 - 1).astype(np.float32)
    cam = p.DefocusBlurCamera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 1.5, 0.1, 10.0)
    a, b = (rng.random(N, dtype=np.float32) * 2 - 1).astype(np.float32), (rng.random(N, dtype=np.float32) * 2 - 1).astype(np.float32)
    glm_dot, glm_ray = rng.standard_normal((N, 6)).astype(np.float32), rng.standard_normal((N, 10)).astype(np.float32)
    scene = config_scene(p, "three_spheres")
    world = scene.getWorldPtr()
    to_world = rays7.copy()                                  # three quarters towards the middle sphere, a quarter up and away
    to_world[:, 3:6] = np.float32([0, 0, -1]) - to_world[:, 0:3] + (rng.random((N, 3), dtype=np.float32) - 0.5)
    to_world[3::4, 3:6] *= -1
    to_world[3::4, 4] = np.abs(to_world[3::4, 4])

    def one(x):
        return x if isinstance(x, tuple) else (x,)

    runs = {
        "aabb": lambda k: api.probe_aabb(boxes[:k], rays6[:k], maxd[:k]),
        "sphere": lambda k: api.probe_sphere(rays6[:k], spheres[:k]),
        "sphere_hit": lambda k: api.probe_sphere_hit(prims[:k], aimed[:k], maxd[:k]),
        "scatter": lambda k: api.probe_scatter(1984, mats[:k], rays7[:k], dist[:k], normals[:k], keys[:k]),
        "scatter_tape": lambda k: api.probe_scatter_tape(mats[:k], rays7[:k], dist[:k], normals[:k], tape[:k * PER_TAPE], offsets[:k]),
        "camera": lambda k: api.probe_camera(1984, cam, st[:k], keys[:k]),
        "camera_tape": lambda k: api.probe_camera_tape(cam, st[:k], tape[:k * PER_TAPE], offsets[:k]),
        "rng": lambda k: api.probe_rng(1984, keys[:k], 5),
        "math": lambda k: api.probe_math(3, a[:k], b[:k]),
        "glm_dot": lambda k: api.probe_glm("dot", glm_dot[:k]),
        "glm_ray": lambda k: api.probe_glm("ray", glm_ray[:k]),
        "aabb_regular": lambda k: api.probe_aabb_regular(boxes[:k], rays6[:k], maxd[:k]),
        "boxpair_filtered": lambda k: api.probe_boxpair_filtered(pairs[:k], rays6[:k], maxd[:k]),
        "boxpair_certified": lambda k: api.probe_boxpair_certified(pairs[:k], rays6[:k], maxd[:k]),
        "trace": lambda k: api.probe_trace(world, to_world[:k]),
    }
    full = {name: one(run(N)) for name, run in runs.items()}
    for outs in full.values():
        for o in outs:
            o.setflags(write=False)
    return {"runs": {name: (lambda k, run=run: one(run(k))) for name, run in runs.items()}, "full": full, "scene": scene,
            "inputs": dict(mats=mats, rays7=rays7, dist=dist, normals=normals, keys=keys, tape=tape, offsets=offsets, st=st, cam=cam)}


PROBES = ("aabb", "sphere", "sphere_hit", "scatter", "scatter_tape", "camera", "camera_tape", "rng", "math", "glm_dot", "glm_ray",
          "aabb_regular", "boxpair_filtered", "boxpair_certified", "trace")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", PROBES)
def test_prefix_runs_return_the_prefix_of_the_full_run(batch, name):
    full = batch["full"][name]
    assert all(len(o) == N for o in full)
    for k in PREFIXES:
        got = batch["runs"][name](k)
        assert len(got) == len(full)
        for j, (g, f) in enumerate(zip(got, full)):
            assert same_bits(g, f[:k]), f"{name}: output {j} of the {k}-case run differs from the {N}-case run's prefix at rows " \
                                        f"{np.nonzero((g != f[:k]).reshape(k, -1).any(axis=1))[0][:5]}"


def test_the_batch_exercises_the_probes(batch):
    """(a batch on which a probe returned all zeros would let a download that never happened pass the prefix test)"""
    full = batch["full"]
    for name in PROBES:
        assert any(o.any() for o in full[name]), name
    assert 0 < full["aabb"][0].sum() < N and 0 < full["sphere_hit"][0].sum() and 0 < full["trace"][0].sum() < N
    assert full["boxpair_certified"][0][:, 0].mean() > 0.9 and 0 < full["boxpair_certified"][0][:, 5].sum() < N
    assert full["scatter"][3].any() and full["scatter_tape"][3].any() and full["camera"][1].all() and full["camera_tape"][1].all()
    assert (full["scatter_tape"][3] <= PER_TAPE).all() and (full["camera_tape"][1] <= PER_TAPE).all()   # no case ran off its tape


@pytest.mark.parametrize("name", PROBES)
def test_no_cases_is_no_error_and_empty_arrays(batch, name):
    got = batch["runs"][name](0)
    assert len(got) == len(batch["full"][name])
    for g, f in zip(got, batch["full"][name]):
        assert g.dtype == f.dtype and g.shape == (0,) + f.shape[1:]


def test_refusals_keep_their_words(p, batch):
    api, i = p.api, batch["inputs"]

    class refused:   # RT_ERR_INVALID with these words
        def __init__(self, words):
            self.ctx = pytest.raises(p.capi.RtError, match=words)

        def __enter__(self):
            self.info = self.ctx.__enter__()

        def __exit__(self, *exc):
            done = self.ctx.__exit__(*exc)
            assert self.info.value.code == RT_ERR_INVALID
            return done

    bad = i["mats"].copy()
    bad["type"][77] = 99
    with refused(r"rt_probe_scatter: case 77: unknown material type"):
        api.probe_scatter(1984, bad, i["rays7"], i["dist"], i["normals"], i["keys"])
    with refused(r"rt_probe_scatter_tape: case 77: unknown material type"):
        api.probe_scatter_tape(bad, i["rays7"], i["dist"], i["normals"], i["tape"], i["offsets"])
    short = i["tape"][:-1]   # the last case's range now ends one past the tape
    last = (N - 1) * PER_TAPE
    words = rf"case {N - 1}: tape range \[{last}, \+{PER_TAPE}\) outside a tape of {len(short)}"
    with refused("rt_probe_scatter_tape: " + words):
        api.probe_scatter_tape(i["mats"], i["rays7"], i["dist"], i["normals"], short, i["offsets"])
    with refused("rt_probe_camera_tape: " + words):
        api.probe_camera_tape(i["cam"], i["st"], short, i["offsets"])
    odd = type(i["cam"]).from_buffer_copy(i["cam"])
    odd.type = 99
    with refused(r"rt_probe_camera: unknown camera type"):
        api.probe_camera(1984, odd, i["st"], i["keys"])
    with refused(r"rt_probe_camera_tape: unknown camera type"):
        api.probe_camera_tape(odd, i["st"], i["tape"], i["offsets"])
    with refused(r"rt_selftest_fastdiv: significand range out of bounds"):
        api.selftest_fastdiv(0, 0)
    with refused(r"rt_selftest_fastdiv: exponent out of range"):
        api.selftest_fastdiv(0, 1, num_exp=128)
    with refused(r"rt_selftest_fastdiv4: exponent out of range"):
        api.selftest_fastdiv(0, 1, den_exp=128, four=True)


@pytest.mark.parametrize("four", [False, True])
def test_fastdiv_selftest_counts_from_zero(p, four):
    """Two blocks (two divisor significands x 2^23 numerators); the mismatch counter and the example start cleared."""
    bad, ex = p.api.selftest_fastdiv(0, 2, four=four)
    assert bad == 0 and not ex.any()
