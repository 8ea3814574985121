"""The renderer's launch images under one walk of setters and modes: whatever order the light-sampling modes, the vertex normals, the texture
coordinates, the environment map and the texture table came in, a launch runs on the image a fresh renderer in that state runs on.

One renderer per kernel form walks one fixed list of steps over _tex_worlds.riders_room; after every step its frame is held, bit for bit, (a) against a fresh
renderer put into the step's state in one canonical order (tables, map, mode), (b) through its FNV-1a-64 against tests/golden/launch_image_walk.json, recorded
by record() below on the commit BEFORE the images were folded into one composer, and (c) its state queries against what the state implies.

    python tests/test_gpu_launch_images.py [out.json]     records the golden file (needs a GPU); it checks (a) and (c) on the way
"""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import pytest

import _tex_worlds as XW
import _tri_worlds as TW
from _common import ROOT, bits_equal, mismatch_report, pkg

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH, SEED = 24, 16, 4, 6, 1984
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_image_walk.json")
# the three forms whose image handling differs: the image in the LDS, a list, the image in global memory
FORMS = {"lds": (TW.BVH, 0, 2, 0, 0), "list": (TW.LIST, 1, 2, 0, 0), "global": (TW.BVH, 0, 2, 1, 0)}
# riders_room's lights: a quad, a sphere and a triangle; its map is 16 x 8
LIGHTS = {0: 1, 1: 1, 2: 2, 4: 3, 16: 3, 32: 16 * 8, 48: 3}

# a state is (mode, normals on, coordinates on, map, table); a step is the calls that lead to it from the state before
FIRST = (48, False, False, "A", "A")
PRELUDE = [("mode", 1), ("mode", 2), ("mode", 4), ("mode", 16), ("mode", 0),   # every table mode before anything is given: nothing can be rendered yet
           ("env", "A"), ("mode", 32), ("mode", 48), ("tab", "A")]             # ... and the two modes of the map before any table
WALK = [
    (PRELUDE, FIRST),
    ([("mode", 0)], (0, False, False, "A", "A")),
    ([("vn", True)], (0, True, False, "A", "A")),
    ([("uv", True)], (0, True, True, "A", "A")),
    ([("mode", 1)], (1, True, True, "A", "A")),                 # every mode once more, the tables on
    ([("mode", 2)], (2, True, True, "A", "A")),
    ([("tab", "B")], (2, True, True, "A", "B")),               # the table replaced while mode 2 is on
    ([("mode", 4)], (4, True, True, "A", "B")),
    ([("uv", False)], (4, True, False, "A", "B")),             # coordinates dropped while mode 4 is on
    ([("mode", 16)], (16, True, False, "A", "B")),
    ([("vn", False)], (16, False, False, "A", "B")),           # normals dropped and given back while mode 16 is on
    ([("vn", True)], (16, True, False, "A", "B")),
    ([("mode", 32)], (32, True, False, "A", "B")),
    ([("env", "B")], (32, True, False, "B", "B")),             # the map replaced while mode 32 is on
    ([("mode", 0)], (0, True, False, "B", "B")),               # 32 -> 0 -> 32
    ([("mode", 32)], (32, True, False, "B", "B")),
    ([("mode", 48)], (48, True, False, "B", "B")),
    ([("env", "A")], (48, True, False, "A", "B")),             # the map replaced while mode 48 is on
    ([("mode", 16)], (16, True, False, "A", "B")),             # 48 -> 16 -> 48
    ([("mode", 48)], (48, True, False, "A", "B")),
    ([("uv", True)], (48, True, True, "A", "B")),
    ([("tab", "A")], (48, True, True, "A", "A")),
    ([("vn", False)], (48, False, True, "A", "A")),
    ([("uv", False)], FIRST),                                    # back where the walk began
]
assert len(WALK) >= 20 and WALK[-1][1] == WALK[0][1]


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@contextlib.contextmanager
def form_env(env):
    """the environment a renderer of this form is created under"""
    keys = ("RT06_FORCE_BIG", "RT06_FORCE_WIDE")
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class Riders:
    """riders_room in one form, and what the setters are given: its own tables, map A and table A, and a second map and a second table"""

    def __init__(self, name):
        self.p, self.name, self.form = pkg(), name, FORMS[name]
        self.variant, self.env = TW.FORMS[self.form]
        self.scene = XW.riders_room(self.p, as_list=self.form[0] == TW.LIST)
        self.cam = XW.camera(self.p)
        self.normals, self.uvs = self.scene.vertex_normals().copy(), self.scene.texture_coords().copy()
        env_a, self.u0 = self.scene.environment()
        self.maps = {"A": env_a, "B": (np.roll(env_a, 3, axis=1)[::-1] * np.float32(0.5) + np.float32(0.05)).astype(np.float32)}
        records, texels = self.scene.textures()
        other = records.copy()
        other["wrap"] ^= 1      # the same images under the other wrap and the other filter
        other["filter"] ^= 1
        self.tables = {"A": (records.copy(), texels.copy()), "B": (other, texels.copy())}

    def bare(self):
        """a renderer of the world without any of its riders"""
        world = self.scene.getWorldPtr()
        for rider in ("vertex_normals", "texture_coords", "environment", "textures"):
            if hasattr(world, rider):
                delattr(world, rider)
        with form_env(self.env):
            r = self.p.Renderer.MakeRenderer(W, H, SPP, DEPTH, self.cam, world, seed=SEED, variant=self.variant)
        assert r.kernel_form() == TW.kernel_form_of(self.form) and not r.textures_info()["enabled"] and not r.environment_info()["enabled"]
        return r

    def apply(self, r, call):
        what, arg = call
        if what == "mode":
            r.light_sampling(arg)
        elif what == "vn":
            r.shading_normals(self.normals if arg else None)
        elif what == "uv":
            r.texture_coords(self.uvs if arg else None)
        elif what == "env":
            r.environment(self.maps[arg], u0=self.u0)
        else:
            r.textures(self.tables[arg])

    def check_queries(self, r, state):
        mode, vn, uv, _, _ = state
        assert r.kernel_form() == TW.kernel_form_of(self.form, nee=1 if mode else 0)
        assert r.kernel_env_light() == (mode in (32, 48)) and r.kernel_light_tree() == (mode in (16, 48)) and r.kernel_triangles()
        assert r.light_sampling_mode() == mode and r.light_sampling_info() == {"enabled": mode != 0, "lights": LIGHTS[mode]}
        assert r.shading_normals_info()["enabled"] == vn and r.texture_coords_info()["enabled"] == uv
        assert r.environment_info()["enabled"] and r.textures_info() == {"enabled": True, "entries": 3}

    @functools.lru_cache(maxsize=None)
    def fresh_frame(self, state):
        """the frame of a fresh renderer put into `state` in the canonical order: tables, then the map, then the mode"""
        mode, vn, uv, env, tab = state
        r = self.bare()
        for call in [("vn", True)] * vn + [("uv", True)] * uv + [("tab", tab), ("env", env), ("mode", mode)]:
            self.apply(r, call)
        self.check_queries(r, state)
        r.Render()
        frame = r.DownloadRenderbuffer()
        r.close()
        frame.setflags(write=False)
        return frame

    def walk(self):
        """yields (step, state, frame) of one renderer led through WALK"""
        r = self.bare()
        try:
            for k, (calls, state) in enumerate(WALK):
                for call in calls:
                    self.apply(r, call)
                self.check_queries(r, state)
                r.Render()
                yield k, state, r.DownloadRenderbuffer()
        finally:
            r.close()


@pytest.fixture(scope="module")
def golden():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(FORMS))
def test_the_walk_renders_what_fresh_renderers_and_the_parent_render(golden, name):
    riders = Riders(name)
    assert golden["steps"] == [list(state) for _, state in WALK]   # the file was recorded for this walk
    frames = {}
    for k, state, frame in riders.walk():
        want = riders.fresh_frame(state)
        assert bits_equal(frame, want), (k, state, mismatch_report(frame, want))                 # (a)
        assert f"{fnv1a(frame.tobytes()):016x}" == golden["fnv"][name][k], (k, state)          # (b)
        frames.setdefault(state, frame)
    assert len({f.tobytes() for f in frames.values()}) == len(frames)   # no two states render one frame: every setter reached the image


def record(path):
    out = {"steps": [list(state) for _, state in WALK], "fnv": {}}
    for name in FORMS:
        riders, hashes = Riders(name), []
        for k, state, frame in riders.walk():
            want = riders.fresh_frame(state)
            if not bits_equal(frame, want):
                print(f"{name} step {k} {state}: NOT the fresh renderer's frame: {mismatch_report(frame, want)}")
            hashes.append(f"{fnv1a(frame.tobytes()):016x}")
        out["fnv"][name] = hashes
        print(name, len(hashes), "steps,", len({state for _, state in WALK}), "states,", len(set(hashes)), "distinct frames")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("recorded", path)


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
