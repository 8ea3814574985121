#!/usr/bin/env python3
"""What the full feature mode costs and buys (EXPERIMENTS.md E28).  One GPU.  Sections, any subset of:

    python tools/aov_full_cost.py --parent-lib PATH ab     # PATH: librt06.so built from the commit to compare with
    python tools/aov_full_cost.py modes quality            # this tree only

  ab       the feature kernels of modes 0 and 1 are unchanged, so a refine step in mode 1 must cost what it cost: the textured room of tools/aov_textured_cost.py's
           kind (tests/_tex_worlds.routing_room) at 400 x 400, 16 samples a step, depth 50, this tree's library against the parent's in alternating rounds, each
           round of each library in a process of its own; host clock around the synchronous step, best, median and worst of 7 steps.  The last lines are the
           median over the rounds of each library's medians, their ratio, and the parent's own round-to-round spread.
  modes    on this tree: mode 2 against mode 1 on that room (a world both take); and on the cutout room under the sky map and the fog room (tests/_aov_full_worlds.room) features
           off against mode 2 — their difference is the feature pass — beside the streaming kernel's own HIP-event time of the same step.
  quality  the same two rooms at 16 and 64 samples against --reference-spp samples of the same world under another seed: RMSE over the frame (the
           displayed values) of the noisy frame and of the denoised one, with the default parameters and with demodulate = 0.
Every line starts with its section's name."""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("sections", nargs="*", default=["modes", "quality"])
ap.add_argument("--parent-lib", default=None, help="librt06.so of the commit to compare with (section ab)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", type=int, default=400)
ap.add_argument("--reference-spp", type=int, default=4096)
ap.add_argument("--one-round", default=None, help=argparse.SUPPRESS)   # the child of section ab: one round of one library, named here
a = ap.parse_args()
W = H = a.size
DEPTH, STEP = 50, 16


def load():
    import numpy as np
    import __graft_entry__ as G
    return G.load_package(), np


def step_times(np, renderers, rounds=7):
    """{name: (sorted host ms of refine(STEP), sorted streaming-kernel ms)}, the renderers taking turns within every round"""
    host, kern = {k: [] for k in renderers}, {k: [] for k in renderers}
    for r in renderers.values():   # warm up: code objects, buffers
        r.refine(STEP)
    for _ in range(rounds):
        for name, r in renderers.items():
            r.refine_reset()
            t0 = time.perf_counter()
            r.refine(STEP)
            host[name].append((time.perf_counter() - t0) * 1e3)
            kern[name].append(r.kernel_times()[1])
    return {k: (sorted(host[k]), sorted(kern[k])) for k in renderers}


def report(section, label, res):
    for name, (h, k) in res.items():
        print(section, label, name, "refine(%d) host ms best %.3f median %.3f worst %.3f | streaming kernel ms median %.3f" % (STEP, h[0], h[len(h) // 2], h[-1], k[len(k) // 2]), flush=True)


if a.one_round:   # section ab's child
    p, np = load()
    import _tex_worlds as XW
    import _tri_worlds as TW
    scene = XW.routing_room(p)
    r = p.Renderer.MakeRenderer(W, H, STEP, DEPTH, TW.camera(p, W, H), scene.getWorldPtr())
    r.enable_aov(textured=True)
    h = step_times(np, {"m": r})["m"][0]
    print("ab", a.one_round, p.lib().rt_source_hash().decode()[:12], "mode 1 refine(%d) host ms best %.3f median %.3f worst %.3f" % (STEP, h[0], h[len(h) // 2], h[-1]), flush=True)
    r.close()
    sys.exit(0)

if "ab" in a.sections:
    import re
    import statistics
    assert a.parent_lib, "section ab needs --parent-lib"
    medians = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, lib in (("parent", os.path.abspath(a.parent_lib)), ("this", None)):
            env = dict(os.environ)
            env.pop("RT06_LIB", None)
            if lib:
                env["RT06_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-round", name, "--size", str(a.size)], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:   # nothing more is started on the GPU after a failure
                sys.exit("ab: a round of %s failed (%d): %s" % (name, out.returncode, out.stderr[-400:]))
            sys.stdout.write(out.stdout)
            sys.stdout.flush()
            medians[name].append(float(re.search(r"median ([0-9.]+)", out.stdout).group(1)))
    mp, mt = statistics.median(medians["parent"]), statistics.median(medians["this"])
    print("ab summary: median of the rounds' medians, parent %.3f ms, this %.3f ms, ratio this / parent %.4f; the parent's own rounds span %.3f to %.3f ms (%.4f of their median)"
          % (mp, mt, mt / mp, min(medians["parent"]), max(medians["parent"]), (max(medians["parent"]) - min(medians["parent"])) / mp), flush=True)

if "modes" in a.sections or "quality" in a.sections:
    p, np = load()
    import _aov_full_worlds as FW
    import _tex_worlds as XW
    import _tri_worlds as TW
    print("source", p.lib().rt_source_hash().decode(), flush=True)
    rooms = {"cutout room under the sky map": dict(env=True), "fog room": dict(masks=False, fog=True)}

if "modes" in a.sections:
    scene, cam = XW.routing_room(p), TW.camera(p, W, H)
    rs = {k: p.Renderer.MakeRenderer(W, H, STEP, DEPTH, cam, scene.getWorldPtr()) for k in ("features off", "mode 1", "mode 2")}
    rs["mode 1"].enable_aov(textured=True)
    rs["mode 2"].enable_aov(full=True)
    report("modes", "textured room", step_times(np, rs))
    print("modes textured room: the feature sums of modes 1 and 2 have the same bits:", np.array_equal(rs["mode 1"].aov_sums().view(np.uint32), rs["mode 2"].aov_sums().view(np.uint32)), flush=True)
    for r in rs.values():
        r.close()
    for label, kw in rooms.items():
        scene, cam = FW.room(p, **kw), FW.camera(p, W, H)
        rs = {k: p.Renderer.MakeRenderer(W, H, STEP, DEPTH, cam, scene.getWorldPtr()) for k in ("features off", "mode 2")}
        rs["mode 2"].enable_aov(full=True)
        report("modes", label, step_times(np, rs))
        for r in rs.values():
            r.close()

if "quality" in a.sections:
    for label, kw in rooms.items():
        scene, cam = FW.room(p, **kw), FW.camera(p, W, H)
        ref = p.Renderer.MakeRenderer(W, H, 64, DEPTH, cam, scene.getWorldPtr(), seed=7)   # another seed than the frames it judges
        for _ in range(a.reference_spp // 64):
            ref.refine(64)
        truth = ref.DownloadRenderbuffer()[..., 0:3].astype(np.float64)
        ref.close()
        rmse = lambda img: float(np.sqrt(np.mean((img[..., 0:3].astype(np.float64) - truth) ** 2)))   # noqa: E731
        for spp in (16, 64):
            r = p.Renderer.MakeRenderer(W, H, 16, DEPTH, cam, scene.getWorldPtr())
            r.enable_aov(full=True)
            for _ in range(spp // 16):
                r.refine(16)
            noisy, den, flat = r.DownloadRenderbuffer(), r.denoise(), r.denoise(demodulate=0)
            print("quality %s, %d spp against %d spp, %d x %d: RMSE noisy %.5f | denoised, default parameters %.5f | denoised, demodulate = 0 %.5f"
                  % (label, spp, a.reference_spp, W, H, rmse(noisy), rmse(den), rmse(flat)), flush=True)
            r.close()
