"""Adaptive sampling (pbr_render_adaptive) timed on one GPU: what the mechanism costs when nothing stops, and what it buys.

  python scripts/adaptive_render.py [--what cost,buys] [--scenes sponza,cornell] [--reps 5] [--thresholds 0.02,0.05,0.1]

Sponza-class (N = 64 frames) and Cornell box (N = 256) as BASELINE.json has them, 1920 x 1080.  Per scene: a warm-up with
pbr_render that lets the schedule tuner settle (pbr_diag_tune_budget frames); the plan it keeps is pinned for every leg.
Times are the device time the library reports for the whole call (pbr_last_kernel_ms: launches, folds and, for an adaptive
call, the host's table building between the rounds) and the wall time around the synchronous call; medians over --reps
repetitions with the spread (min .. max), the legs of a repetition in alternation.

  cost   render( N )  |  render_adaptive( min = max = N ): one round, the heavier fold  |  render_adaptive( min = round = 16,
         max = N, threshold 0 ): a test every 16 frames, only tiles whose frames are exactly constant stop (their share is
         printed: the comparison means "nothing stops" only where it is small).  The adaptive legs' difference to
         render( N ) per round is the price of a round.
  buys   per threshold: device time, units traced / ( W x H x N ), RMSE (rgb) against a 4096-frame render, next to the
         uniform render( n ) whose time is nearest (n from render( N )'s time per frame) and ITS RMSE.

To time another build of the library (the parent commit's), start the script with PBR_LAB_ENV=1 and
PBR_HIP_LIB=<that libpbrhip.so>; a library without pbr_render_adaptive runs the render( N ) leg only.  Run the builds in
alternation, each in a process of its own, and compare only differences larger than the spread of the repetitions."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pbr_loader  # noqa: E402

W, H = 1920, 1080
SCENES = {"sponza": ("sponza", 2, 260000, 3, 64), "cornell": ("cornell", 1, 0, 8, 256)}
REFERENCE_FRAMES = 4096


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(values):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(values)), min(values), max(values))


def rmse(image, reference):
    d = (image[..., :3].astype(np.float64) - reference[..., :3].astype(np.float64)) ** 2
    return float(np.sqrt(np.nanmean(d)))


def main():
    pbr = pbr_loader.load()
    what = arg("--what", "cost,buys").split(",")
    reps = int(arg("--reps", "5"))
    thresholds = [float(t) for t in arg("--thresholds", "0.02,0.05,0.1").split(",")]
    label = arg("--label", os.environ.get("PBR_HIP_LIB", "product"))
    adaptive = hasattr(pbr.hip, "pbr_render_adaptive")
    lines = []
    for name in arg("--scenes", "sponza,cornell").split(","):
        kind, seed, tris, depth, n = SCENES[name]
        pbr.cfg_reset()
        pbr.cfg_set(**{"render.max_depth": depth})
        sc = pbr.HostScene.generate(kind, seed, tris)
        cfg, cam, px, seeds = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H), pbr.frame_seeds(0, n)
        dev = pbr.Device(0)
        dev.upload_scene(sc.desc)
        dev.configure(cfg)
        dev.render(0, pbr.frame_seeds(0, max(dev.tune_budget(), n)), px, cam)
        dev.reset_accum()
        dev.render(0, seeds, px, cam)
        plan, tuned = dev.last_plan()
        if tuned >= 0:
            dev.pin_plan(tuned)
        print("== %s  %d x %d  N = %d  plan %s (%s)  library %s" % (name, W, H, n, plan, "pinned" if tuned >= 0 else "the tuner had not settled", label), flush=True)

        def timed(call):
            dev.reset_accum()
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3, dev.last_kernel_ms()

        legs = {"render(N)": lambda: dev.render(0, seeds, px, cam)}
        if adaptive:
            legs["adaptive min=max=N"] = lambda: dev.render_adaptive(0, seeds, px, cam, n, 16, n, 0.0)
            legs["adaptive 16/16/N thr 0"] = lambda: dev.render_adaptive(0, seeds, px, cam, 16, 16, n, 0.0)
        per_frame_ms = None
        if "cost" in what:
            result = {leg: {"wall": [], "device": [], "fold": [], "rounds": 0, "stopped": 0.0} for leg in legs}
            for leg, call in legs.items():      # once untimed: buffers grown, plans built
                timed(call)
            for _ in range(reps):
                for leg, call in legs.items():
                    wall, device = timed(call)
                    r = result[leg]
                    r["wall"].append(wall)
                    r["device"].append(device)
                    if leg != "render(N)":
                        rounds, units, fold_ms = dev.last_adaptive()
                        r["fold"].append(fold_ms)
                        r["rounds"] = rounds
                        r["stopped"] = float((dev.tile_stats()[0] < n).mean())
            base = float(np.median(result["render(N)"]["device"]))
            per_frame_ms = base / n
            for leg, r in result.items():
                extra = ""
                if leg != "render(N)":
                    over = float(np.median(r["device"])) - base
                    extra = "  fold %s ms  rounds %d  over render(N) %+.3f ms = %+.2f %% = %+.3f ms / round  tiles stopped %.2f %%" % (
                        spread(r["fold"]), r["rounds"], over, 100.0 * over / base, over / r["rounds"], 100.0 * r["stopped"])
                print("%-24s device ms %s  wall ms %s%s" % (leg, spread(r["device"]), spread(r["wall"]), extra), flush=True)
                lines.append({"scene": name, "library": label, "leg": leg, "frames": n, "plan": plan, "device_ms": r["device"], "wall_ms": r["wall"],
                              "fold_ms": r["fold"], "rounds": r["rounds"], "tiles_stopped": r["stopped"]})
        if "buys" in what and adaptive:
            if per_frame_ms is None:
                per_frame_ms = float(np.median([timed(legs["render(N)"])[1] for _ in range(3)])) / n
            dev.reset_accum()
            dev.render(0, pbr.frame_seeds(0, REFERENCE_FRAMES), px, cam)
            reference = dev.read_output()
            dev.reset_accum()
            dev.render(0, seeds, px, cam)
            print("render(N)                device ms %9.3f  RMSE %.5f against %d frames" % (dev.last_kernel_ms(), rmse(dev.read_output(), reference), REFERENCE_FRAMES), flush=True)
            for threshold in thresholds:
                times = []
                for _ in range(reps):
                    times.append(timed(lambda: dev.render_adaptive(0, seeds, px, cam, 16, 16, n, threshold))[1])
                image, (frames, _) = dev.read_output(), dev.tile_stats()
                rounds, units, fold_ms = dev.last_adaptive()
                share = units / float(W * H * n)
                same_time = max(1, min(n, int(round(float(np.median(times)) / per_frame_ms))))
                uniform = [timed(lambda: dev.render(0, seeds[:same_time], px, cam))[1] for _ in range(reps)]
                uniform_rmse = rmse(dev.read_output(), reference)
                hist = {int(c): int(k) for c, k in zip(*np.unique(frames, return_counts=True))}
                print("threshold %-6g adaptive device ms %s  units %.3f of uniform  rounds %d  RMSE %.5f   |   render( %d ) device ms %s  RMSE %.5f" % (
                    threshold, spread(times), share, rounds, rmse(image, reference), same_time, spread(uniform), uniform_rmse), flush=True)
                print("                 frames per tile: %r" % hist, flush=True)
                lines.append({"scene": name, "library": label, "threshold": threshold, "device_ms": times, "units_share": share, "rounds": rounds,
                              "rmse": rmse(image, reference), "uniform_frames": same_time, "uniform_device_ms": uniform, "uniform_rmse": uniform_rmse,
                              "frames_per_tile": hist})
        dev.close()
    for line in lines:
        print(json.dumps(line))


if __name__ == "__main__":
    main()
