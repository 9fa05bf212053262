"""pbr_display on one GPU: device time of its two kernels against pbr_read_display's, and the wall time of an auto call.

  python scripts/display_measure.py [--parent DIR] [--reps 9] [--sizes 1920x1080,3840x2160] [--out FILE]

Per size, medians over --reps calls in one run with the spread (min .. max); the first call of each kind is not counted:
  (a) pbr_read_display's kernel (ptk::displayRGBA8).  The call keeps no device time, so a child process — this script with
      --child — makes the calls under `rocprofv3 --kernel-trace` and the kernel's dispatches are read from the trace: once in
      this tree and, with --parent, once in DIR, a checkout of the parent commit with its libraries built.
  (b) the map kernel (pbr_diag_display_info): { manual, exposure 1, clamp, linear } — pbr_read_display's bytes — and
      { manual, exposure 1, ACES, sRGB }, on the accumulated Cornell frame
  (c) the histogram kernel for each number of merge rounds (knob "display_merge": 0, 1, 2, 4): on the rendered Cornell frame, on a
      rendered Sponza-class frame (260k triangles), on a log-uniform image over 2^-20 .. 2^20 and on an all-equal image — the last two
      handed in as host images, the same kernel over a row-major buffer
  (d) the wall time of an auto call on the accumulated Cornell frame (histogram, read-back of the counts, map, read-back of the
      bytes), and of pbr_read_display
Append the output to profiles/<round>/experiments/display.txt."""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(values):
    import numpy as np
    return "%8.4f (%.4f .. %.4f)" % (float(np.median(values)), min(values), max(values))


def child(root, w, h, reps):
    """reps + 1 pbr_read_display calls on a rendered Cornell frame, with the package of `root`."""
    sys.path.insert(0, root)
    import pbr_loader
    pbr = pbr_loader.load()
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    sc = pbr.HostScene.generate("cornell", 1, 0)
    dev = pbr.Device(0)
    dev.upload_scene(sc.desc)
    dev.configure(sc.config(w, h))
    dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(w, h), sc.camera())
    for _ in range(reps + 1):
        dev.read_display()
    dev.close()


def traced_read_display(root, w, h, reps):
    """Durations in ms of displayRGBA8's dispatches but the first, from a kernel trace of a child process."""
    with tempfile.TemporaryDirectory() as out:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--child", root, str(w), str(h), str(reps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:
            raise RuntimeError("the traced child failed:\n" + done.stdout[-2000:])
        ms = []
        for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "displayRGBA8" in row["Kernel_Name"]:
                        ms.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    if len(ms) != reps + 1:
        raise RuntimeError("%d dispatches of displayRGBA8 in the trace, %d calls made" % (len(ms), reps + 1))
    return ms[1:]


def main():
    if "--child" in sys.argv:
        at = sys.argv.index("--child")
        return child(sys.argv[at + 1], int(sys.argv[at + 2]), int(sys.argv[at + 3]), int(sys.argv[at + 4]))
    sys.path.insert(0, ROOT)
    import numpy as np
    import pbr_loader
    pbr = pbr_loader.load()
    reps, parent = int(arg("--reps", "9")), arg("--parent", "")
    sizes = [tuple(int(v) for v in s.split("x")) for s in arg("--sizes", "1920x1080,3840x2160").split(",")]
    linear = pbr.DisplayParams(exposure_mode=0, exposure=1.0, curve=0, transfer=0)
    aces = pbr.DisplayParams(exposure_mode=0, exposure=1.0, curve=2, transfer=1)
    auto = pbr.DisplayParams()
    lines = []

    def say(text):
        lines.append(text)
        sys.stdout.write(text + "\n")
        sys.stdout.flush()

    def timed(dev, call, pick):
        values = []
        for _ in range(reps + 1):
            call()
            values.append(pick(dev))
        return values[1:]

    def wall(call):
        values = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            call()
            values.append((time.perf_counter() - t0) * 1e3)
        return values[1:]

    def histograms(dev, what, rgba=None):
        for rounds in (0, 1, 2, 4):
            dev.set_knob("display_merge", rounds)
            ms = timed(dev, lambda: dev.display(linear, rgba=rgba, info=True), lambda d: d.display_info()[0])
            say("(c) histogram, %d merge rounds, %-12s %s ms" % (rounds, what + ":", spread(ms)))
        dev.set_knob("display_merge", -1)

    for w, h in sizes:
        say("== %d x %d, medians of %d (min .. max), device time unless it says wall" % (w, h, reps))
        say("(a) displayRGBA8 (pbr_read_display), this tree:      %s ms" % spread(traced_read_display(ROOT, w, h, reps)))
        if parent:
            say("(a) displayRGBA8 (pbr_read_display), parent commit:  %s ms" % spread(traced_read_display(os.path.abspath(parent), w, h, reps)))
        else:
            say("(a) displayRGBA8 of the parent commit: not measured (no --parent)")
        pbr.cfg_reset()
        pbr.cfg_set(**{"render.max_depth": 4})
        px = pbr.pixel_dimension(w, h)
        rng = np.random.default_rng(1)
        log_uniform = np.exp2(rng.uniform(-20.0, 20.0, (h, w, 4))).astype(np.float32)
        equal = np.empty((h, w, 4), np.float32)
        equal[...] = (0.5, 0.4, 0.3, 1.0)
        for name, kind, seed, triangles in (("Cornell", "cornell", 1, 0), ("Sponza-class", "sponza", 2, 260000)):
            sc = pbr.HostScene.generate(kind, seed, triangles)
            dev = pbr.Device(0)
            dev.upload_scene(sc.desc)
            dev.configure(sc.config(w, h))
            dev.render(0, pbr.frame_seeds(0, 4), px, sc.camera())
            if kind == "cornell":
                say("(b) map, manual / clamp / linear:                    %s ms" % spread(timed(dev, lambda: dev.display(linear), lambda d: d.display_info()[1])))
                say("(b) map, manual / ACES / sRGB:                       %s ms" % spread(timed(dev, lambda: dev.display(aces), lambda d: d.display_info()[1])))
                assert np.array_equal(dev.display(linear), dev.read_display())
            histograms(dev, name)
            if kind == "cornell":
                histograms(dev, "log-uniform", log_uniform)
                histograms(dev, "all-equal", equal)
                say("(d) auto call, wall:                                 %s ms" % spread(wall(lambda: dev.display(auto))))
                say("(d) pbr_read_display, wall:                          %s ms" % spread(wall(dev.read_display)))
                _, info = dev.display(auto, info=True)
                say("    auto on the Cornell frame: log2 %.4f, exposure %.4f, %d counted, %d dark" % (info["log2_used"], info["exposure"], info["counted"], info["dark"]))
            dev.close()
    pbr.cfg_reset()
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
