"""pbr_update_vertices under a ray-ordered walk (pbr_refit_ordered_walk) timed on one GPU against the three-call sequence it
replaces, one scene and one layout per process.

  python scripts/relink_measure.py --scene sponza|dragon|hairball --layout 2|3 [--reps 5] [--frames 16] [--out FILE]
  python scripts/relink_measure.py --all [--limit 600] [...]     every scene x layout, each in a child process of its own under
                                                                 `timeout`; the first one that fails ends the run

The BASELINE scenes as bench.py generates them (Sponza-class 260k, Dragon-class 870k, hairball 2M triangles), 1920 x 1080, the
vertices moved with tests/refit_ref.py's seeded deformation at its large amplitude.  Reported, medians over --reps with the
spread (min .. max), wall times around the synchronous calls:
  (a) the re-linked update: device time of its kernels (pbr_last_kernel_ms), the re-link's share of it (pbr_diag_relink_info) and
      the wall time of the call; the first call, which builds the tables, is timed apart
  (b) the three-call sequence on the same library — pbr_configure( traversal 0 ), pbr_update_vertices, pbr_configure( layout ):
      wall time; and the ratio (b) / (a) of the wall medians
  (c) the re-link's device time against its traffic floor: 24 B read and streams x 32 B (compact: 64 B) written per node, plus
      the working tables the design writes and reads back once (pbr_diag_relink_info's bytes, twice) — bytes, GB/s, the fraction
      of 8 TB/s
  (d) Msamples/s of pbr_render( --frames ) on the re-linked streams against the host-built ones, the same pinned plan: the bytes
      are equal (checked here), so the gap is the noise figure
Append the output to profiles/r13/experiments/relink.txt."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

W, H = 1920, 1080
SCENES = {"dragon": ("dragon", 1, 870000), "sponza": ("sponza", 2, 260000), "hairball": ("hairball", 3, 2000000)}
LAYOUTS = (2, 3)
STREAMS = {1: 6, 2: 8, 3: 1}
RECORD_BYTES = {1: 32, 2: 32, 3: 64}
HBM_BYTES_PER_S = 8.0e12


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(values):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(values)), min(values), max(values))


def wall(call):
    start = time.perf_counter()
    call()
    return (time.perf_counter() - start) * 1e3


def every_case():
    limit = arg("--limit", "600")
    passed = [a for a in sys.argv[1:] if a != "--all"]
    for name in SCENES:
        for layout in LAYOUTS:
            done = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--scene", name, "--layout", str(layout)] + passed)
            if done.returncode != 0:
                sys.exit("relink_measure: %s, layout %d ended with status %d; nothing more is started" % (name, layout, done.returncode))


def main():
    import pbr_loader
    import refit_ref
    pbr = pbr_loader.load()
    name, layout = arg("--scene", "sponza"), int(arg("--layout", "2"))
    reps, frames = int(arg("--reps", "5")), int(arg("--frames", "16"))
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = sc.arrays()
    plain, cam, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    ordered = pbr.Config.from_buffer_copy(plain)
    ordered.traversal = layout
    seeds = pbr.frame_seeds(0, frames)
    nodes = a["bvh"].shape[0]
    v = refit_ref.deform(a["facesV"], a["vertices"], "large", seed=3)
    lines = ["== %s, layout %d: %d faces, %d vertices, %d nodes, %d x %d" % (name, layout, a["facesV"].shape[0], a["vertices"].shape[0], nodes, W, H)]

    dev = pbr.Device(0)
    dev.upload_scene(sc.desc)
    dev.configure(ordered)
    dev.render(0, pbr.frame_seeds(0, max(frames, dev.tune_budget())), px, cam)
    plan = dev.last_plan()[1]
    plan = plan if plan >= 0 else 4
    dev.pin_plan(plan)
    dev.refit_ordered_walk(True)
    first = wall(lambda: dev.update_vertices(a["vertices"]))
    info = dev.relink_info()
    lines.append("tables: %d bytes (%.1f per node), %d levels, %d launches; the first re-linked update, which builds them: wall %.3f ms"
                 % (info["table_bytes"], info["table_bytes"] / nodes, info["levels"], info["launches"], first))
    device_ms, relink_ms, wall_a = [], [], []
    for _ in range(reps):
        dev.update_vertices(a["vertices"])
        wall_a.append(wall(lambda: dev.update_vertices(v)))
        device_ms.append(dev.last_kernel_ms())
        relink_ms.append(dev.relink_info()["ms"])
    lines.append("(a) re-linked update: device %s ms, of which the re-link %s ms | wall %s ms" % (spread(device_ms), spread(relink_ms), spread(wall_a)))
    floor = 24 * nodes + STREAMS[layout] * RECORD_BYTES[layout] * nodes + 2 * info["table_bytes"]
    rate = floor / (float(np.median(relink_ms)) * 1e-3)
    lines.append("(c) traffic floor %d bytes -> %.1f GB/s = %.1f %% of 8 TB/s" % (floor, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S))

    other = pbr.Device(0)
    other.upload_scene(sc.desc)
    other.configure(ordered)
    other.pin_plan(plan)

    def three_calls(vertices):
        other.configure(plain)
        other.update_vertices(vertices)
        other.configure(ordered)

    wall_b = []
    for _ in range(reps):
        three_calls(a["vertices"])
        wall_b.append(wall(lambda: three_calls(v)))
    lines.append("(b) configure( 0 ), update, configure( %d ): wall %s ms" % (layout, spread(wall_b)))
    ratios = [b / a_ for a_, b in zip(wall_a, wall_b)]
    lines.append("(b) / (a), wall: %.1f by the medians; %s over the paired repetitions" % (float(np.median(wall_b)) / float(np.median(wall_a)), spread(ratios)))
    same = np.array_equal(dev.read_walk()[0], other.read_walk()[0])
    lines.append("the two contexts' streams are %s" % ("equal in every byte" if same else "DIFFERENT"))

    other.pin_plan(plan)
    samples = W * H * frames * plain.samples / 1e6
    rates = {}
    for what, d in (("re-linked", dev), ("host-built", other)):
        d.reset_accum()
        d.render(0, seeds, px, cam)
        rates[what] = [samples / (wall(lambda: d.render(0, seeds, px, cam)) * 1e-3) for _ in range(reps)]
    lines.append("(d) render( %d ) plan %d: re-linked streams %s Msamples/s | host-built streams %s Msamples/s (wall)" % (frames, plan, spread(rates["re-linked"]), spread(rates["host-built"])))
    other.close()
    dev.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(text)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    every_case() if "--all" in sys.argv else main()
