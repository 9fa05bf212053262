"""Depth of field over many frames, timed on one GPU: the per-frame sequence against pbr_render_dof, and pbr_render
without a focus point as the control.

  python scripts/dof_render.py [--what perframe,dof,plain] [--scenes sponza,cornell] [--reps 5] [--layout 0|1]

Sponza-class (64 frames) and Cornell box (256 frames) as BASELINE.json has them, 1920 x 1080, focus point at the image
centre.  Each measurement: a warm-up that lets the schedule tuner settle (pbr_diag_tune_budget frames) and renders the
timed shape once, then --reps repetitions of the same render from a reset accumulation.  Printed per repetition: wall
time around the (synchronous) calls and the device time the library reports (pbr_last_kernel_ms, summed over the calls);
for pbr_render_dof also the focus chain's share (pbr_diag_last_focus_chain).  One JSON line per measurement at the end.

  perframe   n x { render_frame ; accumulate } — what a caller with a focus point had to do before pbr_render_dof
  dof        render_dof( n frames )
  plain      render( n frames ), focus point off — must not move between two builds of the library

To time another build of the library (the parent commit's, for the yardstick), start the script with PBR_LAB_ENV=1 and
PBR_HIP_LIB=<that libpbrhip.so>; a library without pbr_render_dof skips `dof`.  Run the builds in alternation, each in a
process of its own, and compare only differences larger than the spread of the repetitions."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pbr_loader  # noqa: E402

W, H = 1920, 1080
SCENES = {"sponza": ("sponza", 2, 260000, 3, 64), "cornell": ("cornell", 1, 0, 8, 256)}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    pbr = pbr_loader.load()
    what = arg("--what", "perframe,dof,plain").split(",")
    reps = int(arg("--reps", "5"))
    layout = int(arg("--layout", "-1"))
    label = arg("--label", os.environ.get("PBR_HIP_LIB", "product"))
    lines = []
    for name in arg("--scenes", "sponza,cornell").split(","):
        kind, seed, tris, depth, frames = SCENES[name]
        pbr.cfg_reset()
        pbr.cfg_set(**{"render.max_depth": depth})
        sc = pbr.HostScene.generate(kind, seed, tris)
        cfg, px, seeds = sc.config(W, H), pbr.pixel_dimension(W, H), pbr.frame_seeds(0, frames)
        plain = sc.camera()
        cam = pbr.Camera.from_buffer_copy(plain)
        cam.focusPoint[0], cam.focusPoint[1] = W // 2, H // 2
        for mode in what:
            if mode == "dof" and not hasattr(pbr.hip, "pbr_render_dof"):
                continue
            dev = pbr.Device(0)
            dev.upload_scene(sc.desc)
            dev.configure(cfg)
            if layout >= 0 and mode == "dof":
                dev.set_knob("chain_layout", layout)

            def once():
                """(wall ms, device ms, focus chain ms) of one render of `frames` frames from a reset accumulation"""
                dev.reset_accum()
                device_ms, chain_ms = 0.0, 0.0
                t0 = time.perf_counter()
                if mode == "perframe":
                    for k in range(frames):
                        dev.render_frame(float(seeds[k]), k / (k + 1.0), px, cam)
                        device_ms += dev.last_kernel_ms()
                        dev.accumulate()
                elif mode == "dof":
                    dev.render_dof(0, seeds, px, cam)
                    device_ms, chain_ms = dev.last_kernel_ms(), dev.last_focus_chain_ms()
                else:
                    dev.render(0, seeds, px, plain)
                    device_ms = dev.last_kernel_ms()
                return (time.perf_counter() - t0) * 1e3, device_ms, chain_ms

            # the tuner settles on launches of the shapes this mode renders anyway
            budget, done = dev.tune_budget(), 0
            while done < budget + frames:
                once()
                done += frames
            runs = [once() for _ in range(reps)]
            wall, device, chain = (np.array([r[i] for r in runs]) for i in range(3))
            line = {"scene": name, "mode": mode, "library": label, "frames": frames, "plan": dev.last_plan()[0], "layout": layout,
                    "wall_ms": [round(float(v), 3) for v in wall], "device_ms": [round(float(v), 3) for v in device],
                    "chain_ms": [round(float(v), 3) for v in chain],
                    "wall_ms_per_frame_median": round(float(np.median(wall)) / frames, 4),
                    "device_ms_per_frame_median": round(float(np.median(device)) / frames, 4),
                    "device_ms_spread": round(float(device.max() - device.min()), 3), "wall_ms_spread": round(float(wall.max() - wall.min()), 3)}
            lines.append(line)
            print("%-8s %-9s %-14s %3d frames  wall %8.3f ms (%.3f .. %.3f)  device %8.3f ms (%.3f .. %.3f)  chain %.3f ms  = %.4f ms/frame  [%s]" % (
                name, mode, os.path.basename(os.path.dirname(label)) or label, frames, np.median(wall), wall.min(), wall.max(),
                np.median(device), device.min(), device.max(), np.median(chain), np.median(device) / frames, line["plan"]), flush=True)
            dev.close()
    for line in lines:
        print(json.dumps(line))


if __name__ == "__main__":
    main()
