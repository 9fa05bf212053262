"""pbr_denoise_temporal with per-vertex motion (pbr_temporal_track_motion) on one GPU: device time of the static and of the
motion path, and image quality with a moving object, for one scene per process.

  python scripts/temporal_motion_measure.py --scene cornell|sponza [--reps 7] [--long 512] [--static-only] [--out FILE]

The BASELINE scenes as bench.py generates them (the Cornell box; Sponza-class, 260k triangles), 1920 x 1080, render.max_depth 4,
static camera.  A displayed frame = (an update of the vertices) + reset_accum + one uniform adaptive round of 4 frames + one
pbr_denoise_temporal.  What moves: on the Cornell box the tall block (the vertices of its material's faces); on the
Sponza-class scene the 5 % of the vertices nearest to the median vertex — by 0.2 % of the scene's extent along x per frame.
  (a) device time (pbr_last_kernel_ms: untile, variance, feature pass, [motion,] integrate, five filter passes), medians over
      --reps with the spread (min .. max): the static path (tracking on, nothing moves) and the motion path (an update before
      every frame).  --static-only measures the static path alone and needs neither of the new entry points: with
      PBR_LAB_ENV=1 PBR_HIP_LIB=<a build of the parent commit> it is the yardstick for "the static path is unchanged".
  (b) the motion path's extra traffic against its floor — per pixel: face plane 4 B written + 4 read, motion and reference
      planes 32 written + 32 read, and at most 112 B gathered (facesV 16 + six vertices 96; lanes on one face share them)
  (c) MSE against pbr_render( 0, frame_seeds( 1000, --long ) ) of the final geometry, rgb over the pixels finite in all images:
      pbr_denoise_temporal after 4 displayed frames with the object moving before frames 2 - 4, tracked and untracked (the
      untracked history is dropped by every update: the guided filter on 4 frames), and pbr_denoise_guided on 16 frames
Append the output of the two scenes to profiles/r12/experiments/temporal_motion.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import pbr_loader  # noqa: E402

W, H = 1920, 1080
SCENES = {"cornell": ("cornell", 1, 0), "sponza": ("sponza", 2, 260000)}
FRAMES, CALLS = 4, 4
FLOOR_PLANES, FLOOR_GATHER = 4 + 4 + 32 + 32, 112


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(values):
    return "%7.3f (%.3f .. %.3f)" % (float(np.median(values)), min(values), max(values))


def moving_vertices(name, arrays):
    faces, vertices = arrays["facesV"], arrays["vertices"]
    mask = np.zeros(len(vertices), bool)
    if name == "cornell":
        top = {int(m): float(vertices[faces[faces[:, 3] == m][:, :3].ravel(), 1].max()) for m in np.unique(faces[:, 3])}
        material = [m for m, y in top.items() if y == float(np.float32(1.2))][0]
        mask[faces[faces[:, 3] == material][:, :3].ravel()] = True
    else:
        d = np.linalg.norm(vertices[:, :3] - np.median(vertices[:, :3], axis=0), axis=1)
        mask[np.argsort(d)[:len(vertices) // 20]] = True
    return mask


def main():
    pbr = pbr_loader.load()
    name, reps, long_frames = arg("--scene", "sponza"), int(arg("--reps", "7")), int(arg("--long", "512"))
    static_only = "--static-only" in sys.argv
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    cfg, cam, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    arrays = sc.arrays()
    mask = moving_vertices(name, arrays)
    extent = float((arrays["vertices"][:, :3].max(0) - arrays["vertices"][:, :3].min(0)).max())
    delta = np.array([-0.002 * extent, 0, 0], np.float32)
    lines = ["== %s: %d triangles, %d x %d, BRDF %d, max_depth %d; library %s; %d of %d vertices move (%.1f %%) by %.4g per frame"
             % (name, len(arrays["facesV"]), W, H, cfg.brdf, cfg.max_depth, os.environ.get("PBR_HIP_LIB", "product"), mask.sum(), mask.size,
                100.0 * mask.mean(), float(-delta[0]))]

    dev = pbr.Device(0)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)
    seeds = iter(range(0, 100000, 100))

    def render(frames=FRAMES):
        dev.reset_accum()
        dev.render_adaptive(0, pbr.frame_seeds(next(seeds), frames), px, cam, frames, frames, frames, 0.0)

    def moved(steps):
        v = arrays["vertices"].copy()
        v[mask, :3] += delta * np.float32(steps)
        return v

    # (a) device time
    if not static_only:
        dev.temporal_track_motion(True)
    paths = (("static path", False),) if static_only else (("static path", False), ("motion path", True))
    times = {}
    for label, moving in paths:
        dev.temporal_reset()
        ms, lengths, codes = [], None, None
        for k in range(reps + 2):                      # the first call allocates and has no history, the second warms up
            if moving:
                dev.update_vertices(moved(k))
            render()
            out, hist = dev.denoise_temporal(px, cam, history=True)
            ms.append(dev.last_kernel_ms())
            lengths = hist[..., 2]
            if moving and k > 0:
                codes = dev.temporal_motion()[0][..., 3]
        times[label] = ms[2:]
        more = "" if codes is None else " | pixels on moved faces %.3f" % float((codes >= 2).mean())
        lines.append("(a) %s: denoise_temporal %s ms (device, median of %d) | pixels that continued %.3f, mean L %.2f%s"
                     % (label, spread(ms[2:]), reps, float((lengths > 1).mean()), float(lengths.mean()), more))

    if not static_only:
        extra = float(np.median(times["motion path"]) - np.median(times["static path"])) * 1e-3
        for what, per_pixel in (("planes only", FLOOR_PLANES), ("planes + gathers", FLOOR_PLANES + FLOOR_GATHER)):
            gb = per_pixel * W * H / 1e9
            lines.append("(b) extra traffic floor, %s: %d B per pixel = %.3f GB; the motion path adds %.4f ms: %s"
                         % (what, per_pixel, gb, extra * 1e3, "%.2f TB/s" % (gb / extra / 1e3) if extra > 0 else "no measurable addition"))

        # (c) quality after 4 displayed frames with the object moving
        dev.update_vertices(moved(CALLS - 1))
        dev.reset_accum()
        dev.render(0, pbr.frame_seeds(1000, long_frames), px, cam)
        converged = dev.read_output()[..., :3]
        images = {}
        for label, tracked in (("temporal 4 x 4 frames, tracked", True), ("temporal 4 x 4 frames, untracked", False)):
            dev.temporal_track_motion(tracked)
            dev.update_vertices(moved(0))
            dev.temporal_reset()
            for k in range(CALLS):
                if k > 0:
                    dev.update_vertices(moved(k))
                render()
                out, hist = dev.denoise_temporal(px, cam, history=True)
            images[label] = out[..., :3]
            lines.append("    %s: mean L %.2f" % (label, float(hist[..., 2].mean())))
        images["guided 4 frames"] = dev.denoise_guided(px, cam)[..., :3]
        images["unfiltered 4 frames"] = dev.read_output()[..., :3]
        render(FRAMES * CALLS)
        images["guided 16 frames"] = dev.denoise_guided(px, cam)[..., :3]
        ok = np.isfinite(converged).all(-1)
        for image in images.values():
            ok &= np.isfinite(image).all(-1)
        lines.append("(c) MSE over %d of %d pixels: %s" % (int(ok.sum()), ok.size,
                     " | ".join("%s %.4g" % (k, float(((v - converged)[ok] ** 2).mean())) for k, v in images.items())))
    dev.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
