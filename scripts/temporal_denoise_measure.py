"""pbr_denoise_temporal against pbr_denoise_guided on one GPU: device time and image quality, for one scene per process.

  python scripts/temporal_denoise_measure.py --scene cornell|sponza [--reps 7] [--long 512] [--out FILE]

The BASELINE scenes as bench.py generates them (the Cornell box; Sponza-class, 260k triangles), 1920 x 1080, render.max_depth 4.
A displayed frame = reset_accum + one uniform adaptive round of 4 frames (min = max = 4, threshold 0) with seeds of its own +
one filter call.
  (a) device time (pbr_last_kernel_ms), medians over --reps with the spread (min .. max), same process, same renders:
      pbr_denoise_temporal (untile, variance, feature pass, integrate, five filter passes) with a history under a static
      camera and under a camera that moves every frame, and pbr_denoise_guided (the same without integrate) on the same render
  (b) MSE against pbr_render( 0, frame_seeds( 1000, --long ) ) under the LAST camera, rgb over the pixels that are finite in all
      images: pbr_denoise_temporal after 4 displayed frames (4 x 4 frames) with a static camera and with a camera that moved
      before every one of them (sideways, 1 % of the median first-hit distance per frame, with a turn of 0.005), against
      pbr_denoise_guided on 4 frames and on 16 frames under that camera
Append the output of the two scenes to profiles/r11/experiments/temporal_denoise.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import pbr_loader  # noqa: E402

W, H = 1920, 1080
SCENES = {"cornell": ("cornell", 1, 0), "sponza": ("sponza", 2, 260000)}
FRAMES, CALLS = 4, 4


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(values):
    return "%7.3f (%.3f .. %.3f)" % (float(np.median(values)), min(values), max(values))


def main():
    pbr = pbr_loader.load()
    name, reps, long_frames = arg("--scene", "sponza"), int(arg("--reps", "7")), int(arg("--long", "512"))
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    cfg, base, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    lines = ["== %s: %d triangles, %d x %d, BRDF %d, max_depth %d; reference: %d frames" % (name, triangles, W, H, cfg.brdf, cfg.max_depth, long_frames)]

    dev = pbr.Device(0)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)

    eye, u, w = (np.array([getattr(base, k).x, getattr(base, k).y, getattr(base, k).z], np.float64) for k in ("eye", "u", "w"))

    def view(steps, stride):
        e = (eye + steps * stride * u).astype(np.float32)
        c = (e + w + steps * 0.005 * u).astype(np.float32)
        cam = pbr.Camera()
        pbr.host.pbrh_camera_lookat(e.ctypes.data_as(pbr._fp), c.ctypes.data_as(pbr._fp), cam)
        return cam

    seeds = iter(range(0, 100000, 100))

    def render(cam, frames=FRAMES):
        dev.reset_accum()
        dev.render_adaptive(0, pbr.frame_seeds(next(seeds), frames), px, cam, frames, frames, frames, 0.0)

    render(base)
    distance = dev.denoise(px, base, features=True)[1][0][..., 3]
    stride = 0.01 * float(np.median(distance[np.isfinite(distance)]))
    lines.append("    median first-hit distance %.4g: the moving camera goes %.4g sideways per displayed frame" % (stride * 100, stride))

    # (a) device time
    for label, moving in (("static camera", False), ("moving camera", True)):
        dev.temporal_reset()
        temporal_ms, guided_ms, lengths = [], [], None
        for k in range(reps + 2):                      # the first call allocates and has no history, the second warms up
            cam = view(k if moving else 0, stride)
            render(cam)
            out, hist = dev.denoise_temporal(px, cam, history=True)
            temporal_ms.append(dev.last_kernel_ms())
            dev.denoise_guided(px, cam)
            guided_ms.append(dev.last_kernel_ms())
            lengths = hist[..., 2]
        lines.append("(a) %s: denoise_temporal %s ms | denoise_guided %s ms (device, median of %d) | pixels that continued %.3f, mean L %.2f"
                     % (label, spread(temporal_ms[2:]), spread(guided_ms[2:]), reps, float((lengths > 1).mean()), float(lengths.mean())))

    # (b) quality after 4 displayed frames
    for label, moving in (("static camera", False), ("moving camera", True)):
        last = view(CALLS - 1 if moving else 0, stride)
        dev.reset_accum()
        dev.render(0, pbr.frame_seeds(1000, long_frames), px, last)
        converged = dev.read_output()[..., :3]
        dev.temporal_reset()
        for k in range(CALLS):
            cam = view(k if moving else 0, stride)
            render(cam)
            temporal, hist = dev.denoise_temporal(px, cam, history=True)
        guided4 = dev.denoise_guided(px, last)
        noisy4 = dev.read_output()[..., :3]
        render(last, FRAMES * CALLS)
        guided16 = dev.denoise_guided(px, last)
        images = {"unfiltered 4 frames": noisy4, "guided 4 frames": guided4[..., :3], "temporal 4 x 4 frames": temporal[..., :3],
                  "guided 16 frames": guided16[..., :3]}
        ok = np.isfinite(converged).all(-1)
        for image in images.values():
            ok &= np.isfinite(image).all(-1)
        lines.append("(b) %s: MSE over %d of %d pixels: %s | mean L %.2f"
                     % (label, int(ok.sum()), ok.size, " | ".join("%s %.4g" % (k, float(((v - converged)[ok] ** 2).mean())) for k, v in images.items()),
                        float(hist[..., 2].mean())))
    dev.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
