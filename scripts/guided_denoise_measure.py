"""pbr_denoise_guided against pbr_denoise on one GPU: device time and image quality, for one scene per process.

  python scripts/guided_denoise_measure.py --scene cornell|sponza [--reps 7] [--long 512] [--out FILE]

The BASELINE scenes as bench.py generates them (the Cornell box; Sponza-class, 260k triangles), 1920 x 1080, render.max_depth 4.
Per sample count n in 4, 16, 64 — one uniform adaptive round (min = max = n, threshold 0), so that the variance is there and
the image is pbr_render( n )'s:
  (a) device time (pbr_last_kernel_ms: untile, variance, feature pass, five filter passes), medians over --reps with the
      spread (min .. max), of pbr_denoise_guided at its defaults and of pbr_denoise at its defaults, same build, same image;
      pbr_read_variance on its own
  (b) MSE against pbr_render( 0, frame_seeds( 1000, --long ) ), rgb over the pixels that are finite in all images: unfiltered,
      pbr_denoise at sigma_color 1.2 (its default) and at the value the harness docstring recommends for n (1.2 / 0.6 / 0.3),
      pbr_denoise_guided at sigma_luminance 4 (its default)
Append the output of the two scenes to profiles/r10/experiments/guided_denoise.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import pbr_loader  # noqa: E402

W, H = 1920, 1080
SCENES = {"cornell": ("cornell", 1, 0), "sponza": ("sponza", 2, 260000)}
TUNED_SIGMA_COLOR = {4: 1.2, 16: 0.6, 64: 0.3}


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
    cfg, cam, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    lines = ["== %s: %d triangles, %d x %d, BRDF %d, max_depth %d; reference: %d frames" % (name, triangles, W, H, cfg.brdf, cfg.max_depth, long_frames)]

    dev = pbr.Device(0)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)
    dev.render(0, pbr.frame_seeds(1000, long_frames), px, cam)
    converged = dev.read_output()[..., :3]

    def timed(call):
        ms = []
        for _ in range(reps + 1):
            out = call()
            ms.append(dev.last_kernel_ms())
        return out, ms[1:]                 # the first call warms the allocator up

    for n in sorted(TUNED_SIGMA_COLOR):
        dev.reset_accum()
        dev.render_adaptive(0, pbr.frame_seeds(0, n), px, cam, n, n, n, 0.0)
        noisy = dev.read_output()[..., :3]
        variance, variance_ms = timed(dev.read_variance)
        guided, guided_ms = timed(lambda: dev.denoise_guided(px, cam))
        plain, plain_ms = timed(lambda: dev.denoise(px, cam))
        tuned = dev.denoise(px, cam, pbr.DenoiseParams(sigma_color=TUNED_SIGMA_COLOR[n]))
        images = {"unfiltered": noisy, "denoise sigma_color 1.2": plain[..., :3],
                  "denoise sigma_color %.1f" % TUNED_SIGMA_COLOR[n]: tuned[..., :3], "guided sigma_luminance 4": guided[..., :3]}
        ok = np.isfinite(converged).all(-1)
        for image in images.values():
            ok &= np.isfinite(image).all(-1)
        lines.append("(a) %2d frames: denoise_guided %s ms | denoise %s ms | read_variance %s ms (device, median of %d)"
                     % (n, spread(guided_ms), spread(plain_ms), spread(variance_ms), reps))
        lines.append("(b) %2d frames: MSE over %d of %d pixels: %s | mean variance %.4g"
                     % (n, int(ok.sum()), ok.size, " | ".join("%s %.4g" % (k, float(((v - converged)[ok] ** 2).mean())) for k, v in images.items()),
                        float(variance[np.isfinite(variance)].mean())))
    dev.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
