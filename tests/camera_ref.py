"""A float64 restatement of the camera ray: initRay with its anti-aliasing jitter and the depth-of-field lens.

Derived from the reference's OpenCL sources, not from the oracle or the kernels:

  source/opencl/pathtracing.cl  initRay (25-48)
  source/opencl/pt_utils.cl     rand (39-44), jitter (306-318), antiAliasing (327-337), depthOfField (349-373)
  source/opencl/pt_header.cl    PI_X2 (17)

Item layout: pbr_diag_camera_ray / orc_camera_ray, n x 8 {px, py, seed, tFocus, tObject, pad[3]} in, n x 8 {origin, dir,
seed after, 0} out.  The machinery is shading_ref's (`_Ev`, `Analysis`, `check`): every statement is a rounding point —
the pixel term of initRay term by term, as C evaluates it from the left: it cancels heavily in the middle of a wide image
—, and the random draws are inputs taken from the arithmetic under test: two for the jitter, two more with the lens.

Every branch of this stage is a decision on inputs alone (tFocus >= 0, tObject >= 0, == INFINITY, tObject > 0) and
therefore exact.  The quirks are kept: INFINITY is mapped to 1000 for both focus inputs, the lens runs only for
tObject > 0 (tFocus = 0 with tObject > 0 focuses on the eye itself), and the focal point is taken from the eye, not from
the moved origin.

The camera and the configuration are per batch, like a material: a tuple (CAM_KEYS index it)
  eye[3], w[3], u[3], v[3], lense focal, lense aperture, pxDim, anti-aliasing, width, height
"""
import numpy as np

import shading_ref as sr

EYE, CW, CU, CV, FOCAL, APERTURE, PXDIM, AA, WIDTH, HEIGHT = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), 12, 13, 14, 15, 16, 17
CAM_KEYS = tuple(range(16))            # what the sensitivity moves by an ulp: everything but the (integer) image size


def camera_tuple(eye, w, u, v, lense, px_dim, anti_aliasing, width, height):
    vals = [*eye, *w, *u, *v, *lense, px_dim, anti_aliasing]
    return tuple(float(np.float32(x)) for x in vals) + (float(width), float(height))


def camera_ray(px, py):
    """The stage for the pixels (px, py), whole numbers (n,): fn( ev, cam, x ) with x = {tFocus, tObject (n,), draws
    (n, 4)} -> {val: (n, 6) {origin, dir}, used: draws taken (2, or 4 with the lens), add: 0}."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)

    def fn(ev, cam, x):
        row = lambda s: np.broadcast_to(np.asarray(cam[s], np.float64), (ev.n, 3))
        eye, cw, cu, cv = row(EYE), row(CW), row(CU), row(CV)
        px_dim, aa, W, H = cam[PXDIM], cam[AA], cam[WIDTH], cam[HEIGHT]
        tF, tO, draws = x["tFocus"], x["tObject"], x["draws"]
        fx, fy = (2.0 * px)[:, None], (2.0 * py)[:, None]                    # 2.0f * pos.x: exact
        with np.errstate(invalid="ignore", over="ignore"):
            # pathtracing.cl:30-33: cam.u - W cam.u + 2 x cam.u + cam.v - H cam.v + 2 y cam.v, from the left
            inner = ev.r(cu - ev.r(W * cu))
            inner = ev.r(inner + ev.r(fx * cu))
            inner = ev.r(inner + cv)
            inner = ev.r(inner - ev.r(H * cv))
            inner = ev.r(inner + ev.r(fy * cv))
            initial = ev.r(cw + ev.r((px_dim * 0.5) * inner))                # pxDim * 0.5f: exact
            d = sr._normalize(ev, initial)
            # antiAliasing, pt_utils.cl:327-337
            rnd = draws[:, 0]
            phi = ev.r(sr.PI_X2 * draws[:, 1])
            aa_dir = sr._jitter(ev, d, phi, ev.r(sr._sqrt(rnd)), ev.r(sr._sqrt(ev.r(1.0 - rnd))))
            d = sr._normalize(ev, ev.r(d + ev.r(ev.r(aa_dir * px_dim) * aa)))
            # pathtracing.cl:43 and depthOfField, pt_utils.cl:349-373: decisions on inputs
            on = ev.decide("C.dof", (tF >= 0.0) & (tO >= 0.0))
            tO = np.where(ev.decide("C.objInf", np.isposinf(tO)), 1000.0, tO)
            tF = np.where(ev.decide("C.focInf", np.isposinf(tF)), 1000.0, tF)
            lens = on & ev.decide("C.obj", tO > 0.0)
            aperture = ev.r(cam[FOCAL] / cam[APERTURE])
            radius = ev.r(ev.r(draws[:, 2] * aperture) * 0.5)
            angle = ev.r(sr.PI_X2 * draws[:, 3])
            lx = ev.r(radius * ev.r(np.cos(angle)))
            ly = ev.r(radius * ev.r(np.sin(angle)))
            o = ev.r(ev.r(eye + ev.r(lx[:, None] * cu)) + ev.r(ly[:, None] * cv))
            focal_point = ev.r(np.where(lens, tF, 0.0)[:, None] * d + eye)   # fma: one rounding
            d_lens = sr._normalize(ev, ev.r(focal_point - o))
        val = np.concatenate([sr._sel(lens, o, eye), sr._sel(lens, d_lens, d)], axis=1)
        return {"val": val, "used": np.where(lens, 4, 2), "add": np.zeros(ev.n, bool)}

    fn.dir_cols = (3, 4, 5)
    return fn


def inputs(items, draws):
    r = items.astype(np.float64)
    return {"tFocus": r[:, 3], "tObject": r[:, 4], "draws": draws.astype(np.float64)}


def check(cam, items, got, draws, seq, K, flush=False):
    """Judge got (n x 8, the hook's output) for the items under the camera tuple `cam`; draws (n, 4) and seq (n, 5) from
    the arithmetic under test (shading_ref.seed_sequence).  See shading_ref.check."""
    fn = camera_ray(items[:, 0], items[:, 1])
    return sr.check(fn, cam, inputs(items, draws), got, K, CAM_KEYS, seeds=seq, flush=flush)
