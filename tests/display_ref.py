"""pbr_display (include/pbr_hip.h) restated in numpy, step by step: luminance and bin, the target and the adaptation in
float64, the map per channel in float32, the encode.  The sRGB thresholds are recomputed here from the formula — this is not
a copy of the constants of csrc/pt_display_host.hpp.

numpy's float32 array arithmetic rounds every operation to binary32 and fuses nothing; np.fmax / np.fmin return the other
operand when one is NaN, as fmaxf / fminf do.  The sign of a zero that fmaxf( -0, 0 ) returns is the one thing the C standard
leaves open: comparisons of mapped values are therefore by value (-0 == +0), and no byte of an image depends on it."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
MANUAL, AUTO = 0, 1
CLAMP, REINHARD, ACES = 0, 1, 2
LINEAR, SRGB = 0, 1


def srgb_inverse(c):
    """The inverse sRGB OETF in float64."""
    c = np.asarray(c, np.float64)
    return np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)


def srgb_oetf(x):
    """The sRGB OETF in float64 (the table's test: which code a threshold rounds to)."""
    x = np.asarray(x, np.float64)
    return np.where(x > 0.0031308, 1.055 * x ** (1.0 / 2.4) - 0.055, 12.92 * x)


def srgb_table():
    """(256,) float32: word k = 1 .. 255 is the smallest binary32 not below the inverse OETF of ( k - 0.5 ) / 255; word 0 is 0."""
    x = srgb_inverse((np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0)
    t = x.astype(F32)
    low = t.astype(np.float64) < x
    t[low] = np.nextafter(t[low], F32(np.inf))
    return np.concatenate([np.zeros(1, F32), t])


TABLE = srgb_table()


def luminance(rgb):
    c = np.fmin(np.fmax(np.asarray(rgb, F32), F32(0)), FLT_MAX)
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def slots(rgb):
    """Per pixel the bin 0 .. 255, or 256 for Y == 0."""
    with np.errstate(over="ignore"):
        Y = np.ascontiguousarray(luminance(rgb))
    bins = np.clip((Y.view(np.uint32) >> 20).astype(np.int64) - 888, 0, 255)
    return np.where(Y == 0, 256, bins)


def histogram(rgb):
    """(counts (256,) uint32, counted, dark)."""
    n = np.bincount(slots(rgb).reshape(-1), minlength=257)
    return n[:256].astype(np.uint32), int(n[:256].sum()), int(n[256])


def target(counts, low_fraction, high_fraction, min_log2, max_log2, previous=None):
    """Step 3 in float64, sums in ascending bin order; `previous` is the remembered log2 or None."""
    counts = [int(c) for c in counts]
    total = sum(counts)
    if total == 0:
        return 0.0 if previous is None else float(previous)
    N = float(total)
    lo = float(F32(low_fraction)) * N
    hi = N - float(F32(high_fraction)) * N
    below = weighted = kept = 0.0
    for b, n in enumerate(counts):
        up_to = below + float(n)
        share = max(0.0, min(up_to, hi) - max(below, lo))
        weighted = weighted + share * ((b + 0.5) / 8.0 - 16.0)
        kept = kept + share
        below = up_to
    m = weighted / kept
    return min(max(m, float(F32(min_log2))), float(F32(max_log2)))


def adapt(log2_target, adapt_share, previous=None):
    if previous is None or F32(adapt_share) == F32(1):
        return log2_target
    return previous + float(F32(adapt_share)) * (log2_target - previous)


def exposure_of(key, log2_used):
    return F32(float(F32(key)) * 2.0 ** (-log2_used))


def map_channel(c, exposure, curve, white=1.0):
    c, exposure, white = np.asarray(c, F32), F32(exposure), F32(white)
    with np.errstate(all="ignore"):
        x = np.fmin(np.fmax(c * exposure, F32(0)), F32(65504.0))
        if curve == REINHARD:
            y = (x * (F32(1) + x / (white * white))) / (F32(1) + x)
        elif curve == ACES:
            y = (x * (F32(2.51) * x + F32(0.03))) / (x * (F32(2.43) * x + F32(0.59)) + F32(0.14))
        else:
            y = x
        return np.fmin(np.fmax(y, F32(0)), F32(1))


def encode(y, transfer):
    y = np.asarray(y, F32)
    if transfer == SRGB:
        return np.searchsorted(TABLE[1:], y, side="right").astype(np.uint8)     # how many thresholds are <= y
    return np.floor(y * F32(255.0) + F32(0.5)).astype(np.uint8)


def image(rgba, exposure, curve, transfer, white=1.0, top_row_first=False):
    """(H, W, 4) uint8 from an (H, W, 4) float32 image with row 0 at the bottom."""
    rgba = np.asarray(rgba, F32)
    out = np.empty(rgba.shape[:2] + (4,), np.uint8)
    out[..., :3] = encode(map_channel(rgba[..., :3], exposure, curve, white), transfer)
    out[..., 3] = 255
    return out[::-1] if top_row_first else out
