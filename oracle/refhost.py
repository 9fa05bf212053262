"""The reference's own HOST code as a checker: its loaders (ObjParser, MtlParser, LightParser, ModelLoader), its BVH builder
and MathHelp::triCalcAABB, compiled UNMODIFIED from the reference's source tree together with this repository's driver
(oracle/refhost/dump.cpp) and stand-in headers (oracle/refhost/include/) into oracle/_ref/refhost_dump.

TEST INFRASTRUCTURE ONLY.  Nothing of the reference is copied into this repository: the recipe names its files where they
lie, and the binary lands in oracle/_ref/, which git ignores.  Where the reference's tree does not exist, build() returns
without error and leaves oracle/_ref/ as it is; the tests that run the dumper skip there, the tests that read the recorded
dumps (tests/golden/refhost_*.npz) run everywhere.

Flags: the GNU dialect (cl_float4 has .x .y .z only there), -include cfloat (BVH.cpp uses FLT_MAX without its header), no
-fopenmp (the build is deterministic), no -ffast-math, no -march, -ffp-contract=off: every operation rounds once.
"""
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_SOURCE = "/root/reference/source"
BINARY = os.path.join(_HERE, "_ref", "refhost_dump")
_OWN = os.path.join(_HERE, "refhost")
_REFERENCE_FILES = ("MathHelp.cpp", "accelstructures/BVH.cpp", "accelstructures/AccelStructure.cpp", "ObjParser.cpp", "MtlParser.cpp",
                    "LightParser.cpp", "ModelLoader.cpp", "Logger.cpp", "Cfg.cpp")
FLAGS = ("-O2", "-ffp-contract=off", "-std=gnu++11", "-include", "cfloat", "-DCL_TARGET_OPENCL_VERSION=120", "-w")


def _own_sources():
    out = [os.path.join(_OWN, "dump.cpp")]
    for base, _, files in os.walk(os.path.join(_OWN, "include")):
        out += [os.path.join(base, f) for f in files]
    return out


def available():
    return os.path.isdir(REFERENCE_SOURCE)


def build(force=False):
    """oracle/_ref/refhost_dump, or None where the reference's sources do not exist (nothing is touched then)."""
    if not available():
        return None
    sources = [os.path.join(REFERENCE_SOURCE, f) for f in _REFERENCE_FILES]
    newest = max(os.path.getmtime(s) for s in sources + _own_sources())
    if force or not os.path.exists(BINARY) or os.path.getmtime(BINARY) < newest:
        os.makedirs(os.path.dirname(BINARY), exist_ok=True)
        tmp = "%s.%d.tmp" % (BINARY, os.getpid())       # built aside and moved into place, as oracle.build does
        try:
            subprocess.check_call(["g++", *FLAGS, "-I", os.path.join(_OWN, "include"), "-I", REFERENCE_SOURCE,
                                   "-o", tmp, os.path.join(_OWN, "dump.cpp"), *sources])
            os.replace(tmp, BINARY)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return BINARY


_DTYPES = {b"f": np.float32, b"u": np.uint32, b"i": np.int32}


def read_dump(path):
    """dump.cpp's records as {name: array}; name lists come back as lists of str."""
    with open(path, "rb") as f:
        blob = f.read()
    out, at = {}, 0
    while at < len(blob):
        n = int(np.frombuffer(blob, "<u4", 1, at)[0]); at += 4
        name = blob[at:at + n].decode(); at += n
        kind = blob[at:at + 1]; at += 1
        nd = int(np.frombuffer(blob, "<u4", 1, at)[0]); at += 4
        dims = [int(d) for d in np.frombuffer(blob, "<u4", nd, at)]; at += 4 * nd
        if kind == b"s":
            text = blob[at:at + dims[0]].decode(); at += dims[0]
            out[name] = text.split("\n")[:-1]
        else:
            count = int(np.prod(dims))
            out[name] = np.frombuffer(blob, np.dtype(_DTYPES[kind]).newbyteorder("<"), count, at).reshape(dims).astype(_DTYPES[kind])
            at += 4 * count
    return out


def _run(args, out):
    subprocess.check_call([BINARY, *args, "out=" + out], stdout=subprocess.DEVNULL)
    try:
        return read_dump(out)
    finally:
        os.remove(out)


def dump_scene(directory, obj, scratch, **cfg):
    """Runs `refhost_dump scene`; cfg: the reference's dotted keys, e.g. {"render.phong_tessellation": 0.6}."""
    settings = ["%s=%s" % (k, str(v).lower() if isinstance(v, bool) else repr(float(v)) if isinstance(v, float) else v) for k, v in sorted(cfg.items())]
    return _run(["scene", directory, obj, *settings], os.path.join(scratch, "refhost_scene.%d.bin" % os.getpid()))


def dump_faces(corners, normals, alpha, scratch):
    """MathHelp::triCalcAABB over hand-made faces: corners, normals (N, 3, 3) float32 -> boxes (N, 6) float32."""
    words = np.concatenate([np.asarray(corners, np.float32).reshape(-1, 9), np.asarray(normals, np.float32).reshape(-1, 9)], axis=1)
    src = os.path.join(scratch, "refhost_faces.%d.in" % os.getpid())
    words.astype("<f4").tofile(src)
    try:
        return _run(["faces", src, "alpha=%r" % float(alpha)], os.path.join(scratch, "refhost_faces.%d.bin" % os.getpid()))["boxes"]
    finally:
        os.remove(src)
