"""The reference's own KERNEL text as a checker: its OpenCL C (pathtracing.cl and the parts it names) assembled as the
reference's host assembles it, compiled UNMODIFIED for the host CPU and linked with this repository's builtin shim
(oracle/refkernel/shim.cpp), trailer (oracle/refkernel/trailer.cl) and data-only driver (oracle/refkernel/driver.cpp) into
oracle/_ref/refkernel_<key>, one binary per configuration.

TEST INFRASTRUCTURE ONLY.  Nothing of the reference is copied into this repository: the recipe names its files where they
lie; the assembled text and everything compiled from it land in oracle/_ref/, which git ignores.  Where the reference's
tree does not exist, build() returns None and writes nothing; the tests that run the binaries skip there, the tests that
read the recorded outputs (tests/golden/refkernel_*.npz) run everywhere.

What the compiler reads from the reference, and so what this pins: control flow, operation order, int / double
promotions, the order of the RNG draws, which value goes where, the accumulation.  What stays this project's own choice:
  * the bits of the implementation-defined builtins — the table of oracle/pt_oracle.c, which the shim follows and, for the
    transcendental ones, calls (orc_math in liboracle.so);
  * the image stand-ins (nearest fetch, clamp to edge, on a W x H float4 array);
  * -Dconst= (the text writes through `const Scene*`) and -Dinline= (C99 `inline` alone emits no body to link against).

Placeholders are compile-time, so a configuration is a binary.  The values are formatted as the reference's host formats
them — "%u", "%lu", "%ff", and the SKY_LIGHT string — and every formatted float must parse back to the float32 the oracle
and the device are handed at run time; config_of() refuses a value that does not.
"""
import hashlib
import os
import shutil
import subprocess
import threading

import numpy as np

from . import oracle as _oracle
from .refhost import read_dump

_HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_SOURCE = "/root/reference/source"
_KERNELS = os.path.join(REFERENCE_SOURCE, "opencl")
_MAIN = "pathtracing.cl"
REF_DIR = os.path.join(_HERE, "_ref")
_OWN = os.path.join(_HERE, "refkernel")
_CLANG_DIRS = ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin")
CL_FLAGS = ("-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-target", "x86_64-unknown-linux-gnu",
            "-O2", "-ffp-contract=off", "-Dconst=", "-Dinline=", "-w")
CXX_FLAGS = ("-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-w")

INT_KEYS = ("ACCEL_STRUCT", "BRDF", "IMG_HEIGHT", "IMG_WIDTH", "SHADOW_RAYS", "MAX_DEPTH", "MAX_ADDED_DEPTH", "PHONGTESS", "SAMPLES")
FLOAT_KEYS = ("ANTI_ALIASING", "PHONGTESS_ALPHA")
STRING_KEYS = ("BVH_NUM_NODES", "BVH_TEX_DIM", "NUM_LIGHTS", "SKY_LIGHT")


def clang():
    for d in _CLANG_DIRS:
        if os.path.exists(os.path.join(d, "clang++")):
            return os.path.join(d, "clang"), os.path.join(d, "clang++")
    both = shutil.which("clang"), shutil.which("clang++")
    return both if all(both) else None


def available():
    return os.path.isdir(_KERNELS) and clang() is not None


def _f32(text):
    return np.float32(float(text))


def config_of(width, height, brdf, shadow_rays, max_depth, max_added_depth, samples, anti_aliasing, phong_tessellation,
              sky_light, num_nodes, num_lights):
    """The placeholder values of one configuration, formatted as the reference's host formats them: {name: text}."""
    aa, alpha = np.float32(anti_aliasing), np.float32(phong_tessellation)
    sky = [np.float32(v) for v in list(sky_light)[:3]]
    values = {
        "ACCEL_STRUCT": "%u" % 0, "BRDF": "%u" % int(brdf), "IMG_HEIGHT": "%u" % int(height), "IMG_WIDTH": "%u" % int(width),
        "SHADOW_RAYS": "%u" % int(shadow_rays), "MAX_DEPTH": "%u" % int(max_depth), "MAX_ADDED_DEPTH": "%u" % int(max_added_depth),
        "PHONGTESS": "%u" % (1 if alpha > 0.0 else 0), "SAMPLES": "%u" % int(samples),
        "ANTI_ALIASING": "%ff" % aa, "PHONGTESS_ALPHA": "%ff" % alpha,
        "BVH_NUM_NODES": "%u" % int(num_nodes), "BVH_TEX_DIM": "%u" % 0, "NUM_LIGHTS": "%u" % int(num_lights),
        "SKY_LIGHT": "(float4)( %f, %f, %f, 0.0f )" % tuple(sky),
    }
    for key, want in (("ANTI_ALIASING", aa), ("PHONGTESS_ALPHA", alpha)):
        if _f32(values[key][:-1]) != want:
            raise ValueError("%s = %r does not survive the reference's %%f formatting (%s)" % (key, float(want), values[key]))
    for k, want in enumerate(sky):
        if _f32("%f" % want) != want:
            raise ValueError("sky_light[%d] = %r does not survive the reference's %%f formatting" % (k, float(want)))
    return values


def key_of(values):
    return hashlib.sha1("\n".join("%s=%s" % kv for kv in sorted(values.items())).encode()).hexdigest()[:16]


def binary_of(values):
    return os.path.join(REF_DIR, "refkernel_" + key_of(values))


def assemble(values):
    """The program text as the reference's host builds it: the parts spliced in where the main file names them, then each
    placeholder replaced once."""
    with open(os.path.join(_KERNELS, _MAIN)) as f:
        text = f.read()
    while True:
        a, b = text.find("#FILE:"), text.find(":FILE#")
        if a < 0 or b < 0:
            break
        with open(os.path.join(_KERNELS, text[a + 6:b])) as f:
            text = text[:a] + f.read() + text[b + 6:]
    for name in INT_KEYS + FLOAT_KEYS + STRING_KEYS:
        at = text.find("#%s#" % name)
        if at >= 0:
            text = text[:at] + values[name] + text[at + len(name) + 2:]
    return text


def _own_sources():
    return [os.path.join(_OWN, f) for f in ("shim.cpp", "driver.cpp", "trailer.cl")]


def _reference_sources():
    return [os.path.join(_KERNELS, f) for f in sorted(os.listdir(_KERNELS)) if f.endswith(".cl")]


def _stale(target, sources):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in sources)


def _moved_into_place(target, make):
    tmp = "%s.%d.%d.tmp" % (target, os.getpid(), threading.get_ident())
    try:
        make(tmp)
        os.replace(tmp, target)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def build_shim(directory, force=False):
    """librefkernel_shim.so in `directory`: the shim alone (own text only), for the test of its builtins.  Needs clang++
    (ext_vector_type), not the reference."""
    cxx = clang()[1]
    target = os.path.join(directory, "librefkernel_shim.so")
    lib = _oracle.build()
    if force or _stale(target, [_own_sources()[0], lib]):
        _moved_into_place(target, lambda tmp: subprocess.check_call(
            [cxx, *CXX_FLAGS, "-shared", "-o", tmp, _own_sources()[0], lib, "-Wl,-rpath," + _HERE, "-lm"]))
    return target


def build(values=None, force=False):
    """oracle/_ref/refkernel_<key> for one configuration (config_of), or None where the reference's sources (or a clang)
    do not exist — nothing is touched then.  Without a configuration: only the parts every configuration shares."""
    if not available():
        return None
    cc, cxx = clang()
    os.makedirs(REF_DIR, exist_ok=True)
    lib = _oracle.build()
    shared = os.path.join(REF_DIR, "refkernel_own.a")
    if (force and values is None) or _stale(shared, _own_sources()[:2]):       # forced once, by the call without a configuration
        def make(tmp):
            objs = []
            try:
                for src in _own_sources()[:2]:
                    objs.append("%s.%s.o" % (tmp, os.path.basename(src)))
                    subprocess.check_call([cxx, *CXX_FLAGS, "-c", "-o", objs[-1], src])
                subprocess.check_call(["ar", "rcs", tmp, *objs])
            finally:
                for o in objs:
                    if os.path.exists(o):
                        os.remove(o)
        _moved_into_place(shared, make)
    if values is None:
        return shared
    target = binary_of(values)
    if force or _stale(target, _own_sources() + _reference_sources() + [shared]):
        def make(tmp):
            text, obj = tmp + ".cl", tmp + ".o"
            try:
                with open(text, "w") as f:
                    f.write(assemble(values))
                    f.write('\n#include "%s"\n' % _own_sources()[2])
                subprocess.check_call([cc, *CL_FLAGS, "-c", "-o", obj, text])
                # driver.o first: its main pulls the rest; the kernel object's plain names (rand, swap ...) stay the executable's own
                subprocess.check_call([cxx, "-o", tmp, obj, "-Wl,--whole-archive", shared, "-Wl,--no-whole-archive", lib,
                                       "-Wl,-rpath," + _HERE, "-lm"])
            finally:
                for p in (text, obj):
                    if os.path.exists(p):
                        os.remove(p)
        _moved_into_place(target, make)
    return target


def build_many(configs, force=False, jobs=None):
    """build() over several configurations at once: [binary]."""
    from concurrent.futures import ThreadPoolExecutor
    if build(None, force=force) is None:
        return None
    unique = {key_of(v): v for v in configs}
    with ThreadPoolExecutor(jobs or min(8, os.cpu_count() or 1)) as pool:
        done = dict(zip(unique, pool.map(lambda v: build(v, force=force), unique.values())))
    return [done[key_of(v)] for v in configs]


def build_recorded_cases(force=False):
    """Every configuration tests/golden/make_refkernel.py records (the call of __graft_entry__.build)."""
    if not available():
        return None
    import importlib.util
    import sys
    path = os.path.join(os.path.dirname(_HERE), "tests", "golden", "make_refkernel.py")
    spec = importlib.util.spec_from_file_location("make_refkernel", path)
    mod = importlib.util.module_from_spec(spec)
    quiet, sys.dont_write_bytecode = sys.dont_write_bytecode, True       # a build leaves nothing under tests/
    try:
        spec.loader.exec_module(mod)
        configs = [mod.values_of(mod.case_inputs(name)) for name in mod.CASES] + [mod.walk_values_of(name) for name in mod.WALK_CASES]
    finally:
        sys.dont_write_bytecode = quiet
    return build_many(configs, force=force)


_KINDS = {np.dtype(np.float32): b"f", np.dtype(np.uint32): b"u", np.dtype(np.int32): b"i"}


def write_records(path, arrays):
    with open(path, "wb") as f:
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            f.write(np.uint32(len(name)).tobytes() + name.encode() + _KINDS[a.dtype])
            f.write(np.uint32(a.ndim).tobytes() + np.array(a.shape, "<u4").tobytes() + a.astype(a.dtype.newbyteorder("<")).tobytes())


def run(values, data, seeds, first, px_dim, camera, rays, scratch, t0=None, shadow_rays=None):
    """One child process of the configuration's binary.  data: the seven wire arrays; camera: the 80 bytes of a pbr_camera;
    returns {image, debug, ray_t, ray_face, ray_normal, ray_counts}.  t0: what each closest-hit ray's t starts from (+inf
    without it); shadow_rays (n x 7: origin, dir, tLight): the reference's traverseShadows per ray — shadow_t, shadow_face,
    shadow_tests are returned too."""
    binary = build(values)
    lights = np.asarray(data["lights"], np.float32).reshape(-1, 12)
    records = {k: data[k] for k in ("bvh", "facesV", "facesN", "vertices", "normals", "materials")}
    records = {k: np.asarray(v, np.uint32 if k.startswith("faces") else np.float32) for k, v in records.items()}
    records.update(lights=lights, camera=np.frombuffer(bytes(camera), np.uint32).copy(), seeds=np.asarray(seeds, np.float32).reshape(-1),
                   first=np.array([first], np.uint32), px_dim=np.array([px_dim], np.float32),
                   rays=np.asarray(rays, np.float32).reshape(-1, 6))
    if t0 is not None:
        records["t0"] = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, np.float32), (records["rays"].shape[0],)))
    if shadow_rays is not None:
        records["shadow_rays"] = np.asarray(shadow_rays, np.float32).reshape(-1, 7)
    tag = "%s.%d" % (key_of(values), os.getpid())
    src, out = os.path.join(scratch, "refkernel_%s.in" % tag), os.path.join(scratch, "refkernel_%s.out" % tag)
    write_records(src, records)
    try:
        subprocess.check_call([binary, "in=" + src, "out=" + out], stdout=subprocess.DEVNULL)
        return read_dump(out)
    finally:
        for p in (src, out):
            if os.path.exists(p):
                os.remove(p)
