"""The two dual-quaternion kinds in the host-only unit csrc/pt_update_host.hpp, without a GPU: pbr_update_skin_dq is admitted and
planned as pbr_update_skin is, pbr_update_pose_dq as pbr_update_pose — the same refusals with the call's own name, the same
keepsHistory, gathers, alpha and relinks from the same facts, the dq kernels for the normals — and the kinds that were there keep
their numbers.  Built from tests/update_plan_dq_driver.cpp, which takes tests/update_plan_driver.cpp's functions from its source."""
import ctypes
import itertools
import os
import subprocess

import pytest

from conftest import ROOT
from test_update_plan_cpu import (C_GENERATIONS, C_NO_BONES, C_NO_MORPH, C_NO_PATCHES, C_NO_SCENE, C_NOT_NESTED, C_ORDERED, C_PHONG, FLAGS, KINDS, MORPH,
                                  MORPH_NORMALS, NO_KERNEL, PBR_ESTATE, PBR_OK, POSE, SKIN, Facts, admit, facts, no_morph, not_nested, ordered)

DRIVER = os.path.join(ROOT, "tests", "update_plan_dq_driver.cpp")
SKIN_DQ, POSE_DQ = 7, 8
SKIN_DQ_NORMALS, POSE_DQ_NORMALS = 5, 6
CALL = {SKIN_DQ: "pbr_update_skin_dq", POSE_DQ: "pbr_update_pose_dq"}
TWIN = {SKIN_DQ: SKIN, POSE_DQ: POSE}
SKIN_DQ_NO_SKIN = "pbr_update_skin_dq without a skin: pbr_set_skin declares the influences and captures the rest pose (a new upload drops it)"
POSE_DQ_NO_SKIN = "pbr_update_pose_dq without a skin: pbr_set_skin declares the influences (a new upload drops it)"
POSE_DQ_GENERATIONS = ("pbr_update_pose_dq: pbr_set_skin and pbr_set_morph captured different geometry (an upload or an update lies between them): "
                       "set both on the same rest pose")


def _named(message, kind):
    """A refusal every kind shares, in the name of a dq kind: test_update_plan_cpu's text for the twin with the call replaced."""
    twin = {SKIN_DQ: "pbr_update_skin", POSE_DQ: "pbr_update_pose"}[kind]
    assert message.startswith(twin)
    return CALL[kind] + message[len(twin):]


CHAINS = {
    SKIN_DQ: [(C_NO_BONES, SKIN_DQ_NO_SKIN), (C_NOT_NESTED, _named(not_nested(SKIN), SKIN_DQ)), (C_ORDERED, _named(ordered(SKIN), SKIN_DQ))],
    POSE_DQ: [(C_NO_MORPH, _named(no_morph(POSE), POSE_DQ)), (C_NO_BONES, POSE_DQ_NO_SKIN), (C_GENERATIONS, POSE_DQ_GENERATIONS),
              (C_NOT_NESTED, _named(not_nested(POSE), POSE_DQ)), (C_ORDERED, _named(ordered(POSE), POSE_DQ))],
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("update_plan_dq") / "libupdateplandq.so")
    subprocess.run(["g++"] + FLAGS + ["-I", os.path.join(ROOT, "tests"), "-fPIC", "-shared", DRIVER, "-o", path], check=True, stdout=subprocess.PIPE,
                   stderr=subprocess.STDOUT, text=True)
    lib = ctypes.CDLL(path)
    u32, fp = ctypes.c_uint32, ctypes.POINTER(Facts)
    lib.up_call.argtypes, lib.up_call.restype = [u32], ctypes.c_char_p
    lib.up_admit_kind.argtypes = [u32, fp, ctypes.c_char_p, ctypes.c_size_t]
    lib.up_admit_shared.argtypes = [u32, ctypes.c_int, fp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.up_plan.argtypes = [u32, fp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)]
    lib.up_last.argtypes = [u32, ctypes.POINTER(u32)]
    lib.up_dq_code.argtypes, lib.up_dq_code.restype = [u32], u32
    lib.up_kind_values.argtypes = [ctypes.POINTER(u32)]
    lib.up_kernel_values.argtypes = [ctypes.POINTER(u32)]
    return lib


def test_the_new_kinds_are_appended_and_the_old_ones_keep_their_numbers(driver):
    kinds, kernels = (ctypes.c_uint32 * 9)(), (ctypes.c_uint32 * 7)()
    driver.up_kind_values(kinds)
    driver.up_kernel_values(kernels)
    assert list(kinds) == list(range(9)) and list(kernels) == list(range(7))
    assert list(kinds)[1:7] == list(KINDS) and (NO_KERNEL, MORPH_NORMALS) == (0, 3)
    assert {kind: driver.up_call(kind).decode() for kind in CALL} == CALL
    assert [driver.up_call(kind).decode() for kind in KINDS] == ["pbr_update_vertices", "pbr_update_geometry", "pbr_update_transforms", "pbr_update_skin",
                                                                 "pbr_update_morph", "pbr_update_pose"]


@pytest.mark.parametrize("kind", (SKIN_DQ, POSE_DQ))
def test_every_refusal_has_its_status_and_text_and_the_earlier_one_wins(driver, kind):
    assert admit(driver, kind, facts()) == (PBR_OK, "")
    chain = CHAINS[kind]
    for conditions, message in chain:
        assert admit(driver, kind, facts(**conditions)) == (PBR_ESTATE, message)
    for i, (first, message) in enumerate(chain):
        rest = {}
        for later, _ in chain[i + 1:]:
            rest.update(later)
        assert admit(driver, kind, facts(**dict(rest, **first)), True) == (PBR_ESTATE, message)


def test_refusals_that_are_another_kind_s_do_not_apply(driver):
    """What test_update_plan_cpu asks of pbr_update_skin and pbr_update_pose: Phong tessellation and missing patches refuse
    neither, an ordered walk with the flag stops nobody, a missing morph or two generations do not stop the dq skin, and the
    device kinds ask for their rest pose, not for the scene."""
    for kind in (SKIN_DQ, POSE_DQ):
        assert admit(driver, kind, facts(**C_PHONG)) == (PBR_OK, "")
        assert admit(driver, kind, facts(**C_NO_PATCHES), True) == (PBR_OK, "")
        assert admit(driver, kind, facts(configured=1, traversal=3, refitOrdered=1)) == (PBR_OK, "")
        assert admit(driver, kind, facts(configured=0, traversal=2, phongTessellation=0.5)) == (PBR_OK, "")
        assert admit(driver, kind, facts(configured=1, traversal=1)) == (PBR_ESTATE, _named(ordered(TWIN[kind], 1), kind))
        assert admit(driver, kind, facts(**C_NO_SCENE)) == (PBR_OK, "")
    assert admit(driver, SKIN_DQ, facts(**C_NO_MORPH)) == (PBR_OK, "") and admit(driver, SKIN_DQ, facts(**C_GENERATIONS)) == (PBR_OK, "")


def test_the_plan_follows_the_matrix_kinds_over_the_full_cross_product(driver):
    """ordered, gathers, relinks, keepsHistory and alpha of a dq kind are its twin's from the same facts; the normals' kernel is
    the twin's with the dq kernel in the skin's and the pose's place — a pose whose skin has no normal influences still morphs
    the normals with morphNormals."""
    modes = ((0, 2, 1), (0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 2, 1), (1, 2, 0), (1, 3, 1))
    mine, theirs, alpha, beta, cases = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 5)(), ctypes.c_float(), ctypes.c_float(), 0
    kernel_of = {0: NO_KERNEL, 2: SKIN_DQ_NORMALS, 3: MORPH_NORMALS, 4: POSE_DQ_NORMALS}
    flags = (0, 1)
    seen = set()
    for kind, (configured, traversal, walk_built), refit_ordered, patches, phong, pn, sn, mn, tracking, history, moved in itertools.product(
            (SKIN_DQ, POSE_DQ), modes, flags, flags, (0.0, 0.5), flags, flags, flags, flags, flags, flags):
        f = facts(configured=configured, traversal=traversal, walkBuilt=walk_built, refitOrdered=refit_ordered, hasPatches=patches, phongTessellation=phong,
                  partNormals=pn, skinNormals=sn, morphNormals=mn, tracking=tracking, history=history, moved=moved)
        driver.up_plan(kind, ctypes.byref(f), mine, ctypes.byref(alpha))
        driver.up_plan(TWIN[kind], ctypes.byref(f), theirs, ctypes.byref(beta))
        assert list(mine)[:4] == list(theirs)[:4] and alpha.value == beta.value and mine[4] == kernel_of[theirs[4]], (kind, list(mine), list(theirs))
        assert list(mine)[1] == patches and mine[3] == int(tracking and history and not moved)
        seen.add((kind, mine[4]))
        cases += 1
    assert cases == 2 * 7 * 2 * 2 * 2 * 8 * 8
    assert seen == {(SKIN_DQ, NO_KERNEL), (SKIN_DQ, SKIN_DQ_NORMALS), (POSE_DQ, NO_KERNEL), (POSE_DQ, SKIN_DQ_NORMALS), (POSE_DQ, MORPH_NORMALS),
                    (POSE_DQ, POSE_DQ_NORMALS)}


def test_what_the_context_reports_of_the_last_update(driver):
    """Both dq kinds are "a pbr_update_geometry" to pbr_configure's state rule, none of the morph's two to pbr_diag_morph_info,
    and 1 / 2 to pbr_diag_skin_dq_info, which answers 0 for every other kind."""
    out = (ctypes.c_uint32 * 2)()
    for kind, code in ((SKIN_DQ, 1), (POSE_DQ, 2)):
        driver.up_last(kind, out)
        assert tuple(out) == (1, 0) and driver.up_dq_code(kind) == code
    assert [driver.up_dq_code(kind) for kind in (0,) + KINDS] == [0] * 7
    driver.up_last(MORPH, out)
    assert tuple(out) == (1, 1)
