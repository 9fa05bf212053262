"""The schedule tuner (physically-based-rendering_amd/csrc/pt_tuner.hpp) on the CPU: tests/schedule_tuner_driver.cpp runs it the
way launch() does, against synthetic timings — a chunk of n frames of plan p takes (a[p] + b[p] x n) x the next noise factor
ms — and prints which chunks it ran, what it decided after every render call and every plan's fit.

The expected traces were recorded from the tuner logic as it stood inside launch() before it became a unit of its own, copied
verbatim into a throwaway copy of the driver; the same scenarios through pt_tuner.hpp must give the same traces, bit for bit
(fits included: both are built with -ffp-contract=off, as the library's host code is).

A chunk is plan:frames, then "s" while screening or "f<k>" while it times finalist k; a settled tuner's chunks have neither.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-rendering_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "schedule_tuner_driver.cpp")

NOISE = "noise 1.0 1.013 0.991 1.007 0.985 1.021 0.996 1.004 0.978 1.011\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tuner") / "schedule_tuner_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, DRIVER, "-o", exe],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return exe


def run(driver, tmp_path, scenario, noise=NOISE):
    path = tmp_path / "scenario.txt"
    path.write_text(scenario + noise)
    return subprocess.run([driver, str(path)], check=True, stdout=subprocess.PIPE, text=True).stdout


def chunks(trace):
    """(plan, frames, tag) of every chunk, in order; tag "s", "f<k>" or ""."""
    return [(int(p), int(n), t) for line in trace.splitlines() if line.startswith("call ")
            for p, n, t in re.findall(r"(\d+):(\d+)(s|f\d|)", line.split(":", 1)[1])]


def fits(trace):
    return {int(p): tuple(map(float, v.split())) for p, v in re.findall(r"^fit (\d): (.*)$", trace, re.M) if v != "none"}


def decisions(trace):
    return [int(d) for d in re.findall(r"^  -> (-?\d+)", trace, re.M)]


CLEAR_WINNER_SCENARIO = """\
scale 1
cost 0.5 1.6  0.6 1.5  0.5 1.7  0.7 1.55  0.4 1.0  0.5 1.45  0.5 0.9
calls 300
"""
CLEAR_WINNER_TRACE = """\
budget 206
call 300: 0:2s 1:2s 2:2s 3:2s 4:2s 5:2s 6:2s 6:4f0 4:4f1 4:12f1 6:12f0 6:12f0 4:12f1 4:4f1 6:4f0 6:222
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.344300 1.005675
fit 5: none
fit 6: 0.429450 0.912000
"""

CLOSE_CALL_SCENARIO = """\
scale 1
cost 0.5 1.6  0.6 1.5  0.5 1.7  0.7 1.55  0.4 1.0  0.3 1.12  0.5 0.98
calls 300
"""
CLOSE_CALL_TRACE = """\
budget 206
call 300: 0:2s 1:2s 2:2s 3:2s 4:2s 5:2s 6:2s 4:4f0 6:4f1 5:4f2 5:12f2 6:12f1 4:12f0 4:12f0 6:12f1 5:12f2 5:4f2 6:4f1 4:4f0 4:4f0 6:4f1 5:4f2 5:12f2 6:12f1 4:12f0 4:12f0 6:12f1 5:12f2 5:4f2 6:4f1 4:4f0 6:94
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.382250 1.002512
fit 5: 0.268935 1.127169
fit 6: 0.486865 0.981350
"""

VIEWER_THEN_BATCH_SCENARIO = """\
scale 1
cost 30 1.5  30 1.6  30 1.7  30 1.5  0.2 1.0  30 1.5  20.2 0.9
calls 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 100 150 250 1
"""
VIEWER_THEN_BATCH_TRACE = """\
budget 206
call 1: 0:1s
  -> -1 (measuring)
call 1: 0:1s
  -> -1 (measuring)
call 1: 1:1s
  -> -1 (measuring)
call 1: 1:1s
  -> -1 (measuring)
call 1: 2:1s
  -> -1 (measuring)
call 1: 2:1s
  -> -1 (measuring)
call 1: 3:1s
  -> -1 (measuring)
call 1: 3:1s
  -> -1 (measuring)
call 1: 4:1s
  -> -1 (measuring)
call 1: 4:1s
  -> -1 (measuring)
call 1: 5:1s
  -> -1 (measuring)
call 1: 5:1s
  -> -1 (measuring)
call 1: 6:1s
  -> -1 (measuring)
call 1: 6:1s
  -> -1 (measuring)
call 1: 4:1f0
  -> -1 (measuring)
call 1: 6:1f1
  -> -1 (measuring)
call 1: 6:1f1
  -> -1 (measuring)
call 1: 4:1f0
  -> -1 (measuring)
call 1: 4:1f0
  -> -1 (measuring)
call 1: 6:1f1
  -> -1 (measuring)
call 1: 6:1f1
  -> -1 (measuring)
call 1: 4:1f0
  -> 4
call 1: 4:1
  -> 4
call 1: 4:1
  -> 4
call 1: 4:1
  -> 4
call 1: 4:1
  -> 4
call 100: 4:4f0 6:4f1 6:12f1 4:12f0 4:12f0 6:12f1 6:4f1 4:4f0 4:36
  -> 4
call 150: 4:150
  -> 4
call 250: 6:250
  -> 6
call 1: 6:1
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.175900 1.007600
fit 5: none
fit 6: 20.180501 0.890000
"""

NEGATIVE_INTERCEPT_SCENARIO = """\
scale 1
cost 0.5 1.6  0.6 1.5  0.5 1.7  0.7 1.55  0.4 1.0  0.5 1.45  -0.3 1.0
calls 300
"""
NEGATIVE_INTERCEPT_TRACE = """\
budget 206
call 300: 0:2s 1:2s 2:2s 3:2s 4:2s 5:2s 6:2s 6:4f0 4:4f1 4:12f1 6:12f0 6:12f0 4:12f1 4:4f1 6:4f0 6:4f0 4:4f1 4:12f1 6:12f0 6:12f0 4:12f1 4:4f1 6:4f0 6:158
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.380800 1.003150
fit 5: none
fit 6: none
"""

SHARD_SCENARIO = """\
scale 8
cost 0.5 1.6  0.6 1.5  0.5 1.7  0.7 1.55  0.4 1.0  0.3 1.12  0.5 0.98
calls 2000
"""
SHARD_TRACE = """\
budget 1648
call 2000: 0:16s 1:16s 2:16s 3:16s 4:16s 5:16s 6:16s 6:32f0 4:32f1 4:96f1 6:96f0 6:96f0 4:96f1 4:32f1 6:32f0 6:32f0 4:32f1 4:96f1 6:96f0 6:96f0 4:96f1 4:32f1 6:32f0 6:864
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.254801 1.003019
fit 5: none
fit 6: 0.488303 0.980614
"""

BUDGET_SCALE_3_SCENARIO = """\
scale 3
cost 0.5 1.6  0.6 1.5  0.5 1.7  0.7 1.55  0.4 1.0  0.3 1.12  0.5 0.98
calls 700
"""
BUDGET_SCALE_3_TRACE = """\
budget 618
call 700: 0:6s 1:6s 2:6s 3:6s 4:6s 5:6s 6:6s 4:12f0 6:12f1 6:36f1 4:36f0 4:36f0 6:36f1 6:12f1 4:12f0 4:12f0 6:12f1 6:36f1 4:36f0 4:36f0 6:36f1 6:12f1 4:12f0 6:274
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.395550 1.000629
fit 5: none
fit 6: 0.445581 0.983002
"""

TUNE_LOG_SCENARIO = """\
scale 1
log
cap 5
cost 0.5 1.6  0.6 1.5  0.5 1.7  0.7 1.55  0.4 1.0  0.3 1.12  0.5 0.98
calls 7 3 40 52 15
"""
TUNE_LOG_TRACE = """\
budget 206
call 7: 0:2s
[pbr tune] screen refill-lean  2 frame(s) 3.700 ms = 1.850 ms/frame
 1:2s
[pbr tune] screen refill-wide  2 frame(s) 3.647 ms = 1.823 ms/frame
 2:2s
[pbr tune] screen phased-lean  2 frame(s) 3.865 ms = 1.932 ms/frame
 3:1s
[pbr tune] screen phased-wide  1 frame(s) 2.266 ms = 2.266 ms/frame

  -> -1 (measuring)
call 3: 3:1s
[pbr tune] screen phased-wide  1 frame(s) 2.216 ms = 2.216 ms/frame
 4:2s
[pbr tune] screen phased-mid   2 frame(s) 2.450 ms = 1.225 ms/frame

  -> -1 (measuring)
call 40: 5:2s
[pbr tune] screen refill-mid   2 frame(s) 2.530 ms = 1.265 ms/frame
 6:2s
[pbr tune] screen phased-dual  2 frame(s) 2.470 ms = 1.235 ms/frame
 4:4f0
[pbr tune] refine phased-mid   4 frame(s) 4.303 ms = 1.076 ms/frame
 6:4f1
[pbr tune] refine phased-dual  4 frame(s) 4.469 ms = 1.117 ms/frame
 5:4f2
[pbr tune] refine refill-mid   4 frame(s) 4.780 ms = 1.195 ms/frame
 5:5f2
[pbr tune] refine refill-mid   5 frame(s) 5.977 ms = 1.195 ms/frame
 6:5f1
[pbr tune] refine phased-dual  5 frame(s) 5.351 ms = 1.070 ms/frame
 4:5f0
[pbr tune] refine phased-mid   5 frame(s) 5.438 ms = 1.088 ms/frame
 4:5f0
[pbr tune] refine phased-mid   5 frame(s) 5.319 ms = 1.064 ms/frame
 6:4f1
[pbr tune] refine phased-dual  4 frame(s) 4.513 ms = 1.128 ms/frame

  -> -1 (measuring)
call 52: 5:5f2
[pbr tune] refine refill-mid   5 frame(s) 5.876 ms = 1.175 ms/frame
 5:4f2
[pbr tune] refine refill-mid   4 frame(s) 4.799 ms = 1.200 ms/frame
 6:4f1
[pbr tune] refine phased-dual  4 frame(s) 4.323 ms = 1.081 ms/frame
 4:4f0
[pbr tune] refine phased-mid   4 frame(s) 4.448 ms = 1.112 ms/frame
[pbr tune] fit phased-mid   a 0.365 ms  b 1.003 ms/frame  -> 1.0096 ms/frame at 52 frames
[pbr tune] fit phased-dual  a 0.768 ms  b 0.917 ms/frame  -> 0.9314 ms/frame at 52 frames
[pbr tune] fit refill-mid   a 0.242 ms  b 1.137 ms/frame  -> 1.1416 ms/frame at 52 frames
 6:5 6:5 6:5 6:5 6:5 6:5 6:5
  -> 6
call 15: 6:5 6:5 6:5
  -> 6
fit 0: none
fit 1: none
fit 2: none
fit 3: none
fit 4: 0.365400 1.002600
fit 5: 0.241601 1.136990
fit 6: 0.768067 0.916667
"""


def test_clear_winner_two_finalists_one_palindrome(driver, tmp_path):
    trace = run(driver, tmp_path, CLEAR_WINNER_SCENARIO)
    assert trace == CLEAR_WINNER_TRACE
    refine = [(p, n) for p, n, t in chunks(trace) if t.startswith("f")]
    # A B short, B A long, A B long, B A short
    assert refine == [(6, 4), (4, 4), (4, 12), (6, 12), (6, 12), (4, 12), (4, 4), (6, 4)]
    # kept: the lowest a / N + b at the render's length
    f = fits(trace)
    assert decisions(trace) == [min(f, key=lambda p: f[p][0] / 300 + f[p][1])]


def test_close_call_runs_a_second_round(driver, tmp_path):
    trace = run(driver, tmp_path, CLOSE_CALL_SCENARIO)
    assert trace == CLOSE_CALL_TRACE
    refine = [(p, n) for p, n, t in chunks(trace) if t.startswith("f")]
    assert len(refine) == 24 and refine[:12] == refine[12:]
    assert sorted({p for p, _ in refine}) == [4, 5, 6]


def test_viewer_then_a_batch(driver, tmp_path):
    trace = run(driver, tmp_path, VIEWER_THEN_BATCH_SCENARIO)
    assert trace == VIEWER_THEN_BATCH_TRACE
    calls = [line for line in trace.splitlines() if line.startswith("call ")]
    # single-frame calls settle on fits of one length; the first long call times the same finalists again ...
    assert calls[26] == "call 100: 4:4f0 6:4f1 6:12f1 4:12f0 4:12f0 6:12f1 6:4f1 4:4f0 4:36"
    # ... and a call > 2 x the tuned length re-decides from the (now separable) fits, without timing
    assert calls[28] == "call 250: 6:250"
    assert decisions(trace)[-4:] == [4, 4, 6, 6]


def test_negative_intercept_falls_back_to_the_mean(driver, tmp_path):
    trace = run(driver, tmp_path, NEGATIVE_INTERCEPT_SCENARIO)
    assert trace == NEGATIVE_INTERCEPT_TRACE
    assert 6 not in fits(trace) and 4 in fits(trace)


def test_shard_scales_every_length(driver, tmp_path):
    trace = run(driver, tmp_path, SHARD_SCENARIO)
    assert trace == SHARD_TRACE
    assert {n for _, n, t in chunks(trace) if t} == {16, 32, 96}


def test_budget_scale_3(driver, tmp_path):
    assert run(driver, tmp_path, BUDGET_SCALE_3_SCENARIO) == BUDGET_SCALE_3_TRACE


def test_tune_log_lines(driver, tmp_path):
    assert run(driver, tmp_path, TUNE_LOG_SCENARIO) == TUNE_LOG_TRACE


@pytest.mark.parametrize("scale", [1, 2, 3, 8, 64])
def test_budget_is_206_frames_per_scale(driver, tmp_path, scale):
    trace = run(driver, tmp_path, "scale %d\ncalls\n" % scale)
    assert trace.splitlines()[0] == "budget %d" % (206 * scale)


def test_close_call_uses_the_whole_budget(driver, tmp_path):
    trace = run(driver, tmp_path, CLOSE_CALL_SCENARIO)
    measured = sum(n for _, n, t in chunks(trace) if t)
    assert measured == int(trace.splitlines()[0].split()[1]) == 206
