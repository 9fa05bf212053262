"""The dealing orders of the banded work queue (physically-based-rendering_amd/csrc/pt_deal.hpp) on the CPU, through
tests/deal_order_driver.cpp: the grid of the local tiles and its spatial order, the two cost orders, the rule that picks an
order by the size of the render call, and the check of a table a caller hands in.

The expected tables (tests/deal_order_tables.py) were recorded from the order functions as they stood inside pbr_hip.hip before
they became a unit of their own, copied verbatim into a throwaway copy of the driver; the same scenarios through pt_deal.hpp
must print the same text, character for character.  The costs are whole numbers, so every comparison below is exact."""
import os
import subprocess

import pytest

import deal_order_tables as recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-rendering_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
DRIVER = os.path.join(ROOT, "tests", "deal_order_driver.cpp")
BANDS = 8
MAPS = ("equal", "rising", "random", "ties")
PBR_OK, PBR_EINVAL = 0, -1
KI = 1024


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deal") / "deal_order_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CSRC, DRIVER, "-o", exe],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return exe


def run(driver, *args, stdin=""):
    return subprocess.run([driver] + [str(a) for a in args], input=stdin, check=True, stdout=subprocess.PIPE, text=True).stdout


def parse(text):
    """The driver's "tables" output: (first, costs, spatial, cost classes, expensive last) as lists of int."""
    lines = dict(line.split(":", 1) for line in text.splitlines()[1:])
    return tuple([int(v) for v in lines[key].split()] for key in ("first", "costs", "spatial", "cost-classes", "expensive-last"))


def spatial_runs(seg, base):
    """seg, a reordering of the stretch base, cut where it steps back in base's sequence."""
    place = {t: k for k, t in enumerate(base)}
    cuts = [0] + [k for k in range(1, len(seg)) if place[seg[k]] < place[seg[k - 1]]] + [len(seg)]
    return [seg[a:b] for a, b in zip(cuts, cuts[1:]) if b > a]


def check_properties(first, cost, spatial, classes, last, all_equal):
    assert len(first) == BANDS + 1 and first[0] == 0 and first[BANDS] == len(spatial) == len(cost)
    assert sorted(spatial) == list(range(len(cost)))
    for b in range(BANDS):
        base, seg, tail = (order[first[b]:first[b + 1]] for order in (spatial, classes, last))
        assert sorted(seg) == sorted(base) and sorted(tail) == sorted(base), b
        # cost classes: at most eight spatial runs, each no cheaper than all of the next
        runs = spatial_runs(seg, base)
        assert len(runs) <= 8, (b, len(runs))
        for this, after in zip(runs, runs[1:]):
            assert min(cost[t] for t in this) >= max(cost[t] for t in after), b
        # expensive last: at most two spatial runs, the second all above the edge (the band's sorted costs at 3/4) and no such tile in the first
        runs = spatial_runs(tail, base)
        assert len(runs) <= 2, (b, len(runs))
        if base:
            edge = sorted(cost[t] for t in base)[min(len(base) - 1, (3 * len(base)) // 4)]
            assert tail == [t for t in base if cost[t] <= edge] + [t for t in base if cost[t] > edge], b
            if len(runs) == 2:
                assert all(cost[t] > edge for t in runs[1]), b
    if all_equal:
        assert classes == spatial and last == spatial


@pytest.mark.parametrize("costs", MAPS)
@pytest.mark.parametrize("grid", sorted(recorded.GRIDS))
def test_the_tables_are_the_recorded_ones(driver, grid, costs):
    got = run(driver, "tables", *recorded.GRIDS[grid], costs)
    want = dict(recorded.SPATIAL[grid], **recorded.COST_ORDERS[grid, costs])
    lines = got.splitlines()
    assert lines[0] == want["grid"]
    for line in lines[1:]:
        key, values = line.split(":", 1)
        if key != "costs":                                             # the test's own input
            assert values == (" " + want[key] if want[key] else ""), (grid, costs, key)
    assert [line.split(":")[0] for line in lines[1:]] == ["first", "costs", "spatial", "cost-classes", "expensive-last"]
    check_properties(*parse(got), all_equal=(costs == "equal"))


def test_the_edge_grids_are_what_they_are_meant_to_be():
    """The recorded cases cover: bands of unequal rows, a ragged last row, one row per band, fewer rows than bands, no tiles."""
    first = {name: [int(v) for v in recorded.SPATIAL[name]["first"].split()] for name in recorded.SPATIAL}
    assert recorded.SPATIAL["200x120"]["grid"] == "grid 25 x 15, 375 tiles" and len(set(b - a for a, b in zip(first["200x120"], first["200x120"][1:]))) > 1
    assert recorded.SPATIAL["200x120 rank 1 of 3"]["grid"] == "grid 9 x 14, 125 tiles" and 125 % 9 != 0
    assert first["64x64"] == list(range(0, 65, 8))
    assert first["16x8"] == [0] * 8 + [2]                               # seven bands without tiles
    assert first["8x8 rank 1 of 2"] == [0] * 9


def test_the_cost_orders_of_a_1080p_grid(driver):
    first, cost, spatial, classes, last = parse(run(driver, "tables", 1920, 1080, 1, 0, "random"))
    assert len(spatial) == 240 * 135
    check_properties(first, cost, spatial, classes, last, all_equal=False)


SPATIAL, CLASSES, LAST = "0 spatial", "1 cost-classes", "2 expensive-last"
SIZES = (128 * KI, 128 * KI + 1, 192 * KI, 192 * KI + 1, KI * KI, KI * KI + 1)


def rule_cases():
    """(pinned, learnt, knob, settled, sharded, tiles, frames) -> the driver's line, read from dealOrder() / adaptiveDealTable()
    as they stood."""
    cases = []
    for size in SIZES:
        for tiles, frames in ((size, 1), (1, size)) + (((size // 256, 256),) if size % 256 == 0 else ()):
            unsharded = CLASSES if size <= 128 * KI else SPATIAL if size <= 192 * KI else LAST
            sharded = CLASSES if size <= KI * KI else LAST
            cases.append(((0, 1, -1, 1, 0, tiles, frames), unsharded))
            cases.append(((0, 1, -1, 1, 1, tiles, frames), sharded))
            for shard in (0, 1):
                cases.append(((0, 0, -1, 1, shard, tiles, frames), SPATIAL))          # no costs learnt
                cases.append(((0, 0, 2, 1, shard, tiles, frames), SPATIAL))
                cases.append(((0, 1, 0, 1, shard, tiles, frames), SPATIAL))           # the knob: always spatial
                cases.append(((1, 1, -1, 1, shard, tiles, frames), "0 pinned"))
                cases.append(((1, 1, 1, 1, shard, tiles, frames), "0 pinned"))
                cases.append(((1, 0, 0, 0, shard, tiles, frames), "0 pinned"))
                cases.append(((0, 1, -1, 0, shard, tiles, frames), SPATIAL))          # the tuner is still measuring
                for settled in (0, 1):                                                # a positive knob forces its order, settled or not
                    cases.append(((0, 1, 1, settled, shard, tiles, frames), CLASSES))
                    cases.append(((0, 1, 2, settled, shard, tiles, frames), LAST))
                    cases.append(((0, 1, 3, settled, shard, tiles, frames), LAST))
                    cases.append(((0, 1, 7, settled, shard, tiles, frames), LAST))
    return cases


def test_the_size_rule(driver):
    cases = rule_cases()
    got = run(driver, "rule", stdin="".join(" ".join(map(str, args)) + "\n" for args, _ in cases)).splitlines()
    assert len(got) == len(cases)
    for (args, want), line in zip(cases, got):
        assert line == want, args


def check(driver, grid, order, first=None):
    text = run(driver, "check", *recorded.GRIDS[grid], stdin=" ".join(map(str, [len(order)] + list(order) + list(first or []))))
    status, _, message = text.rstrip("\n").partition(" ")
    return int(status), message


@pytest.mark.parametrize("grid", ["64x64", "200x120 rank 1 of 3"])
def test_the_check_of_a_callers_table(driver, grid):
    order = [int(v) for v in recorded.SPATIAL[grid]["spatial"].split()]
    first = [int(v) for v in recorded.SPATIAL[grid]["first"].split()]
    n = len(order)
    assert check(driver, grid, order) == (PBR_OK, "")
    assert check(driver, grid, order, first) == (PBR_OK, "")
    reverse = [t for b in range(BANDS) for t in reversed(order[first[b]:first[b + 1]])]
    assert check(driver, grid, reverse) == (PBR_OK, "")

    status, why = check(driver, grid, order[:-1])                                     # the wrong count
    assert status == PBR_EINVAL and "%u entries, the queue has %u tiles" % (n - 1, n) in why
    status, why = check(driver, grid, order + [0])
    assert status == PBR_EINVAL and "%u entries, the queue has %u tiles" % (n + 1, n) in why

    twice = list(order); twice[1] = twice[0]                                          # a tile named twice
    status, why = check(driver, grid, twice)
    assert status == PBR_EINVAL and "entry 1 (tile %u) is not a tile of band 0, or is named twice" % order[0] in why
    status, why = check(driver, grid, twice, first)
    assert status == PBR_EINVAL and "or is named twice" in why

    beyond = list(order); beyond[first[3]] = n                                        # a tile the queue does not have
    for given in (None, first):
        status, why = check(driver, grid, beyond, given)
        assert status == PBR_EINVAL and "entry %u (tile %u) is not a tile of band 3" % (first[3], n) in why

    swapped = list(order); swapped[first[0]], swapped[first[7]] = order[first[7]], order[first[0]]
    status, why = check(driver, grid, swapped)                                        # a tile in another band's stretch
    assert status == PBR_EINVAL and "entry 0 (tile %u) is not a tile of band 0" % order[first[7]] in why
    assert check(driver, grid, swapped, first) == (PBR_OK, "")                        # ... which band_first allows: any partition
    assert check(driver, grid, sorted(order), [0, 1, 1, 1, n - 2, n - 2, n - 1, n, n]) == (PBR_OK, "")

    status, why = check(driver, grid, order, [1] + first[1:])
    assert status == PBR_EINVAL and "band_first[0] = 0, band_first[8] = %u" % n in why
    status, why = check(driver, grid, order, first[:-1] + [n - 1])
    assert status == PBR_EINVAL and "the bands' stretches must cover the table" in why
    status, why = check(driver, grid, order, first[:3] + [first[2] - 1] + first[4:])
    assert status == PBR_EINVAL and "band_first must not decrease (band 2)" in why
