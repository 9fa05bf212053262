"""The hand-scheduled node phases (pt_kernel.hpp nodePhaseAsm / nodePhaseAsmCompact, pt_dual.hpp nodePhaseDualPipe) send a
visit's cold request before anything else: the cold lanes come from the walk's mask, the lanes that just parked and one signed
compare, and the resident lanes, the walk's next mask, the park mask and "nobody goes on" are worked out behind the global
loads, with the cold lanes — whose cursor register the load may overwrite at any time — out of EXEC.  In the two-walk loop
walk A's last visit takes the counted wait while walk B's request is in flight.  The shapes at which that order can go wrong
— cold, resident, parked and ended lanes in one visit; a visit all cold or all resident; a request without any lane; a phase
that ends on its first departure or only when nobody walks; the any-hit and the compact loops — against the CPU oracle, bit
for bit: image, debug image and the four counters.  Small generated scenes at 64 x 64, three frames in one pbr_render; the
scene table, the oracle renders (one per scene, shared with that file's cases) and the comparison are those of
test_gpu_node_phase_fetch_order.py."""
import pytest

import test_gpu_node_phase_fetch_order as base

pytestmark = pytest.mark.gpu

PLANS = (0, 1, 2, 3, 4, 5, 6)
WHOLE_TREE = 1 << 20        # knob lds_slots: a cap, so anything above the tree's size stages all of it
MOST_OF_MID = 1700


def test_the_scenes_have_the_sizes_the_cases_rely_on(pbr, oracle):
    assert base.SCENES["mid"][:3] == ("hairball", 3, 2400) and base.SCENES["large"][:3] == ("sponza", 4, 6000)
    assert base.SCENES["mid_compact"][4] == 3 and base.SCENES["large_compact"][4] == 3 and base.SCENES["mid_ordered"][4] == 2
    assert base.reference(pbr, oracle, "cornell")[1].num_nodes < 64
    # MOST_OF_MID staged records leave a few hundred cold ones in every plan
    assert MOST_OF_MID + 200 <= base.reference(pbr, oracle, "mid")[1].num_nodes <= MOST_OF_MID + 500
    assert base.reference(pbr, oracle, "large")[1].num_nodes > 5200      # a block's share of LDS holds at most 5112 records
    for name in ("mid_compact", "mid_ordered"):
        assert base.reference(pbr, oracle, name)[1].num_nodes == base.reference(pbr, oracle, "mid")[1].num_nodes
    assert base.reference(pbr, oracle, "large_compact")[1].num_nodes == base.reference(pbr, oracle, "large")[1].num_nodes


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name,lds_slots", [
    ("mid", 0), ("mid", 8), ("mid", MOST_OF_MID), ("mid", None),     # cold, resident, parked and ended lanes in one visit
    ("large", 8), ("large", None),
    ("cornell", 0),                  # every visit all cold: no resident lane ever, the global loads carry every lane that goes on
    ("cornell", WHOLE_TREE),         # every visit all resident: the global loads issue with an empty EXEC
])
def test_cold_resident_and_ended_lanes_bit_exact(pbr, oracle, gpu_device, name, lds_slots, plan):
    base.check(pbr, oracle, gpu_device, name, plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, None])
def test_nobody_goes_on_bit_exact(pbr, oracle, gpu_device, lds_slots, plan):
    """Every walk ends on its first visit: the request that follows has neither kind of lane."""
    base.check(pbr, oracle, gpu_device, "mid_all_miss", plan, lds_slots)


@pytest.mark.parametrize("plan", [2, 4, 6])
@pytest.mark.parametrize("ph_park", [1, 128])
@pytest.mark.parametrize("lds_slots", [8, None])
def test_phase_length_extremes_bit_exact(pbr, oracle, gpu_device, lds_slots, ph_park, plan):
    """ph_park 1: the phase ends on its first departure, so walk A's last visit regularly finds walk B's request in flight
    (the counted wait of the last visit); ph_park 128: the phase runs until nobody walks."""
    base.check(pbr, oracle, gpu_device, "mid", plan, lds_slots, ph_park)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, 4, None])
@pytest.mark.parametrize("name", ["lit_brdf1", "lit_brdf0"])
def test_any_hit_loop_bit_exact(pbr, oracle, gpu_device, name, lds_slots, plan):
    base.check(pbr, oracle, gpu_device, name, plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS[:6])                  # (compact records have no two-paths kernel)
@pytest.mark.parametrize("lds_slots", [0, 8, None])
@pytest.mark.parametrize("name", ["mid_compact", "large_compact"])
def test_compact_loop_bit_exact(pbr, oracle, gpu_device, name, lds_slots, plan):
    base.check(pbr, oracle, gpu_device, name, plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, 8, None])
def test_ordered_walk_bit_exact(pbr, oracle, gpu_device, lds_slots, plan):
    base.check(pbr, oracle, gpu_device, "mid_ordered", plan, lds_slots)
