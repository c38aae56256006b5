"""CPU companion of test_batch_sweep_gpu.py: what the GPU sweep rests on, shown without a GPU.

- the committed route census (tests/golden/forward_routes.json, written by tools/route_census.py) tiles 1 .. 129, and
  the sweep's batches reach every route the forward takes at any batch up to 129;
- the replica builder repeats the distinct scenes byte for byte, with period 5;
- the float64 oracle does not depend on the batch (a scene in a batch of 2 against the scene alone, <= 1e-10), so one
  oracle forward of the distinct scenes is the truth for every replica;
- the oracle is well conditioned on the degenerate scenes: its fp32 self stays within half of every parity bar of its
  float64 self, so the bars mean on those inputs what they mean on the synthetic ones.
"""
import numpy as np
import pytest

import batch_sweep_util as U
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)


@pytest.fixture(scope="module")
def ranges():
    return U.load_routes()


def test_census_ranges_tile_every_batch(ranges):
    assert ranges[0]["from"] == 1 and ranges[-1]["to"] == U.MAX_BATCH
    for a, b in zip(ranges, ranges[1:]):
        assert a["from"] <= a["to"] and b["from"] == a["to"] + 1, (a["from"], a["to"], b["from"])
        assert a["routes"] != b["routes"], (a["to"], b["from"])  # maximal runs
    for r in ranges:
        assert r["routes"] == sorted(set(r["routes"])) and r["routes"], (r["from"], r["to"])
    assert all(U.routes_at(ranges, B) for B in range(1, U.MAX_BATCH + 1))


def test_sweep_reaches_every_route(ranges):
    """The union of the route sets at the sweep's batches is the union over all batches: every kernel configuration,
    group count and form the forward can take up to 129 scenes is run against the float64 oracle by the GPU sweep."""
    assert len(U.SWEEP_ALL) <= 20 and len(set(U.SWEEP_ALL)) == len(U.SWEEP_ALL)
    assert set(U.SWEEP) <= set(U.SWEEP_ALL) and set(U.FP32_SWEEP) <= set(U.SWEEP_ALL)
    every = set().union(*(r["routes"] for r in ranges))
    swept = set().union(*(U.routes_at(ranges, B) for B in U.SWEEP_ALL))
    assert swept == every, sorted(every - swept)
    # the census saw the batch-dependent choices of the megakernels: all three decoder group counts, both tf-decoder forms
    assert {"decoder -> groups=4", "decoder -> groups=2", "decoder -> groups=1", "tfdec -> groups=4",
            "tfdec -> groups=1", "gpt_tail", "value_proj -> form=union"} <= every
    assert any("ksplit" in r for r in every) and any(r.startswith("conv_x5") for r in every)


def test_census_group_boundaries(ranges):
    """The group counts in the census are the dispatcher's: decoder 4 / 2 / 1 for B <= 16 / 17..32 / above, tf decoder
    4 up to 16 and 1 above, the fused GPT tail up to 16 (a chunked 129 runs as 65 + 64)."""
    for B in range(1, U.MAX_BATCH + 1):
        rs = U.routes_at(ranges, B)
        dec = {r for r in rs if r.startswith("decoder -> ")}
        tf = {r for r in rs if r.startswith("tfdec -> ")}
        assert dec == {"decoder -> groups=%d" % (4 if B <= 16 else 2 if B <= 32 else 1)}, (B, dec)
        assert tf == {"tfdec -> groups=%d" % (4 if B <= 16 else 1)}, (B, tf)
        assert ("gpt_tail" in rs) == (B <= 16), B


def test_route_string_drops_what_scales_with_the_batch():
    a = U.route_string("conv_x6", "M=8192 N=64 K=576 k=3 s=1 z=1 HW=64x64 cfg=conv_x6<8,8,64,2,2>")
    b = U.route_string("conv_x6", "M=16384 N=64 K=576 k=3 s=1 z=1 HW=64x64 cfg=conv_x6<8,8,64,2,2>")
    assert a == b == "conv_x6 N=64 K=576 k=3 s=1 HW=64x64 -> conv_x6<8,8,64,2,2>"
    g = U.route_string("conv_x3", "M=640 N=256 K=64 k=1 s=1 z=1 HW=640x1 cfg=conv_x3<64,64,f16x3>")
    assert g == "conv_x3 N=256 K=64 k=1 s=1 HW=rows -> conv_x3<64,64,f16x3>"
    assert U.route_string("decoder", "groups=2") == "decoder -> groups=2"
    assert U.route_string("value_proj", "form=union") == "value_proj -> form=union"
    assert U.route_string("misc", "") == "misc"
    sets = {1: ["a"], 2: ["a"], 3: ["b"], 4: ["a"]}
    assert [(r["from"], r["to"]) for r in U.ranges_of(sets)] == [(1, 2), (3, 3), (4, 4)]


def test_replica_builder():
    rng = np.random.default_rng(0)
    distinct = {k: rng.standard_normal((U.N_DISTINCT, 3, 4)).astype(np.float32) for k in U.INPUT_KEYS}
    for B in (1, 4, 5, 6, 13, 129):
        idx = U.replica_index(B)
        assert idx.tolist() == [i % U.N_DISTINCT for i in range(B)]
        rep = U.build_replicas(distinct, B)
        for k in U.INPUT_KEYS:
            assert rep[k].shape == (B, 3, 4) and rep[k].flags["C_CONTIGUOUS"]
            for i in range(B):
                assert rep[k][i].tobytes() == distinct[k][i % U.N_DISTINCT].tobytes(), (k, i)
    assert U.first_occurrence(U.replica_index(12)).tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    # a later chunk starts in the middle of a period: scenes 65 .. 128 of 129 are distinct scenes 0 1 2 3 4 0 ...
    assert U.chunk_ranges(129) == [(0, 65), (65, 64)] and U.chunk_ranges(128) == [(0, 128)]
    assert U.chunk_ranges(7, 3) == [(0, 3), (3, 3), (6, 1)]
    tail = U.replica_index(129)[65:]
    assert tail[:6].tolist() == [0, 1, 2, 3, 4, 0] and U.first_occurrence(tail)[:7].tolist() == [0, 1, 2, 3, 4, 0, 1]
    # period 5 against the groupings: within 20 scenes every distinct scene meets every position modulo 2 and 4
    seen = {(int(d), i % 4) for i, d in enumerate(U.replica_index(20))}
    assert len(seen) == 20


def test_degenerate_inputs_are_what_the_table_says():
    from diffusiondrive_amd.weights import synthetic_inputs
    drawn = synthetic_inputs(6, U.DEGENERATE_SEED)
    inp = U.degenerate_inputs()
    cam, lid, st = inp["camera_feature"], inp["lidar_feature"], inp["status_feature"]
    assert all(np.array_equal(inp[k][0], drawn[k][0]) for k in U.INPUT_KEYS)
    assert not lid[1].any() and np.array_equal(cam[1], drawn["camera_feature"][1])
    assert not cam[2].any() and np.array_equal(lid[2], drawn["lidar_feature"][2])
    assert (cam[3] == 1.0).all() and (lid[3] == 1.0).all()
    assert not cam[4].any() and not lid[4].any() and not st[4].any()
    assert st[5, 4:].tolist() == [40.0, -12.0, -9.0, 9.0] and np.array_equal(st[5, :4], drawn["status_feature"][5, :4])
    assert np.array_equal(inp["noise"], drawn["noise"]) and len(U.DEGENERATE) == 6
    assert all(v.dtype == np.float32 for v in inp.values())


def test_float64_oracle_does_not_depend_on_the_batch(seeded_sd):
    """Scene i of a float64 oracle forward of 2 scenes against the same scene alone: every output and tap within
    1e-10 (relative to max(1, max |ref|) on the maps). The fp32 oracle moves by up to 8.6e-5 with the batch (its
    BLAS blocks by it), which is why the sweep's truth is the float64 run."""
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(2, U.SCENE_SEED)
    both = U.oracle_run(seeded_sd, inp)
    assert both["trajectory"].dtype == np.float64
    for i in range(2):
        one = U.oracle_run(seeded_sd, {k: inp[k][i:i + 1] for k in U.INPUT_KEYS})
        e = U.errors({k: v[i:i + 1] for k, v in both.items()}, one)
        assert max(e.values()) <= 1e-10, (i, e)


def test_oracle_is_well_conditioned_on_the_degenerate_scenes(seeded_sd):
    """fp32 oracle against float64 oracle on the six degenerate scenes: everything finite, every output and tap within
    half of its parity bar (measured: waypoint L2 <= 1.2e-5, agent_states <= 9.8e-5, bev_semantic_map <= 2.7e-5
    absolute on values up to 29)."""
    inp = U.degenerate_inputs()
    r64 = U.oracle_run(seeded_sd, inp)
    r32 = U.oracle_run(seeded_sd, inp, np.float32)
    for k, v in r32.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    for i in range(6):
        e = U.errors({k: v[i:i + 1] for k, v in r32.items()}, {k: v[i:i + 1] for k, v in r64.items()})
        for k, v in e.items():
            assert v <= 0.5 * U.bar_of(k, BARS), (U.DEGENERATE[i], k, v)
