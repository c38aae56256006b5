"""The forward with conv_x6's F(2,3) walk routed (the default), and which launches take it.

B = 16 is the smallest batch at which a launch is routed (image layer 2 reaches 256 workgroups): the sweep's five
distinct scenes repeated, every output and tap within the unchanged bars of the float64 oracle, replicas bit-equal, the
replay bit-equal to the first call, no flag; a handle created and run under DDMI_X6_WALK=0 takes the same routes with
no walk. tests/golden/x6_walk_routes.json pins the set of launches that carry ``walk=f23`` at every batch of
batch_sweep_util.SWEEP_ALL (a route string drops the token, so tests/golden/forward_routes.json is unchanged and
test_batch_sweep_gpu.py holds the routed forwards of those batches to the oracle).
"""
import json
import os

import pytest
import torch

import batch_sweep_util as U
from test_batch_sweep_gpu import _batch, _check_batch, _run, _unequal
from test_parity_gpu import WAYPOINT_L2_TOL

pytestmark = pytest.mark.gpu

WALK_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x6_walk_routes.json")


def walk_routes(entries):
    """The route strings of the launches of a profiling log that took the walk."""
    return sorted({U.route_string(n, d) for n, d in entries if "walk=f23" in d.split()})


@pytest.fixture(scope="module")
def walk_golden():
    with open(WALK_PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenes(gpu):
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED)
    return inp, {k: torch.from_numpy(inp[k]).cuda() for k in U.INPUT_KEYS}


@pytest.fixture(scope="module")
def handle(gpu, seeded_sd):
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    yield m
    m.close()


def _profiled(m, dev, last_n, log, monkeypatch):
    monkeypatch.setenv("DDMI_LAUNCH_LOG", str(log))
    m.set_profiling(True)
    try:
        out, _ = _run(m, dev, last_n)
        torch.cuda.synchronize()
    finally:
        m.set_profiling(False)
    return out, U.read_launch_log(log)


def test_forward_b16_with_the_walk_routed(handle, seeded_sd, scenes, walk_golden, tmp_path, monkeypatch):
    B = 16
    monkeypatch.delenv("DDMI_X6_WALK", raising=False)
    truth = U.oracle_run(seeded_sd, scenes[0])
    m = handle
    m.numerics_flags(clear=True)
    idx, dev = _batch(scenes, B)
    out1, taps1 = _run(m, dev, B)
    out2, taps2 = _run(m, dev, B)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    assert not _unequal(out1, out2) and not _unequal(taps1, taps2), (_unequal(out1, out2), _unequal(taps1, taps2))
    _check_batch(out2, taps2, idx, [(0, B)], truth, "B=16 f16x3, walk routed", {}, "x6 walk")
    out3, entries = _profiled(m, dev, B, tmp_path / "walk.tsv", monkeypatch)
    assert not _unequal(out3, out2), _unequal(out3, out2)
    assert walk_routes(entries) == U.routes_at(walk_golden, B) != []
    assert sum("walk=f23" in d.split() for _, d in entries) == 7   # the stride-1 convs of image layer 2

    # a handle of its own under DDMI_X6_WALK=0: the same routes, none with the walk, the direct walk's results
    from diffusiondrive_amd.model import DiffusionDriveModel
    monkeypatch.setenv("DDMI_X6_WALK", "0")
    m0 = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    try:
        m0.numerics_flags(clear=True)
        _run(m0, dev, B)   # a handle's first forward also runs its once-per-handle launches: profile the second
        out0, entries0 = _profiled(m0, dev, B, tmp_path / "direct.tsv", monkeypatch)
        assert m0.numerics_flags() == 0
    finally:
        m0.close()
    assert walk_routes(entries0) == []
    x6 = lambda es: [r for r in U.route_set(es) if r.startswith("conv_x6")]  # noqa: E731
    assert x6(entries0) == x6(entries) != []
    assert sorted(n for n, _ in entries0) == sorted(n for n, _ in entries)
    # both walks are within the waypoint bar of float64 (about 1e-5 off): they differ, by less than two bars
    d = (out0["trajectory"] - out2["trajectory"]).abs().max().item()
    print(f"== x6 walk B=16: max |trajectory(walk) - trajectory(direct)| = {d:.3e}")
    assert 0 < d <= 2 * WAYPOINT_L2_TOL, d


@pytest.mark.parametrize("B", U.SWEEP_ALL)
def test_walk_launches_are_the_pinned_ones(handle, scenes, walk_golden, tmp_path, monkeypatch, B):
    """The launches that carry walk=f23 at batch B are exactly those of tests/golden/x6_walk_routes.json."""
    monkeypatch.delenv("DDMI_X6_WALK", raising=False)
    idx, dev = _batch(scenes, B)
    _, entries = _profiled(handle, dev, U.chunk_ranges(B)[-1][1], tmp_path / "launches.tsv", monkeypatch)
    assert handle.numerics_flags() == 0
    assert walk_routes(entries) == U.routes_at(walk_golden, B), B
