"""The whole forward against the float64 oracle at every batch-dependent route, and on degenerate inputs.

The forward picks its kernels from the batch size on the host (conv_x6 / conv_x5 / conv_x3 configurations and the K
split, the query groups of decoder_mk, the workgroups of tfdec_mk, gpt_tail, the 128-scene chunking). tools/
route_census.py recorded the set of routes at every B in 1 .. 129 (tests/golden/forward_routes.json); the batches of
batch_sweep_util.SWEEP_ALL reach every one of them (tests/test_batch_sweep.py shows that, and the oracle premises used
here, on the CPU). Each batch is made of 5 distinct scenes repeated with period 5, so one float64 oracle forward of the
5 scenes is the truth for every batch, and - the kernels use no floating-point atomics and keep a fixed K order per
output element - every replica must equal the first occurrence of its scene to the bit.

Bars: those of test_parity_gpu.py, unchanged (waypoint L2 / heading / per-(step, layer) reg and cls / agents absolute;
bev_semantic_map and the taps relative to max(1, max |ref|), every element compared).

Measured on the MI355X (every case writes its figures to the parity report, test_parity_gpu._report; the table is in DESIGN.md
section 5, "Batch sweep"): over the 20 batches in f16x3 the largest waypoint L2 is 1.3e-5, reg / cls tap 1.6e-5,
agent_states 2.1e-4 (bar 2e-3), map and tap error 7.6e-6 relative (query_out; the others <= 2.3e-6); the fp32 mode,
the uneven chunks and the degenerate batch read the same within a factor of two. Every replica is bit-equal.
"""
import numpy as np
import pytest
import torch

import batch_sweep_util as U
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL, _report

pytestmark = pytest.mark.gpu

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)
FEATS = U.INPUT_KEYS[:3]
# device taps checked for replicas; p3 (the oracle's name) is columns 256.. of cross_in
TAP_SHAPES = {"img_l4": (8, 32, 512), "cross_in": (64, 64, 320), "bev_feature": (8, 8, 512), "keyval": (65, 256),
              "cross_bev": (4096, 256), "query_out": (31, 256)}
for _s, _l in U.SL:
    TAP_SHAPES[f"gs_s{_s}l{_l}"] = (U.Q, 256)
    TAP_SHAPES[f"reg_s{_s}l{_l}"] = (U.Q, U.P, 3)
    TAP_SHAPES[f"cls_s{_s}l{_l}"] = (U.Q,)


@pytest.fixture(scope="module")
def ranges():
    return U.load_routes()


@pytest.fixture(scope="module")
def scenes(gpu):
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED)
    return inp, {k: torch.from_numpy(inp[k]).cuda() for k in U.INPUT_KEYS}


@pytest.fixture(scope="module")
def truth(seeded_sd, scenes):
    """One float64 oracle forward of the 5 distinct scenes, shared by every batch and both gemm modes."""
    return U.oracle_run(seeded_sd, scenes[0])


@pytest.fixture(scope="module")
def handle(gpu, seeded_sd):
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    yield m
    m.close()


@pytest.fixture(scope="module")
def degenerate(seeded_sd):
    inp = U.degenerate_inputs()
    return inp, U.oracle_run(seeded_sd, inp)


@pytest.fixture(scope="module")
def record():
    """Largest error per quantity over the module's cases, by group; reported when the module is done."""
    rec = {}
    yield rec
    lines = []
    for group, e in rec.items():
        lines.append(f"== batch sweep summary, {group}: " + " ".join(f"{k} {v:.3e}" for k, v in sorted(e.items())))
    if lines:
        _report(lines)


def _note(record, group, errs):
    g = record.setdefault(group, {})
    for k, v in errs.items():
        g[k] = max(g.get(k, 0.0), v)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(m, dev, last_n):
    """One forward of the device inputs ``dev`` (heads and modes on): its outputs and, for the scenes of the last chunk
    (the handle's buffers hold that chunk), the taps; everything stays on the device."""
    out = m.forward({k: dev[k] for k in FEATS}, noise=dev["noise"], heads=True, modes=True)
    taps = {k: m.tap(k, (last_n,) + s) for k, s in TAP_SHAPES.items()}
    return out, taps


def _unequal(a, b):
    """Names whose tensors differ in any bit."""
    return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


def _replica_mismatches(name, t, idx, b0):
    """Scenes of ``t`` (scenes on axis 0, the chunk that starts at scene b0; ``idx`` their distinct scenes) that differ
    in any bit from the first scene of the chunk with the same distinct scene: (tap, scene, place in the chunk)."""
    first = torch.from_numpy(U.first_occurrence(idx)).to(t.device)
    ti = _bits(t).flatten(1)
    same = (ti == ti[first]).all(1)
    return [(name, b0 + i, i) for i in (~same).nonzero().flatten().tolist()]


def _first_rows(t, idx):
    """(rows of the first occurrence of every distinct scene in the chunk as float64 numpy, their distinct scenes)."""
    pos = sorted(set(U.first_occurrence(idx).tolist()))
    return t[torch.tensor(pos, device=t.device)].double().cpu().numpy(), np.asarray(idx)[pos]


def _check_batch(out, taps, idx, chunks, ref, tag, record, group):
    """Replicas to the bit within every chunk, and the first occurrences against the oracle at the bars. A chunk is
    one forward of its own batch size (another route set), so replicas are compared within their chunk and every
    chunk's first occurrences are held to the truth."""
    bad = []
    for b0, n in chunks:
        for k, v in out.items():
            bad += _replica_mismatches(k, v[b0:b0 + n], idx[b0:b0 + n], b0)
    b0, n = chunks[-1]
    for k, v in taps.items():
        bad += _replica_mismatches(k, v, idx[b0:b0 + n], b0)
    assert not bad, f"{tag}: replicas differ from their scene's first occurrence (tap, scene, place in chunk): {bad[:20]}"
    errs = {}
    for c0, cn in chunks:
        got, which = {}, None
        for k, v in out.items():
            got[k], which = _first_rows(v[c0:c0 + cn], idx[c0:c0 + cn])
        e = U.errors(got, {k: ref[k][which] for k in got})
        for k, v in e.items():
            errs[k] = max(errs.get(k, 0.0), v)
    got = {}
    for k, v in taps.items():
        if k == "cross_in":
            got["p3"], which = _first_rows(v[..., 256:], idx[b0:b0 + n])
        else:
            got[k], which = _first_rows(v, idx[b0:b0 + n])
    errs.update(U.errors(got, {k: ref[k][which] for k in got}))
    _report([f"== batch sweep {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items())])
    _note(record, group, errs)
    for k, v in errs.items():
        assert v <= U.bar_of(k, BARS), (tag, k, v, U.bar_of(k, BARS))
    return errs


def _batch(scenes, B):
    idx = U.replica_index(B)
    sel = torch.from_numpy(idx).cuda()
    return idx, {k: scenes[1][k][sel].contiguous() for k in U.INPUT_KEYS}


@pytest.mark.parametrize("B", U.SWEEP_ALL)
def test_sweep_f16x3(handle, scenes, truth, ranges, record, tmp_path, monkeypatch, B):
    """Batch B in the default mode: the first call of the shape and its captured replay are bit-equal with no flag
    raised, every replica is bit-equal to the first occurrence of its scene, the first occurrences are within the bars
    of the float64 oracle, the profiled forward takes exactly the census's routes for B (and the group counts the
    dispatcher documents) and computes the replay's outputs to the bit."""
    m = handle
    m.set_gemm_mode("f16x3")
    m.numerics_flags(clear=True)
    idx, dev = _batch(scenes, B)
    chunks = U.chunk_ranges(B)
    last_n = chunks[-1][1]
    out1, taps1 = _run(m, dev, last_n)
    out2, taps2 = _run(m, dev, last_n)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    assert not _unequal(out1, out2) and not _unequal(taps1, taps2), (_unequal(out1, out2), _unequal(taps1, taps2))
    del out1, taps1
    _check_batch(out2, taps2, idx, chunks, truth, f"B={B} f16x3", record, "sweep f16x3")

    log = tmp_path / "launches.tsv"
    monkeypatch.setenv("DDMI_LAUNCH_LOG", str(log))
    m.set_profiling(True)
    try:
        out3, _ = _run(m, dev, last_n)
        torch.cuda.synchronize()
    finally:
        m.set_profiling(False)
    entries = U.read_launch_log(log)
    got, want = set(U.route_set(entries)), set(U.routes_at(ranges, B))
    assert got == want, (B, sorted(got - want), sorted(want - got))
    assert U.groups_of(entries, "decoder") == [4 if B <= 16 else 2 if B <= 32 else 1], U.groups_of(entries, "decoder")
    assert U.groups_of(entries, "tfdec") == [4 if B <= 16 else 1], U.groups_of(entries, "tfdec")
    assert m.numerics_flags() == 0
    assert not _unequal(out3, out2), _unequal(out3, out2)


@pytest.mark.parametrize("B", U.FP32_SWEEP)
def test_sweep_fp32(handle, scenes, truth, record, B):
    """The replica and truth checks in gemm mode fp32 (the fp32-MFMA conv_gemm path, the dense value maps) at an odd
    small batch, past the decoder's group boundary and on the chunked 129."""
    m = handle
    idx, dev = _batch(scenes, B)
    chunks = U.chunk_ranges(B)
    m.set_gemm_mode("fp32")
    try:
        m.numerics_flags(clear=True)
        out1, taps1 = _run(m, dev, chunks[-1][1])
        out2, taps2 = _run(m, dev, chunks[-1][1])
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
    finally:
        m.set_gemm_mode("f16x3")
    assert not _unequal(out1, out2) and not _unequal(taps1, taps2), (_unequal(out1, out2), _unequal(taps1, taps2))
    del out1, taps1
    _check_batch(out2, taps2, idx, chunks, truth, f"B={B} fp32", record, "sweep fp32")


def test_uneven_chunks_at_inference(gpu, handle, seeded_sd, record, monkeypatch):
    """An inference forward whose last chunk is shorter (DDMI_MAX_CHUNK=3, 7 scenes: chunks 3, 3, 1): every scene within
    the bars of a float64 oracle forward of the 7 scenes, and the result bit-equal to three forwards of scenes [0:3],
    [3:6] and [6:7] on a default handle. (B = 129 of the sweep covers the default split, 65 + 64.)"""
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import synthetic_inputs
    B = 7
    inp = synthetic_inputs(B, U.CHUNK_SEED)
    ref = U.oracle_run(seeded_sd, inp)
    dev = {k: torch.from_numpy(inp[k]).cuda() for k in U.INPUT_KEYS}
    chunks = U.chunk_ranges(B, 3)
    assert chunks == [(0, 3), (3, 3), (6, 1)]
    monkeypatch.setenv("DDMI_MAX_CHUNK", "3")
    m3 = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    monkeypatch.delenv("DDMI_MAX_CHUNK")
    try:
        m3.numerics_flags(clear=True)
        out, taps = _run(m3, dev, 1)
        out_b, taps_b = _run(m3, dev, 1)
        torch.cuda.synchronize()
        assert m3.numerics_flags() == 0
    finally:
        m3.close()
    assert not _unequal(out, out_b) and not _unequal(taps, taps_b)
    handle.set_gemm_mode("f16x3")
    parts = [_run(handle, {k: v[b0:b0 + n].contiguous() for k, v in dev.items()}, n) for b0, n in chunks]
    torch.cuda.synchronize()
    assert handle.numerics_flags() == 0
    whole = {k: torch.cat([p[0][k] for p in parts]) for k in out}
    assert not _unequal(out, whole), _unequal(out, whole)
    assert not _unequal(taps, parts[-1][1]), _unequal(taps, parts[-1][1])
    # every scene is distinct: each is the first occurrence of itself
    _check_batch(out, taps, np.arange(B), chunks, ref, "uneven chunks 3+3+1 f16x3", record, "uneven chunks")


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
def test_degenerate_inputs(handle, degenerate, record, mode):
    """The six degenerate scenes (batch_sweep_util.DEGENERATE: an empty point cloud, a black frame, a saturated frame
    and histogram, all-zero inputs, a fast braking ego) in one batch: every output and tap within the bars of the
    float64 oracle, no flag, the replay bit-equal to the first call. The trunks run on bias-only or saturated
    activations here; for f16x3 that is the regime of subnormal lo halves."""
    inp, ref = degenerate
    dev = {k: torch.from_numpy(inp[k]).cuda() for k in U.INPUT_KEYS}
    m = handle
    m.set_gemm_mode(mode)
    try:
        m.numerics_flags(clear=True)
        out1, taps1 = _run(m, dev, 6)
        out2, taps2 = _run(m, dev, 6)
        torch.cuda.synchronize()
        flags = m.numerics_flags()
    finally:
        m.set_gemm_mode("f16x3")
    assert flags == 0, flags
    assert not _unequal(out1, out2) and not _unequal(taps1, taps2), (_unequal(out1, out2), _unequal(taps1, taps2))
    for k, v in out2.items():
        assert torch.isfinite(v).all(), k
    _check_batch(out2, taps2, np.arange(6), [(0, 6)], ref, f"degenerate B=6 {mode}", record, f"degenerate {mode}")
