"""dd_forward_samples on the GPU: S trajectory samples per scene over one perception pass, against the float64 oracle.

Decoder scene d = b * S + s reads scene b's cross-BEV map, agent K / V and ego row; everything else in the trajectory
head is per decoder scene. The oracle is per scene, so the truth of a samples forward is one oracle forward of the
batch in which scene b is repeated once per noise (samples_util.oracle_batch), run through batch_sweep_util.oracle_run
(config_matrix_util.oracle_case where the config or the schedule differs). The shapes are the smallest at which the
indexing can go wrong: two scenes with three noises each (a wrong divisor - d % B, d for d / S - in a tap table, the
agent K / V, the ego row or the K / V stride reads another scene), the decoder's group boundaries by D = B * S (16, 17,
33), head passes inside uneven scene chunks, the unfused chain, the vanilla schedule, a single-stream handle, the
device draw and the best candidate.

Bars: those of test_parity_gpu.py, unchanged. Every case writes its largest errors to the parity report.
"""
import ctypes

import numpy as np
import pytest
import torch

import batch_sweep_util as U
import config_matrix_util as C
import samples_util as SU
from philox_ref import device_normals
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL, _report

pytestmark = pytest.mark.gpu

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)
FEATS = U.INPUT_KEYS[:3]
HEADS = ("bev_semantic_map", "agent_states", "agent_labels")
Q, P = U.Q, U.P


def _bits(t):
    return t.contiguous().view(torch.int32)


def _unequal(a, b):
    return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


def _dev(scenes):
    return {k: torch.from_numpy(np.ascontiguousarray(scenes[k])).cuda() for k in FEATS}


def _mode_taps(m, D, steps=2, q=Q):
    t = {}
    for s in range(steps):
        for l in range(2):
            t[f"reg_s{s}l{l}"] = m.tap(f"reg_s{s}l{l}", (D, q, P, 3)).clone()
            t[f"cls_s{s}l{l}"] = m.tap(f"cls_s{s}l{l}", (D, q)).clone()
    return t


def _flat(out, B, S):
    """A samples result by decoder scene: (B, S, ...) -> (B * S, ...); the per-scene heads stay (B, ...)."""
    return {k: (v if k in HEADS or k.startswith("best") else v.reshape((B * S,) + tuple(v.shape[2:])))
            for k, v in out.items()}


def _check(got, ref, rows, S, tag):
    """``got`` (decoder scenes on axis 0, heads by scene) against the oracle rows ``rows`` (one per decoder scene; the
    heads of a scene are those of its first sample's row): every error reported, then held to its bar."""
    rows = np.asarray(rows)
    g, r = {}, {}
    for k, v in got.items():
        g[k] = v.double().cpu().numpy()
        r[k] = ref[k][rows[::S]] if k in HEADS else ref[k][rows]
    errs = C.errors(g, r)
    _report([f"== samples {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items())])
    for k, v in errs.items():
        assert v <= C.bar_of(k, BARS), (tag, k, v, C.bar_of(k, BARS))
    return errs


@pytest.fixture(scope="module")
def handle(gpu, seeded_sd):
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    yield m
    m.close()


@pytest.fixture(scope="module")
def pairs(seeded_sd):
    """The two scenes, their three noises each, and ONE float64 oracle forward of the 6 (scene, noise) pairs."""
    from diffusiondrive_amd.weights import synthetic_inputs
    scenes = synthetic_inputs(2, SU.PAIR_SEED)
    noise = SU.sample_noise(2, 3)
    return scenes, noise, U.oracle_run(seeded_sd, SU.oracle_batch(scenes, noise))


@pytest.fixture(scope="module")
def pairs_run(handle, pairs):
    """The f16x3 samples forward of the pairs with everything requested: the first (eager) call, the captured replay
    and the replay's taps (shared by the distinct-pairs and the best-candidate cases)."""
    scenes, noise, _ = pairs
    m = handle
    m.set_gemm_mode("f16x3")
    m.numerics_flags(clear=True)
    dev, nz = _dev(scenes), torch.from_numpy(noise).cuda()
    out1 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True, best=True)
    out2 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True, best=True)
    taps = _mode_taps(m, 6)
    torch.cuda.synchronize()
    return out1, out2, taps, m.numerics_flags(), m.graph_info()


def _profiled(m, tmp_path, monkeypatch, name, fn):
    log = tmp_path / name
    monkeypatch.setenv("DDMI_LAUNCH_LOG", str(log))
    m.set_profiling(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        m.set_profiling(False)
        monkeypatch.delenv("DDMI_LAUNCH_LOG")
    return out, U.read_launch_log(log)


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
def test_one_sample_is_the_existing_forward(handle, tmp_path, monkeypatch, mode):
    """S = 1 at B = 3, heads and modes on: every output bit-equal to forward() on the same inputs and noise, and the
    profiled launches are the same route set."""
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(3, SU.PAIR_SEED + 1)
    dev, nz = _dev(inp), torch.from_numpy(inp["noise"]).cuda()
    m = handle
    m.set_gemm_mode(mode)
    try:
        m.numerics_flags(clear=True)
        ref = m.forward(dev, noise=nz, heads=True, modes=True)
        got = m.forward_samples(dev, 1, noise=nz[:, None], heads=True, modes=True)
        torch.cuda.synchronize()
        assert got["trajectory"].shape == (3, 1, P, 3) and got["poses_reg"].shape == (3, 1, Q, P, 3)
        got = _flat(got, 3, 1)
        assert sorted(got) == sorted(ref) and not _unequal(ref, got), _unequal(ref, got)
        _, log_f = _profiled(m, tmp_path, monkeypatch, "f.tsv",
                             lambda: m.forward(dev, noise=nz, heads=True, modes=True))
        got_p, log_s = _profiled(m, tmp_path, monkeypatch, "s.tsv",
                                 lambda: m.forward_samples(dev, 1, noise=nz[:, None], heads=True, modes=True))
        assert U.route_set(log_s) == U.route_set(log_f)
        assert [n for n, _ in log_s] == [n for n, _ in log_f]
        assert not _unequal(ref, _flat(got_p, 3, 1))
        assert m.numerics_flags() == 0
    finally:
        m.set_gemm_mode("f16x3")


def test_distinct_scenes_distinct_noises_f16x3(pairs, pairs_run):
    """2 scenes x 3 noises in f16x3 (the megakernel head, the union value_proj): every sample's outputs and every
    (step, layer)'s reg / cls within the bars of the oracle forward of the 6 pairs; the eager call and the captured
    replay bit-equal; no numerics flag; the captured segments are single-stream with kernel nodes only."""
    _, _, ref = pairs
    out1, out2, taps, flags, info = pairs_run
    assert flags == 0
    assert not _unequal(out1, out2), _unequal(out1, out2)
    assert info["programs"] >= 1 and info["other_nodes"] == 0 and info["multi_stream_execs"] == 0, info
    got = {k: v for k, v in _flat(out2, 2, 3).items() if not k.startswith("best")}
    got.update(taps)
    _check(got, ref, np.arange(6), 3, "B=2 S=3 f16x3")
    # the samples of a scene differ (distinct noises), the scenes differ
    t = out2["trajectory"]
    assert not torch.equal(t[0, 0], t[0, 1]) and not torch.equal(t[0, 0], t[1, 0])


def test_distinct_scenes_distinct_noises_fp32(handle, pairs):
    """The same in the fp32 mode: the unfused chain with the dense value maps (bev_sample_attn reads the map of scene
    d / S), mha_small's shared K / V batch and the hoisted-ego LayerNorm."""
    scenes, noise, ref = pairs
    m = handle
    dev, nz = _dev(scenes), torch.from_numpy(noise).cuda()
    m.set_gemm_mode("fp32")
    try:
        m.numerics_flags(clear=True)
        out1 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True)
        out2 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True)
        taps = _mode_taps(m, 6)
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
        info = m.graph_info()
    finally:
        m.set_gemm_mode("f16x3")
    assert not _unequal(out1, out2), _unequal(out1, out2)
    assert info["other_nodes"] == 0 and info["multi_stream_execs"] == 0, info
    got = _flat(out2, 2, 3)
    got.update(taps)
    _check(got, ref, np.arange(6), 3, "B=2 S=3 fp32")


def test_samples_are_independent_and_sampled(handle, pairs):
    """B = 2, S = 4 with noise[:, 2] = noise[:, 0]: sample 2 equals sample 0 to the bit in every output (a sample
    depends on its scene and its noise only), sample 1 differs from sample 0 (the noise is used)."""
    scenes = pairs[0]
    noise = SU.sample_noise(2, 4, seed=SU.NOISE_SEED + 1)
    noise[:, 2] = noise[:, 0]
    m = handle
    m.set_gemm_mode("f16x3")
    m.numerics_flags(clear=True)
    out = m.forward_samples(_dev(scenes), 4, noise=torch.from_numpy(noise).cuda(), modes=True)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    for k in ("trajectory", "poses_reg", "poses_cls"):
        assert torch.equal(_bits(out[k][:, 2]), _bits(out[k][:, 0])), k
        assert not torch.equal(out[k][:, 1], out[k][:, 0]), k


@pytest.fixture(scope="module")
def group_truth(seeded_sd):
    """Three scenes x three noises, ONE oracle forward of the 9 pairs (row b * 3 + j); the (1, 16) and (1, 17) shapes
    use scene 0 and scene 1 of them (the oracle is per scene: their 3 pairs are rows 0..2 and 3..5)."""
    from diffusiondrive_amd.weights import synthetic_inputs
    scenes = synthetic_inputs(3, SU.GROUP_SEED)
    noise = SU.sample_noise(3, 3, seed=SU.NOISE_SEED + 2)
    return scenes, noise, U.oracle_run(seeded_sd, SU.oracle_batch(scenes, noise), heads=False)


@pytest.mark.parametrize("first,B,S", [(0, 1, 16), (1, 1, 17), (0, 3, 11)])
def test_group_boundaries_follow_the_decoder_scenes(handle, group_truth, tmp_path, monkeypatch, first, B, S):
    """D = B * S = 16, 17, 33: decoder_mk runs 4, 2, 1 workgroups per decoder scene (chosen by D, not B). The noises
    repeat with period 3 over s: every repeat is bit-equal to its first occurrence, and the first occurrences are
    within the bars of the oracle forward of the distinct pairs (3, 3 and 9 of them)."""
    scenes, noise3, ref = group_truth
    sc = {k: scenes[k][first:first + B] for k in FEATS}
    noise = np.ascontiguousarray(noise3[first:first + B][:, np.arange(S) % 3])
    m = handle
    m.set_gemm_mode("f16x3")
    m.numerics_flags(clear=True)
    dev, nz = _dev(sc), torch.from_numpy(noise).cuda()
    out = m.forward_samples(dev, S, noise=nz, modes=True)
    taps = _mode_taps(m, B * S)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    period = torch.arange(S, device="cuda") % 3
    for k, v in out.items():
        assert torch.equal(_bits(v), _bits(v[:, period])), k
    firsts = (np.arange(B)[:, None] * S + np.arange(3)[None]).reshape(-1)
    got = {k: v[torch.from_numpy(firsts).cuda()] for k, v in {**_flat(out, B, S), **taps}.items()}
    rows = ((first + np.arange(B))[:, None] * 3 + np.arange(3)[None]).reshape(-1)
    _check(got, ref, rows, 3, f"B={B} S={S} (D={B * S}) f16x3")
    out_p, log = _profiled(m, tmp_path, monkeypatch, "g.tsv", lambda: m.forward_samples(dev, S, noise=nz, modes=True))
    assert U.groups_of(log, "decoder") == [SU.decoder_groups(B * S)], U.groups_of(log, "decoder")
    assert U.groups_of(log, "tfdec") == [4], U.groups_of(log, "tfdec")  # the perception part is sized by B
    assert not _unequal(out, out_p)


def test_head_passes_and_scene_chunks(gpu, seeded_sd, pairs, monkeypatch):
    """A handle under DDMI_MAX_CHUNK=4, B = 5 scenes (the pairs' two scenes, arange(5) % 2) x S = 3: scene chunks of
    3 + 2, head passes of one scene each (floor(4 / 3) = 1). Every output within the bars of the pairs' truth, the
    replay bit-equal. A head pass holds one scene's three distinct noises, so no (scene, noise) pair repeats inside
    one; the repeats inside a scene chunk (other passes of the same shape) are bit-equal. S = 5 exceeds the handle's
    limit and is refused with its name; S = 0 and DD_MAX_SAMPLES + 1 are refused on any handle."""
    from diffusiondrive_amd import _lib
    from diffusiondrive_amd.model import DiffusionDriveModel
    scenes, noise, ref = pairs
    idx = np.arange(5) % 2
    assert U.chunk_ranges(5, 4) == [(0, 3), (3, 2)] and SU.head_passes(3, 3, 4) == [(0, 1), (1, 1), (2, 1)]
    dev = _dev({k: scenes[k][idx] for k in FEATS})
    nz = torch.from_numpy(np.ascontiguousarray(noise[idx])).cuda()
    monkeypatch.setenv("DDMI_MAX_CHUNK", "4")
    m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    monkeypatch.delenv("DDMI_MAX_CHUNK")
    try:
        m.numerics_flags(clear=True)
        out1 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True, best=True)
        out2 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True, best=True)
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
        info = m.graph_info()
        with pytest.raises(_lib.DDMIError, match="max_chunk = 4"):
            m.forward_samples(dev, 5)
        lib, s = m.lib, torch.cuda.current_stream().cuda_stream
        outs = _lib.DDSampleOutputs()
        outs.trajectory = out2["trajectory"].data_ptr()
        for bad in (0, SU.MAX_SAMPLES + 1):
            rc = lib.dd_forward_samples(m.handle, dev["camera_feature"].data_ptr(), dev["lidar_feature"].data_ptr(),
                                        dev["status_feature"].data_ptr(), None, 5, bad, 2, ctypes.byref(outs), s)
            assert rc == -1 and b"S must be in [1, 32]" in lib.dd_last_error(), (bad, rc, lib.dd_last_error())
    finally:
        m.close()
    assert not _unequal(out1, out2), _unequal(out1, out2)
    assert info["other_nodes"] == 0 and info["multi_stream_execs"] == 0, info
    got = {k: v for k, v in _flat(out2, 5, 3).items() if not k.startswith("best")}
    rows = (idx[:, None] * 3 + np.arange(3)[None]).reshape(-1)
    _check(got, ref, rows, 3, "B=5 S=3 max_chunk=4 f16x3")
    for k in ("trajectory", "poses_reg", "poses_cls") + HEADS:
        assert torch.equal(_bits(out2[k][2]), _bits(out2[k][0])), k  # scenes 0 and 2 of chunk (0, 3): the same scene
    # the best candidate over the gathered passes
    cls = out2["poses_cls"].reshape(5, 3 * Q)
    assert torch.equal(out2["best_index"].long().cpu(), cls.cpu().argmax(1))
    pick = out2["poses_reg"].reshape(5, 3 * Q, P, 3)[torch.arange(5), out2["best_index"].long()]
    assert torch.equal(_bits(out2["best_trajectory"]), _bits(pick))


def test_unfused_chain_num_modes_6(gpu):
    """num_modes = 6 (the unfused chain in f16x3: mha_small over a shared K / V batch, the hoisted-ego LayerNorm,
    bev_tap_dedup's image rows, conv_x3's gathered rows), B = 2, S = 3, within the bars of the oracle."""
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import seeded_state_dict, synthetic_inputs
    cfg = TransfuserConfig(num_modes=6)
    sd = seeded_state_dict(cfg, C.WEIGHT_SEED)
    scenes = synthetic_inputs(2, SU.MODES6_SEED, cfg)
    noise = SU.sample_noise(2, 3, q=6, seed=SU.NOISE_SEED + 3)
    ref = C.oracle_case(sd, SU.oracle_batch(scenes, noise), cfg, 2, "truncated")
    m = DiffusionDriveModel(cfg, state_dict=sd, device=0, gemm="f16x3")
    try:
        m.numerics_flags(clear=True)
        dev, nz = _dev(scenes), torch.from_numpy(noise).cuda()
        out1 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True)
        out2 = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True)
        taps = _mode_taps(m, 6, q=6)
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
    finally:
        m.close()
    assert not _unequal(out1, out2), _unequal(out1, out2)
    got = _flat(out2, 2, 3)
    got.update(taps)
    _check(got, ref, np.arange(6), 3, "num_modes=6 B=2 S=3 f16x3")


def test_vanilla_schedule(handle, seeded_sd):
    """set_schedule("vanilla"), 10 steps, B = 1, S = 2 against the oracle's restatement of that schedule."""
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.weights import synthetic_inputs
    scenes = synthetic_inputs(1, SU.VANILLA_SEED)
    noise = SU.sample_noise(1, 2, seed=SU.NOISE_SEED + 4)
    ref = C.oracle_case(seeded_sd, SU.oracle_batch(scenes, noise), TransfuserConfig(), 10, "vanilla")
    m = handle
    m.set_gemm_mode("f16x3")
    m.set_schedule("vanilla")
    try:
        m.numerics_flags(clear=True)
        out = m.forward_samples(_dev(scenes), 2, noise=torch.from_numpy(noise).cuda(), steps=10, modes=True)
        taps = _mode_taps(m, 2, steps=10)
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
    finally:
        m.set_schedule("truncated")
    got = _flat(out, 1, 2)
    got.update(taps)
    _check(got, ref, np.arange(2), 2, "vanilla 10 steps B=1 S=2 f16x3")


def test_single_stream_handle_on_a_caller_stream(handle, pairs):
    """set_streams(1) and a non-default stream (the batches-in-flight mode: the forward runs on the caller's stream
    itself) with the pairs' inputs: within the bars, and the stream count is left as found."""
    scenes, noise, ref = pairs
    m = handle
    m.set_gemm_mode("f16x3")
    before = m.stream_count()
    s = torch.cuda.Stream()
    dev, nz = _dev(scenes), torch.from_numpy(noise).cuda()
    torch.cuda.synchronize()
    m.set_streams(1)
    try:
        m.numerics_flags(clear=True)
        with torch.cuda.stream(s):
            m.forward_samples(dev, 3, noise=nz, heads=True, modes=True, stream=s)
            out = m.forward_samples(dev, 3, noise=nz, heads=True, modes=True, stream=s)
        s.synchronize()
        assert m.numerics_flags() == 0
        info = m.graph_info()
    finally:
        m.set_streams(before)
    assert m.stream_count() == before
    assert info["other_nodes"] == 0 and info["multi_stream_execs"] == 0, info
    _check(_flat(out, 2, 3), ref, np.arange(6), 3, "B=2 S=3 one stream f16x3")


def test_device_noise_draw_blocks(handle):
    """noise="device": a samples call of B = 2, S = 3 draws blocks position .. position + 5 of the handle's stream
    (sample s of scene b: block position + b * S + s, 320 normals each), equal to the Philox restatement within
    float32 libm ulps (test_boundary_gpu.py's bound); a plain forward consumes one block per scene; a shard seeded at
    first_scene * S reproduces the unsharded call's blocks to the bit."""
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(4, SU.SHARD_SEED)
    dev = _dev(inp)
    two = {k: v[:2] for k, v in dev.items()}
    m = handle
    m.set_gemm_mode("f16x3")

    def noise_of(call, n):
        call()
        t = m.tap("in_noise", (n, Q, P, 2)).clone()
        torch.cuda.synchronize()
        return t

    m.set_seed(99)
    a = noise_of(lambda: m.forward_samples(two, 3, noise="device"), 6)
    b = noise_of(lambda: m.forward_samples(two, 3, noise="device"), 6)
    np.testing.assert_allclose(a.cpu().numpy().reshape(-1), device_normals(99, 0, 6 * 320), rtol=0, atol=2e-6)
    np.testing.assert_allclose(b.cpu().numpy().reshape(-1), device_normals(99, 6 * 320, 6 * 320), rtol=0, atol=2e-6)
    for bb in range(2):
        for s in range(3):
            first, n = SU.block_window(6, bb, 3, s)
            np.testing.assert_allclose(b[bb * 3 + s].cpu().numpy().reshape(-1), device_normals(99, first, n), rtol=0,
                                       atol=2e-6)
    # after a plain forward of 2 scenes the samples call starts at block 2
    m.set_seed(99)
    m.forward(two, noise="device")
    c = noise_of(lambda: m.forward_samples(two, 3, noise="device"), 6)
    np.testing.assert_allclose(c.cpu().numpy().reshape(-1), device_normals(99, 2 * 320, 6 * 320), rtol=0, atol=2e-6)
    # the shard of scenes 2..3 of a 4-scene samples run
    m.set_seed(99)
    full = noise_of(lambda: m.forward_samples(dev, 3, noise="device"), 12)
    m.set_seed(99, first_scene=2 * 3)
    half = noise_of(lambda: m.forward_samples({k: v[2:] for k, v in dev.items()}, 3, noise="device"), 6)
    assert torch.equal(_bits(half), _bits(full[6:]))


def test_best_candidate(handle, pairs, pairs_run, tmp_path, monkeypatch):
    """best_index is the first-maximum argmax of the returned poses_cls over the scene's S * Q candidates (an exact
    comparison on the kernel's own output), best_trajectory that candidate's poses_reg to the bit; the kernel runs
    only when one of the two is requested."""
    scenes, noise, _ = pairs
    _, out, _, _, _ = pairs_run
    cls = out["poses_cls"].reshape(2, 3 * Q)
    assert out["best_index"].dtype == torch.int32
    assert torch.equal(out["best_index"].long().cpu(), cls.cpu().argmax(1))  # CPU argmax: the first maximum
    s, q = out["best_index"].long() // Q, out["best_index"].long() % Q
    assert torch.equal(_bits(out["best_trajectory"]), _bits(out["poses_reg"][torch.arange(2), s, q]))
    m = handle
    m.set_gemm_mode("f16x3")
    dev, nz = _dev(scenes), torch.from_numpy(noise).cuda()
    _, log0 = _profiled(m, tmp_path, monkeypatch, "b0.tsv", lambda: m.forward_samples(dev, 3, noise=nz, modes=True))
    got, log1 = _profiled(m, tmp_path, monkeypatch, "b1.tsv",
                          lambda: m.forward_samples(dev, 3, noise=nz, modes=True, best=True))
    assert [n for n, _ in log0].count("select_best") == 0
    assert [n for n, _ in log1].count("select_best") == 1
    assert torch.equal(got["best_index"], out["best_index"])
    # ties go to the first candidate: sample 2 repeats sample 0, so every logit of sample 0 appears again at + 2 Q
    tied = noise.copy()
    tied[:, 2] = tied[:, 0]
    t = m.forward_samples(dev, 3, noise=torch.from_numpy(tied).cuda(), modes=True, best=True)
    torch.cuda.synchronize()
    assert torch.equal(t["best_index"].long().cpu(), t["poses_cls"].reshape(2, 3 * Q).cpu().argmax(1))
    assert (t["best_index"] < 2 * Q).all()


def test_agent_surface(gpu, seeded_sd, tmp_path):
    """DiffusionDriveAgent.compute_trajectories draws num_samples Trajectory objects for one scene from
    torch.randn((1, S, Q, P, 2)) on the CPU generator (as compute_trajectory draws its one noise);
    forward_trajectory(num_samples=S) is the same forward, and with the default of 1 the plain one. Each sample and the
    plain forward on that sample's noise are both within WAYPOINT_L2_TOL of the same oracle scene, so they are within
    twice that of each other."""
    from diffusiondrive_amd.agent import DiffusionDriveAgent, Trajectory
    from diffusiondrive_amd.config import TransfuserConfig
    from golden_util import waypoint_l2
    from test_agent import make_agent_input
    ckpt = tmp_path / "dd.pth"
    torch.save({"state_dict": {"agent._transfuser_model." + k: torch.from_numpy(np.asarray(v))
                               for k, v in seeded_sd.items()}}, ckpt)
    agent = DiffusionDriveAgent(TransfuserConfig(), lr=1e-4, checkpoint_path=str(ckpt), device=0)
    ai = make_agent_input(5)
    torch.manual_seed(77)
    trajs = agent.compute_trajectories(ai, 3)
    assert len(trajs) == 3 and all(isinstance(t, Trajectory) and t.poses.shape == (P, 3) for t in trajs)
    torch.manual_seed(77)
    noise = torch.randn((1, 3, Q, P, 2))
    feats = {}
    for b in agent.get_feature_builders():
        feats.update(b.compute_features(ai))
    feats = {k: v.unsqueeze(0) for k, v in feats.items()}
    again = agent.forward_trajectory(feats, noise=noise, num_samples=3)["trajectory"]
    assert again.shape == (1, 3, P, 3)
    assert np.array_equal(again[0].cpu().numpy(), np.stack([t.poses for t in trajs]))
    assert not np.array_equal(trajs[0].poses, trajs[1].poses)
    for s in range(3):
        one = agent.forward_trajectory(feats, noise=noise[:, s])["trajectory"]
        assert one.shape == (1, P, 3)
        assert waypoint_l2(one.cpu().numpy(), again[:, s].cpu().numpy()) <= 2 * WAYPOINT_L2_TOL
    with pytest.raises(ValueError, match="num_samples"):
        agent.compute_trajectories(ai, 0)
