"""Every configuration dd_create accepts, away from the default, against the float64 oracle.

The rule ("Configuration matrix"): a dd_config either passes dd_create and then matches the
float64 oracle at the parity bars, in the eval forward and in forward_train, or dd_create refuses it
(tests/test_config_matrix.py, which also shows the premises used here on the CPU). The cases are
config_matrix_util.CASES: 2, 3 and 4 LiDAR channels (the NCHW stem's 2- and 3-channel forms, the NHWC4 transpose at 4,
the per-chunk LiDAR offset), the ResNet-50 image trunk with 2 LiDAR channels, 1, 33, 64 and 128 modes (the unfused
decoder chain: decoder_mk is built for 20), both ends of trunc_timestep / step_span, and on the default config the
step counts and schedules no other test runs. B = 3 distinct scenes, one fresh handle per case (the default-config
cases run on the session's handle).

Bars: those of test_parity_gpu.py, unchanged, every element compared - waypoint L2 / heading / reg and cls of every
(step, layer) 1e-4 absolute, agents 2e-3, bev_semantic_map and the taps 2e-5 relative to max(1, max |ref|). bf16
(2 LiDAR channels only: stem_pool<bf16> has a 2-channel form) at test_parity_gpu._bf16_bar. forward_train: the checks
and bars of test_train_sweep_gpu._check.

Measured on the MI355X: every case writes its figures to the parity report (test_parity_gpu._report); the table is in
DESIGN.md section 5, "Configuration matrix".

Mutations of the library this module was run against on the MI355X, each from a scratch build, and what failed:
the chunk's LiDAR offset computed with one channel - test_uneven_chunks[lidar2-*]; the two LiDAR channels swapped in
the NCHW stem's read - test_case_matches_the_oracle[lidar2-f16x3], [r50_lidar2-f16x3], test_two_lidar_channels_in_bf16,
test_uneven_chunks[lidar2-f16x3], test_forward_train[lidar2-f16x3] (the fp32 mode does not read NCHW);
ac[cfg.trunc_timestep] replaced by ac[8] - test_case_matches_the_oracle[trunc0_span1-*], [trunc999_span1000-*]; the
mode loop of the loss kernel capped at 64 - test_forward_train[modes128-*]; the truncated roll computed with
truncation, not rounding - test_case_matches_the_oracle[steps3-*], [steps7-*].
"""
import os

import numpy as np
import pytest
import torch

import batch_sweep_util as U
import config_matrix_util as C
import train_sweep_util as T
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL, _bf16_bar, _report
from test_train_sweep_gpu import _call, _check, _parts, _unequal

pytestmark = pytest.mark.gpu

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)
KNOBS = {"groups1": {"DDMI_MK_GROUPS": "1"}, "unfused": {"DDMI_DECODER_MK": "0"}}


def _tap_shapes(case):
    cfg = C.case_config(case)
    Q = cfg.num_modes
    shapes = {"img_l4": (8, 32, 2048 if cfg.image_architecture == "resnet50" else 512), "cross_in": (64, 64, 320),
              "bev_feature": (8, 8, 512), "keyval": (65, 256), "cross_bev": (4096, 256), "query_out": (31, 256)}
    for s, l in C.step_layers(case):
        shapes[f"gs_s{s}l{l}"] = (Q, 256)
        shapes[f"reg_s{s}l{l}"] = (Q, 8, 3)
        shapes[f"cls_s{s}l{l}"] = (Q,)
    return shapes


def _make_handle(case, env=None):
    """A fresh f16x3 handle of the case's config and weights; ``env``: knobs dd_create reads."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DiffusionDriveModel(C.case_config(case), C.case_state_dict(case), device=0, gemm="f16x3")
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def handles(gpu, gpu_model):
    """case -> its handle, created on first use and kept for the module (the default-config cases: the session's)."""
    made = {}

    def get(case):
        if case in C.DEFAULT_CASES:
            return gpu_model
        if case not in made:
            made[case] = _make_handle(case)
        return made[case]

    yield get
    for m in made.values():
        m.close()


_DEV, _TRUNKS, _TRUTH = {}, {}, {}


def _dev(case):
    """The case's scenes on the device (inputs, noise, timesteps, targets) and on the host."""
    if case not in _DEV:
        inp, t, tg = C.case_inputs(case)
        host = dict(inp, timesteps=t, target=tg)
        _DEV[case] = (host, {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()})
    return _DEV[case]


def _trunk(case):
    """The float64 oracle before the trajectory head, once per trunk (config_matrix_util.trunk_key)."""
    key = C.trunk_key(case)
    if key not in _TRUNKS:
        _TRUNKS[key] = C.oracle_trunk(C.case_state_dict(case), _dev(case)[0], C.case_config(case))
    return _TRUNKS[key]


def _truth(case):
    if case not in _TRUTH:
        steps, schedule = C.case_steps(case)
        _TRUTH[case] = C.oracle_case(C.case_state_dict(case), _dev(case)[0], C.case_config(case), steps, schedule,
                                     trunk=_trunk(case))
    return _TRUTH[case]


def _run(m, dev, case, n=C.BATCH):
    """One forward of the device inputs (heads and modes on) with the case's step count: (outputs, taps of the last
    chunk's ``n`` scenes); everything stays on the device."""
    out = m.forward({k: dev[k] for k in C.FEATS}, noise=dev["noise"], steps=C.case_steps(case)[0], heads=True,
                    modes=True)
    taps = {k: m.tap(k, (n,) + s) for k, s in _tap_shapes(case).items()}
    return out, taps


class _Mode:
    """The handle in a gemm mode and the case's schedule; restores what it found."""

    def __init__(self, m, mode, case):
        self.m, self.mode, self.schedule = m, mode, C.case_steps(case)[1]

    def __enter__(self):
        self.old = self.m.gemm_mode()
        self.m.set_gemm_mode(self.mode)
        self.m.set_schedule(self.schedule)
        self.m.numerics_flags(clear=True)
        return self.m

    def __exit__(self, *exc):
        self.m.set_schedule("truncated")
        self.m.set_gemm_mode(self.old)


_RUNS = {}


def _eval(handles, case, mode, tmp_path, monkeypatch):
    """The case in the mode on its handle, once: the first call of the shape, its captured replay and a profiled
    eager call with the launch log on. Returns the replay's (outputs, taps), the names that differ between the three
    in any bit, the flags and the launch-log entries."""
    if (case, mode) in _RUNS:
        return _RUNS[case, mode]
    _, dev = _dev(case)
    log = tmp_path / "launches.tsv"
    with _Mode(handles(case), mode, case) as m:
        out1, taps1 = _run(m, dev, case)
        out2, taps2 = _run(m, dev, case)
        torch.cuda.synchronize()
        flags = m.numerics_flags()
        monkeypatch.setenv("DDMI_LAUNCH_LOG", str(log))
        m.set_profiling(True)
        try:
            out3, taps3 = _run(m, dev, case)
            torch.cuda.synchronize()
        finally:
            m.set_profiling(False)
        flags |= m.numerics_flags()
    unequal = (_unequal(out1, out2) + _unequal(taps1, taps2) + [k + " (profiled)" for k in _unequal(out3, out2)]
               + [k + " (profiled)" for k in _unequal(taps3, taps2)])
    _RUNS[case, mode] = dict(out=out2, taps=taps2, unequal=unequal, flags=flags, entries=U.read_launch_log(log))
    return _RUNS[case, mode]


def _hold(r, case, mode):
    """The run against the float64 oracle at the bars, every output and tap; one line to the parity report."""
    ref = _truth(case)
    got = {k: v.double().cpu().numpy() for k, v in r["out"].items()}
    for k, v in r["taps"].items():
        got["p3" if k == "cross_in" else k] = (v[..., 256:] if k == "cross_in" else v).double().cpu().numpy()
    assert set(U.OUTPUT_NAMES) <= set(got)
    errs = C.errors(got, ref)
    worst = {}
    for k, v in errs.items():
        g = k.split("_s")[0] if k[:3] in ("gs_", "reg", "cls") and "_s" in k else k
        worst[g] = max(worst.get(g, 0.0), v)
    _report([f"== config matrix {case} {mode}: " + " ".join(f"{k} {v:.3e}" for k, v in worst.items())])
    bad = [(k, v, C.bar_of(k, BARS)) for k, v in errs.items() if not v <= C.bar_of(k, BARS)]
    assert not bad, (case, mode, bad)


def _decoder_launches(entries):
    return [d for n, d in entries if n == "decoder"]


EVAL = [(c, m) for c in C.FRESH_CASES + C.DEFAULT_CASES for m in C.gemm_modes(c)]


@pytest.mark.parametrize("case,mode", EVAL, ids=[f"{c}-{m}" for c, m in EVAL])
def test_case_matches_the_oracle(handles, tmp_path, monkeypatch, case, mode):
    """The first call, the captured replay and a profiled eager call are bit-equal in every output and tap with no
    numerics flag; every output and every tap the oracle has, at every (step, layer) the case runs, is within the bars
    of the float64 oracle; a mode count other than 20 launches no decoder megakernel, 20 modes in f16x3 do (four query
    groups at B = 3)."""
    r = _eval(handles, case, mode, tmp_path, monkeypatch)
    assert r["flags"] == 0 and not r["unequal"], (r["flags"], r["unequal"])
    for k, v in r["out"].items():
        assert torch.isfinite(v).all(), k
    if C.case_config(case).num_modes != 20:
        assert not _decoder_launches(r["entries"]), _decoder_launches(r["entries"])[:3]
    elif mode == "f16x3":
        assert U.groups_of(r["entries"], "decoder") == [4], U.groups_of(r["entries"], "decoder")
    _hold(r, case, mode)


def test_two_lidar_channels_in_bf16(handles):
    """The 2-channel form of stem_pool<bf16>: the reduced-precision mode at its own bar (test_parity_gpu._bf16_bar:
    pre-argmax tensors no worse than a fixed bar and than the reference path's own bf16 autocast)."""
    from oracle.model import OracleModel
    case = "lidar2"
    host, dev = _dev(case)
    with _Mode(handles(case), "bf16", case) as m:
        out = m.forward({k: dev[k] for k in C.FEATS}, noise=dev["noise"], modes=True)
        out2 = m.forward({k: dev[k] for k in C.FEATS}, noise=dev["noise"], modes=True)
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
    assert not _unequal(out, out2), _unequal(out, out2)
    om = OracleModel(C.case_state_dict(case), C.case_config(case))
    _bf16_bar({k: v.cpu() for k, v in out.items()}, om, tuple(host[k] for k in U.INPUT_KEYS), C.BATCH,
              "config matrix lidar2 bf16 B=3")


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("case", C.CHUNK_CASES)
def test_uneven_chunks(handles, case, mode):
    """The batch under DDMI_MAX_CHUNK=2 (chunks 2 + 1) equals the forwards of scenes [0:2] and [2:3] on the case's own
    handle to the bit, outputs and the last chunk's taps: the per-chunk LiDAR offset counts every channel and the
    noise offset every mode."""
    _, dev = _dev(case)
    assert U.chunk_ranges(C.BATCH, 2) == [(0, 2), (2, 1)]
    m2 = _make_handle(case, {"DDMI_MAX_CHUNK": "2"})
    try:
        with _Mode(m2, mode, case):
            out, taps = _run(m2, dev, case, 1)
            torch.cuda.synchronize()
            assert m2.numerics_flags() == 0
    finally:
        m2.close()
    with _Mode(handles(case), mode, case) as m:
        parts = [_run(m, {k: v[b0:b0 + n].contiguous() for k, v in dev.items()}, case, n) for b0, n in [(0, 2), (2, 1)]]
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
    joined = {k: torch.cat([p[0][k] for p in parts]) for k in out}
    assert not _unequal(out, joined), _unequal(out, joined)
    assert not _unequal(taps, parts[-1][1]), _unequal(taps, parts[-1][1])
    # (not the whole batch's bits: a forward of 2 or 1 scenes takes other K splits than one of 3, DESIGN.md section 5,
    # "Batch sweep"; both are held to the oracle)
    ref = _truth(case)
    got = {k: v.double().cpu().numpy() for k, v in out.items()}
    errs = C.errors(got, ref)
    bad = [(k, v, C.bar_of(k, BARS)) for k, v in errs.items() if not v <= C.bar_of(k, BARS)]
    assert not bad, (case, mode, bad)


@pytest.mark.parametrize("case", C.MODE_CASES)
def test_decoder_knobs_change_nothing_off_20_modes(handles, tmp_path, monkeypatch, case):
    """With a mode count other than 20 the megakernel's knobs (one query group per scene, the megakernel off) select
    nothing: fresh handles under them compute the case's outputs and taps to the bit, in both gemm modes."""
    _, dev = _dev(case)
    for knob, env in KNOBS.items():
        mk = _make_handle(case, env)
        try:
            for mode in ("f16x3", "fp32"):
                base = _eval(handles, case, mode, tmp_path, monkeypatch)
                with _Mode(mk, mode, case):
                    out, taps = _run(mk, dev, case)
                    torch.cuda.synchronize()
                    assert mk.numerics_flags() == 0
                assert not _unequal(out, base["out"]), (knob, mode, _unequal(out, base["out"]))
                assert not _unequal(taps, base["taps"]), (knob, mode, _unequal(taps, base["taps"]))
        finally:
            mk.close()


TRAIN = [(c, m) for c in C.TRAIN_CASES for m in ("f16x3", "fp32")]


@pytest.mark.parametrize("case,mode", TRAIN, ids=[f"{c}-{m}" for c, m in TRAIN])
def test_forward_train(handles, case, mode):
    """forward_train with per-scene timesteps 0, 49 and 999: the first call and its replay bit-equal with no flag, and
    the checks of test_train_sweep_gpu._check - both layers' reg and cls at the eval bars against the float64 oracle,
    each layer's loss against the float64 LossComputer on the GPU's own reg / cls within 1e-5 * max(1, |ref|) (batch
    loss and per-scene partials: above 64 modes the loss kernel's threads take two modes each), and end to end with
    the train sweep's formula."""
    from diffusiondrive_amd.config import TransfuserConfig
    host, dev = _dev(case)
    sd = C.case_state_dict(case)
    ref = T.oracle_train(sd, host, host["timesteps"], host["target"], features=_trunk(case)[0][:3])
    with _Mode(handles(case), mode, case) as m:
        out1 = _call(m, dev)
        parts1 = _parts(m, C.BATCH)
        out2 = _call(m, dev)
        parts2 = _parts(m, C.BATCH)
        torch.cuda.synchronize()
        assert m.numerics_flags() == 0
    assert not _unequal(out1, out2), _unequal(out1, out2)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(parts1, parts2))
    _check(out2, parts2, np.arange(C.BATCH), [(0, C.BATCH)], ref, host["target"], sd["_trajectory_head.plan_anchor"],
           TransfuserConfig(), f"config matrix {case} {mode}")
