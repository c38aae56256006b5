"""forward_train (dd_forward_train: the per-scene FiLM and add-noise paths of decoder_mk, train_loss.hip) against a
float64 oracle at every batch-dependent route, in every form of the trajectory head and on doctored weights.

The batches of train_sweep_util.TRAIN_SWEEP run in order on one f16x3 handle. Scene i of a batch is distinct scene
i % 5 with that scene's inputs, noise, timestep (0, 49, 7, 999, 500) and target, so one float64 oracle forward_train
of the 5 scenes is the truth for every batch, every replica must equal the first occurrence of its scene in its chunk
to the bit, and a FiLM row or add-noise coefficient taken from a neighbouring scene carries another timestep.
tests/test_train_sweep.py shows the premises (the oracle's conditioning at every timestep, the anchor margins, the
doctored cases) on the CPU.

Bars. Outputs: those of test_parity_gpu.py (MODE_TOL absolute on both layers' reg and cls, WAYPOINT_L2_TOL /
HEADING_TOL on the trajectory). Loss kernels alone - trajectory_loss_l against oracle.loss_computer in float64 on the
GPU's own reg and cls of that call: 1e-5 * max(1, |ref|), test_train_loss.LOSS_TOL["trajectory_loss"]; the kernels'
fp32 chain is 44 sequential adds per scene (20 focal terms, 24 |differences|), then at most 2 adds per thread and an
8-level tree over non-negative partials: under 3e-6 relative. The per-scene partial sums of the last chunk get the same
bar per scene. Loss end to end against the truth: 1e-5 * |ref| + reg_w * e_reg + cls_w * e_cls with the layer's errors
just measured (the loss is 1-Lipschitz in the selected mode's mean |d reg| and below 1 in mean |d cls|).

Measured on the MI355X: every case writes its figures to the parity report (test_parity_gpu._report); the table is in
DESIGN.md section 5, "Training sweep".
"""
import os

import numpy as np
import pytest
import torch

import batch_sweep_util as U
import train_sweep_util as T
from test_decoder_edges_gpu import FORMS, MEGAKERNEL_FORMS, _has_tap
from test_parity_gpu import HEADING_TOL, MODE_TOL, WAYPOINT_L2_TOL, _report
from test_train_loss import LOSS_TOL

pytestmark = pytest.mark.gpu

OUT_KEYS = ("trajectory", "reg_l0", "reg_l1", "cls_l0", "cls_l1")
LOSS_KEYS = ("loss_0", "loss_1", "loss")
LOSS_BAR = LOSS_TOL["trajectory_loss"]


def _bar(name):
    return WAYPOINT_L2_TOL if name == "waypoint_l2" else HEADING_TOL if name == "heading" else MODE_TOL


def _bits(t):
    return t.contiguous().view(torch.int32)


def _unequal(a, b):
    """Names whose tensors differ in any bit."""
    return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


@pytest.fixture(scope="module")
def cfg():
    from diffusiondrive_amd.config import TransfuserConfig
    return TransfuserConfig()


@pytest.fixture(scope="module")
def ranges():
    return U.load_routes()


@pytest.fixture(scope="module")
def scenes(gpu):
    """The 5 distinct scenes on the host and on the device (inputs, noise, timesteps, targets)."""
    inp, t, tg = T.distinct_scenes()
    host = dict(inp, timesteps=t, target=tg)
    return host, {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}


@pytest.fixture(scope="module")
def truth(seeded_sd, scenes):
    """One float64 oracle forward_train of the 5 distinct scenes, shared by every batch and form."""
    host = scenes[0]
    return T.oracle_train(seeded_sd, host, host["timesteps"], host["target"])


@pytest.fixture(scope="module")
def handle(gpu, seeded_sd):
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    yield m
    m.close()


def _make_handle(sd, form):
    """A fresh handle of the form (test_decoder_edges_gpu.FORMS; the knobs are read at dd_create)."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    mode, env = FORMS[form]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DiffusionDriveModel(state_dict=sd, device=0, gemm=mode)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _batch(scenes, B):
    """(distinct scene of every scene, the batch on the device): built on the device by indexing."""
    idx = U.replica_index(B)
    sel = torch.from_numpy(idx).cuda()
    return idx, {k: v[sel].contiguous() for k, v in scenes[1].items()}


def _call(m, dev, targets=True):
    """One forward_train on device tensors, heads off, no fp32 re-run (the caller reads the flags): the outputs by the
    oracle's names and, with targets, the three losses as 0-d tensors; everything stays on the device."""
    out = m.forward_train({k: dev[k] for k in T.FEATS}, {"trajectory": dev["target"]} if targets else None,
                          timesteps=dev["timesteps"], noise=dev["noise"], heads=False, safe=False)
    res = {"trajectory": out["trajectory"]}
    for l in range(2):
        res[f"reg_l{l}"], res[f"cls_l{l}"] = out["poses_reg_list"][l], out["poses_cls_list"][l]
    assert all(v.is_cuda for v in res.values())
    assert ("trajectory_loss" in out) == targets
    if targets:
        for l in range(2):
            res[f"loss_{l}"] = out["trajectory_loss_dict"][f"trajectory_loss_{l}"]
        res["loss"] = out["trajectory_loss"]
    return res


def _parts(m, n):
    """The last chunk's per-scene LossComputer partials of both layers, (n, 2) each."""
    return [m.tap(f"train_part_l{l}", (n, 2)) for l in range(2)]


def _replica_mismatches(name, t, idx, b0):
    first = torch.from_numpy(U.first_occurrence(idx)).to(t.device)
    ti = _bits(t).flatten(1)
    same = (ti == ti[first]).all(1)
    return [(name, b0 + i, i) for i in (~same).nonzero().flatten().tolist()]


def _check(out, parts, idx, chunks, ref, target, anchor, cfg, tag):
    """Everything one call with targets is held to: replicas to the bit within every chunk; the first occurrences of
    every chunk against the float64 truth ``ref`` (its scenes indexed by ``idx``) at the parity bars; the loss kernels
    alone against the float64 LossComputer on the GPU's own outputs (batch losses, and the last chunk's per-scene
    partials); trajectory_loss the fp32 sum of the layers' to the bit; the losses end to end against the truth's.
    One line with every figure goes to the parity report. Returns the figures."""
    bad = []
    for b0, n in chunks:
        for k in OUT_KEYS:
            bad += _replica_mismatches(k, out[k][b0:b0 + n], idx[b0:b0 + n], b0)
    assert not bad, f"{tag}: replicas differ from their scene's first occurrence (output, scene, place in chunk): {bad[:20]}"
    host = {k: out[k].cpu().numpy() for k in OUT_KEYS + LOSS_KEYS}
    for k in LOSS_KEYS:
        assert np.isfinite(host[k]), (tag, k, host[k])
    errs = {}
    for b0, n in chunks:
        pos = np.array(sorted(set(U.first_occurrence(idx[b0:b0 + n]).tolist()))) + b0
        e = T.train_errors({k: host[k][pos] for k in OUT_KEYS}, {k: ref[k][idx[pos]] for k in OUT_KEYS})
        for k, v in e.items():
            errs[k] = max(errs.get(k, 0.0), v)
    figs = dict(errs)
    fails = [(k, v, _bar(k)) for k, v in errs.items() if not v <= _bar(k)]

    # the loss kernels alone: float64 LossComputer on the GPU's own reg / cls
    b0, n = chunks[-1]
    for l in range(2):
        reg, cls = host[f"reg_l{l}"], host[f"cls_l{l}"]
        alone = T.loss64(reg, cls, target, anchor, cfg)
        got = float(host[f"loss_{l}"])
        figs[f"loss_{l}_kernel"] = abs(got - alone) / max(1.0, abs(alone))
        if not abs(got - alone) <= LOSS_BAR * max(1.0, abs(alone)):
            fails.append((f"loss_{l} against LossComputer on the GPU's outputs", got, alone))
        pref = T.scene_partials64(reg[b0:b0 + n], cls[b0:b0 + n], target[b0:b0 + n], anchor)
        pgot = parts[l].double().cpu().numpy()
        assert np.isfinite(pgot).all(), (tag, l)
        perr = np.abs(pgot - pref) / np.maximum(1.0, np.abs(pref))
        figs[f"part_l{l}"] = float(perr.max())
        if not (perr <= LOSS_BAR).all():
            worst = np.unravel_index(perr.argmax(), perr.shape)
            fails.append((f"train_part_l{l} (scene in chunk, focal | l1)", worst, pgot[worst], pref[worst]))
        # end to end against the truth's loss
        want = T.loss64(ref[f"reg_l{l}"][idx], ref[f"cls_l{l}"][idx], target, anchor, cfg)
        bar = (LOSS_BAR * abs(want) + cfg.trajectory_reg_weight * errs[f"reg_l{l}"]
               + cfg.trajectory_cls_weight * errs[f"cls_l{l}"])
        figs[f"loss_{l}_truth"] = abs(got - want) / abs(want)
        if not abs(got - want) <= bar:
            fails.append((f"loss_{l} against the truth", got, want, bar))
    s = np.float32(host["loss_0"]) + np.float32(host["loss_1"])
    if s.tobytes() != np.float32(host["loss"]).tobytes():
        fails.append(("trajectory_loss is not the fp32 sum of the layers'", host["loss"], s))
    _report([f"== train sweep {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in figs.items())])
    assert not fails, (tag, fails)
    return figs, host


TRAIN_GEMMS = {(256, 1024), (1024, 256), (256, 512)}  # (K, N) of the rows = B GEMMs: the time MLP, the FiLM Linear


def _train_gemm_routes(entries, chunks):
    """Route strings of the launches the eval forward does not have: the k = 1 GEMMs with one row per scene of a chunk
    and a training (K, N)."""
    rows = {n for _, n in chunks}
    out = set()
    for name, detail in entries:
        tok = dict(t.split("=", 1) for t in detail.split() if "=" in t)
        if tok.get("k") == "1" and int(tok.get("M", -1)) in rows and (int(tok["K"]), int(tok["N"])) in TRAIN_GEMMS:
            out.add(U.route_string(name, detail))
    return sorted(out)


def _profiled(m, dev, chunks, tmp_path, monkeypatch):
    """One profiled call with the launch log on: (outputs, log entries)."""
    log = tmp_path / "launches.tsv"
    monkeypatch.setenv("DDMI_LAUNCH_LOG", str(log))
    m.set_profiling(True)
    try:
        out = _call(m, dev)
        torch.cuda.synchronize()
    finally:
        m.set_profiling(False)
    return out, U.read_launch_log(log)


@pytest.mark.parametrize("B", T.TRAIN_SWEEP)
def test_train_sweep_f16x3(handle, scenes, truth, ranges, seeded_sd, cfg, tmp_path, monkeypatch, B):
    """Batch B with targets in the default mode: the first call of the shape and its captured replay are bit-equal in
    every output and loss with no flag raised; the checks of _check; the profiled call runs decoder_mk with the group
    count the dispatcher documents for every chunk and computes the replay's results to the bit. The routes of the
    launches the eval forward does not have (the rows = B GEMMs of the time MLP and the FiLM Linear) go to the parity
    report; there is no committed census for training, so they are not asserted."""
    m = handle
    m.set_gemm_mode("f16x3")
    m.numerics_flags(clear=True)
    idx, dev = _batch(scenes, B)
    chunks = U.chunk_ranges(B)
    out1 = _call(m, dev)
    parts1 = _parts(m, chunks[-1][1])
    out2 = _call(m, dev)
    parts2 = _parts(m, chunks[-1][1])
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    assert not _unequal(out1, out2), _unequal(out1, out2)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(parts1, parts2))
    del out1, parts1
    _check(out2, parts2, idx, chunks, truth, scenes[0]["target"][idx], seeded_sd["_trajectory_head.plan_anchor"], cfg,
           f"B={B} f16x3")

    out3, entries = _profiled(m, dev, chunks, tmp_path, monkeypatch)
    want = sorted({4 if n <= 16 else 2 if n <= 32 else 1 for _, n in chunks})
    assert U.groups_of(entries, "decoder") == want, (U.groups_of(entries, "decoder"), want)
    assert m.numerics_flags() == 0
    assert not _unequal(out3, out2), _unequal(out3, out2)
    evals = set().union(*(U.routes_at(ranges, n) for _, n in chunks))
    _report([f"== train sweep B={B} f16x3 training-only GEMM routes: " + "; ".join(_train_gemm_routes(entries, chunks)),
             f"== train sweep B={B} f16x3 routes outside the eval census of its chunks: "
             + "; ".join(sorted(set(U.route_set(entries)) - evals))])


def test_no_target_call_between_target_calls(handle, scenes):
    """B = 33 on the sweep's handle: a call with targets, two without (the first of that shape, then its replay) and
    one with targets again. Reg, cls and the trajectory are bit-equal throughout, the losses of the two target calls
    are bit-equal, and a call without targets returns no loss."""
    m = handle
    m.set_gemm_mode("f16x3")
    m.numerics_flags(clear=True)
    _, dev = _batch(scenes, 33)
    t1 = _call(m, dev)
    n1 = _call(m, dev, targets=False)
    n2 = _call(m, dev, targets=False)
    t2 = _call(m, dev)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    assert set(n1) == set(OUT_KEYS)
    assert not _unequal(n1, t1) and not _unequal(n2, t1), (_unequal(n1, t1), _unequal(n2, t1))
    assert not _unequal(t2, t1), _unequal(t2, t1)
    assert all(torch.isfinite(t1[k]) for k in LOSS_KEYS)


def test_timestep_range_is_checked_before_any_gpu_work(handle, scenes):
    """A timestep of -1 or 1000 raises ValueError before anything is staged: the features of these calls hold no
    camera or LiDAR tensor, so reaching the staging would raise KeyError instead. A device tensor of timesteps is
    checked as well; the documented ends 0 and 999 are accepted (the sweep runs them)."""
    feats = {"status_feature": torch.zeros(2, 8)}
    nz = torch.zeros(2, T.Q, T.P, 2)
    for bad in (-1, 1000):
        for safe in (False, True):
            with pytest.raises(ValueError, match="timesteps must lie in"):
                handle.forward_train(feats, None, timesteps=torch.tensor([0, bad]), noise=nz, heads=False, safe=safe)
        with pytest.raises(ValueError, match="timesteps must lie in"):
            handle.forward_train(feats, None, timesteps=torch.tensor([bad, 0]).cuda(), noise=nz, heads=False)
    with pytest.raises(KeyError):
        handle.forward_train(feats, None, timesteps=torch.tensor([0, 999]), noise=nz, heads=False)


# --------------------------------------------------------------------------- the other forms, B = 3
_FORM_RUNS = {}


def _form_run(form, handle, seeded_sd, scenes, tmp_path, monkeypatch):
    """B = 3 in the form: default on the sweep's handle, the others on a fresh handle each. Cached."""
    if form in _FORM_RUNS:
        return _FORM_RUNS[form]
    idx, dev = _batch(scenes, T.FORM_BATCH)
    chunks = [(0, T.FORM_BATCH)]
    m = handle if form == "default" else _make_handle(seeded_sd, form)
    try:
        if form == "default":
            m.set_gemm_mode("f16x3")
        m.numerics_flags(clear=True)
        out1 = _call(m, dev)
        out = _call(m, dev)
        parts = _parts(m, T.FORM_BATCH)
        torch.cuda.synchronize()
        r = {"flags": m.numerics_flags(), "unequal": _unequal(out1, out), "out": out, "parts": parts}
        if form != "default":
            # which path ran: buffers only that path allocates (test_decoder_edges_gpu._run)
            r["route"] = {"query_groups": _has_tap(m, "mk_cls_x"), "megakernel": _has_tap(m, "value_cnt_s0l0"),
                          "unfused_chain": _has_tap(m, "dr1"), "dense_value": _has_tap(m, "value_l0")}
        r["groups"] = U.groups_of(_profiled(m, dev, chunks, tmp_path, monkeypatch)[1], "decoder")
    finally:
        if form != "default":
            m.close()
    _FORM_RUNS[form] = r
    return r


@pytest.mark.parametrize("form", ["groups1", "groups2", "unfused", "fp32"])
def test_training_in_the_other_forms(handle, seeded_sd, scenes, truth, cfg, tmp_path, monkeypatch, form):
    """forward_train at B = 3 with one and two query groups per scene, on the unfused chain (whose LayerNorm takes the
    per-scene film_div path, here in f16x3) and in gemm mode fp32: the form asked for is the one that ran, no flag,
    the replay bit-equal to the first call, and the checks of _check at the same bars."""
    r = _form_run(form, handle, seeded_sd, scenes, tmp_path, monkeypatch)
    mk, groups = form in MEGAKERNEL_FORMS, form in ("default", "groups2")
    assert r["route"] == {"query_groups": groups, "megakernel": mk, "unfused_chain": not mk,
                          "dense_value": form == "fp32"}, r["route"]
    assert r["groups"] == ([int(form[-1])] if mk else []), r["groups"]
    assert r["flags"] == 0 and not r["unequal"], (r["flags"], r["unequal"])
    idx = U.replica_index(T.FORM_BATCH)
    _check(r["out"], r["parts"], idx, [(0, T.FORM_BATCH)], truth, scenes[0]["target"][idx],
           seeded_sd["_trajectory_head.plan_anchor"], cfg, f"B={T.FORM_BATCH} {form}")


def test_training_query_groups_are_bit_equal(handle, seeded_sd, scenes, tmp_path, monkeypatch):
    """1, 2 and the default 4 query groups per scene at B = 3: reg, cls, trajectory, the per-scene partials and the
    losses to the bit."""
    runs = {f: _form_run(f, handle, seeded_sd, scenes, tmp_path, monkeypatch) for f in MEGAKERNEL_FORMS}
    assert runs["default"]["groups"] == [4] and runs["default"]["flags"] == 0
    for f in ("groups2", "default"):
        assert not _unequal(runs[f]["out"], runs["groups1"]["out"]), (f, _unequal(runs[f]["out"], runs["groups1"]["out"]))
        for a, b in zip(runs[f]["parts"], runs["groups1"]["parts"]):
            assert torch.equal(_bits(a), _bits(b)), f


# --------------------------------------------------------------------------- doctored weights, B = 2
@pytest.fixture(scope="module")
def case_features(seeded_sd):
    """The float64 oracle before the trajectory head on the doctored cases' batch (the cases edit the head only)."""
    return T.oracle_features(seeded_sd, T.make_train_case(seeded_sd, "clamp_noise")[1])


@pytest.mark.parametrize("form", ["default", "groups1"])
@pytest.mark.parametrize("case", T.TRAIN_CASES)
def test_loss_kernel_edges_on_doctored_weights(gpu, seeded_sd, case_features, cfg, case, form):
    """A doctored training case (train_sweep_util.make_train_case; timesteps (49, 0)) on a fresh handle of the form
    against the float64 oracle on the same dict: no flag, the replay bit-equal, the checks of _check (outputs at the
    parity bars, every loss finite and at the loss bars), and the case's exact conditions:

      equal_modes    all 20 anchor distances tie: every mode's reg and cls row is bit-equal, the trajectory is mode 0's
      tied_anchors   the distances tie while the rows differ: the loss bars hold only with the first minimum, mode 0,
                     as the class target (torch.argmin)
      clamp_noise    scene 1's noised anchors clamp to the range corners under its own coefficients
      saturated_cls  every logit beyond +-58: (1 - sigmoid) underflows in the focal term
    """
    sd, inp, t, tg = T.make_train_case(seeded_sd, case)
    ref = T.oracle_train(sd, inp, t, tg, features=case_features)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(inp, timesteps=t, target=tg).items()}
    m = _make_handle(sd, form)
    try:
        m.numerics_flags(clear=True)
        out1 = _call(m, dev)
        out = _call(m, dev)
        parts = _parts(m, 2)
        torch.cuda.synchronize()
        flags = m.numerics_flags()
        has_groups = _has_tap(m, "mk_cls_x")
    finally:
        m.close()
    assert has_groups == (form == "default") and flags == 0, (has_groups, flags)
    assert not _unequal(out1, out), _unequal(out1, out)
    _, host = _check(out, parts, np.arange(2), [(0, 2)], ref, tg, sd["_trajectory_head.plan_anchor"], cfg,
                     f"{case} {form}")
    if case == "equal_modes":
        for k in OUT_KEYS[1:]:
            v = host[k].view(np.int32)
            bad = np.argwhere((v != v[:, :1]).reshape(2, T.Q, -1).any(-1))
            assert bad.size == 0, (k, bad.tolist())
        assert np.array_equal(host["trajectory"].view(np.int32), host["reg_l1"][:, 0].view(np.int32))
    if case.startswith("saturated_cls"):
        sign = 1.0 if case.endswith("pos") else -1.0
        assert (sign * host["cls_l0"] > 58.0).all() and (sign * host["cls_l1"] > 58.0).all()
