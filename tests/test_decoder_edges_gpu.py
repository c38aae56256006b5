"""Edge cases of the trajectory-head kernels (decoder_mk / value_proj / the unfused decoder glue / the fp32 dense
path) and of the f16x3 overflow flag, driven through whole-model forwards on doctored weights with the CPU oracle
(the same dict, the same noise) beside them. tests/decoder_edge_util.py holds the cases, tests/test_decoder_edges.py
shows their premises on the oracle without a GPU.

"A" cases (no flag may be raised), each in four forms - f16x3 default (4 query groups at B = 2), DDMI_MK_GROUPS=1,
DDMI_DECODER_MK=0 (the unfused chain) and gemm mode fp32 (dense value map) - and equal_modes also with 2 groups:

  clamp_noise   the clamp of the DDIM start / trajectory embedding, points at the range's corners, duplicate taps,
                live and zero-padded taps within a scene
  offmap_l1     every layer-1 tap zero-padded: dedup count 0, a value_proj launch without a live row, gs == 0
  tied_cls      an exact 20-way cls tie: the first maximal mode (torch.argmax), also where the last query group to
                arrive reads the logits back
  equal_modes   identical inputs in every mode's row: a row's arithmetic must not depend on its place in the 32-row
                MFMA tile or on its query group

Every per-(step, layer) reg / cls / gs tap and the trajectory are held to the oracle at the bars of
tests/test_parity_gpu.py (MODE_TOL absolute on reg / cls, MODE_TOL relative to the tensor's scale on gs,
WAYPOINT_L2_TOL on the trajectory); the megakernel forms also pass the dedup invariants of every (step, layer).

"B" cases: one weight edit per f16x3 site puts that site's input beyond the fp16 range; the forward must raise
DD_NUM_F16_OVERFLOW_BIT (and nothing else), and forward(safe=True) must return the fp32 path's result.
"""
import os

import numpy as np
import pytest
import torch

from decoder_edge_util import (BATCH, CASES, OVERFLOW_SITES, check_gathered_taps, make_case, make_overflow_sd)
from golden_util import waypoint_l2
from test_parity_gpu import MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL, _report

pytestmark = pytest.mark.gpu

B, Q, P = BATCH, 20, 8
CAP = Q * P * 4
SL = [(s, l) for s in range(2) for l in range(2)]
F16_OVERFLOW_BIT = 1  # DD_NUM_F16_OVERFLOW_BIT (include/ddmi.h)

# form -> (gemm mode, environment read at dd_create)
FORMS = {
    "default": ("f16x3", {}),
    "groups1": ("f16x3", {"DDMI_MK_GROUPS": "1"}),
    "groups2": ("f16x3", {"DDMI_MK_GROUPS": "2"}),
    "unfused": ("f16x3", {"DDMI_DECODER_MK": "0"}),
    "fp32": ("fp32", {}),
}
MEGAKERNEL_FORMS = ("default", "groups1", "groups2")
A_PARAMS = [(c, f) for c in CASES for f in ("default", "groups1", "unfused", "fp32")] + [("equal_modes", "groups2")]

_ORACLE, _RUNS = {}, {}


def _oracle(seeded_sd, case):
    """One fp32 oracle forward per case (taps included), shared by the case's forms."""
    if case not in _ORACLE:
        from oracle.model import OracleModel, Taps
        sd, inp = make_case(seeded_sd, case)
        taps = Taps()
        out = OracleModel(sd).forward(inp["camera_feature"], inp["lidar_feature"], inp["status_feature"],
                                      inp["noise"], taps=taps, heads=False)
        ref = {k: v.numpy() for k, v in taps.items() if k[:3] in ("reg", "cls", "gs_")}
        ref["trajectory"] = out["trajectory"].numpy()
        _ORACLE[case] = ref
    return _ORACLE[case]


def _has_tap(m, name):
    from diffusiondrive_amd._lib import DDMIError
    try:
        m.tap(name)
        return True
    except DDMIError:
        return False


def _ints(m, name, n):
    return m.tap(name)[:n].view(torch.int32).cpu().numpy().copy()


def _run(seeded_sd, case, form):
    """The case on a fresh handle of the form (the knobs are read at dd_create): one forward, its taps, and in the
    megakernel forms one steps = 1 forward (the first step's points) and one fp32 forward (the dense value maps) on
    the same handle. Cached: the cross-form comparison of equal_modes reuses the forms' runs."""
    if (case, form) in _RUNS:
        return _RUNS[(case, form)]
    from diffusiondrive_amd.model import DiffusionDriveModel
    mode, env = FORMS[form]
    sd, inp = make_case(seeded_sd, case)
    feats = {k: torch.from_numpy(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}
    nz = torch.from_numpy(inp["noise"])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = DiffusionDriveModel(state_dict=sd, device=0, gemm=mode)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        m.numerics_flags(clear=True)
        r = {"trajectory": m.forward(feats, noise=nz)["trajectory"].numpy().copy()}
        r["flags"] = m.numerics_flags(clear=True)
        for s, l in SL:
            r[f"reg_s{s}l{l}"] = m.tap(f"reg_s{s}l{l}", (B, Q, P, 3)).cpu().numpy().copy()
            r[f"cls_s{s}l{l}"] = m.tap(f"cls_s{s}l{l}", (B, Q)).cpu().numpy().copy()
            r[f"gs_s{s}l{l}"] = m.tap(f"gs_s{s}l{l}", (B, Q, 256)).cpu().numpy().copy()
        r["mode_idx"] = _ints(m, "mode_idx", B)
        r["pts"] = m.tap("pts", (B, Q, P, 2)).cpu().numpy().copy()
        r["pts_next"] = m.tap("pts_next", (B, Q, P, 2)).cpu().numpy().copy()
        # which path ran: buffers only that path allocates (there is no route string for the trajectory head)
        r["route"] = {"query_groups": _has_tap(m, "mk_cls_x"), "megakernel": _has_tap(m, "value_cnt_s0l0"),
                      "unfused_chain": _has_tap(m, "dr1"), "dense_value": _has_tap(m, "value_l0")}
        if mode == "f16x3":
            for s, l in SL:
                r[f"value_taps_s{s}l{l}"] = _ints(m, f"value_taps_s{s}l{l}", B * CAP)
        if form in MEGAKERNEL_FORMS:
            for s, l in SL:
                r[f"value_slots_s{s}l{l}"] = _ints(m, f"value_slots_s{s}l{l}", B * CAP)
                r[f"value_cnt_s{s}l{l}"] = _ints(m, f"value_cnt_s{s}l{l}", B)
                r[f"value_rows_s{s}l{l}"] = m.tap(f"value_rows_s{s}l{l}", (B * CAP, 256)).cpu().numpy().copy()
            m.forward(feats, noise=nz, steps=1)
            r["pts_s0"] = m.tap("pts", (B, Q, P, 2)).cpu().numpy().copy()
            r["value_taps_s0l0_steps1"] = _ints(m, "value_taps_s0l0", B * CAP)
            m.set_gemm_mode("fp32")
            m.forward(feats, noise=nz)
            for l in range(2):
                r[f"dense_l{l}"] = m.tap(f"value_l{l}", (B * 64 * 64, 256)).cpu().numpy().copy()
            r["flags_after"] = m.numerics_flags(clear=True)
    finally:
        m.close()
    _RUNS[(case, form)] = r
    return r


@pytest.mark.parametrize("case,form", A_PARAMS, ids=[f"{c}-{f}" for c, f in A_PARAMS])
def test_doctored_case_matches_oracle(gpu, seeded_sd, case, form):
    """The case in the form: no flag, every reg / cls / gs tap and the trajectory within the parity bars of the
    oracle, the case's exact conditions on the GPU's own output, and (megakernel forms) the dedup invariants of all
    four (step, layer) tap sets with the points taken from the GPU's own taps. One line per (case, form) with every
    tap's max error goes to the parity report (test_parity_gpu._report). Measured on the MI355X (first run, all
    forms): the largest reg / cls / gs error 2.6e-5 (clamp_noise, fp32 form, reg_s1l0; the f16x3 forms 2.1e-5) and
    the largest trajectory L2 2.0e-5 against bars of 1e-4; gs_s0l1 / gs_s1l1 of offmap_l1 and the tied logits
    exactly 0 from the oracle."""
    ref = _oracle(seeded_sd, case)
    r = _run(seeded_sd, case, form)
    errs = {}
    for s, l in SL:
        for k in ("reg", "cls", "gs"):
            n = f"{k}_s{s}l{l}"
            errs[n] = float(np.abs(r[n].astype(np.float64) - ref[n]).max())
    l2 = waypoint_l2(r["trajectory"], ref["trajectory"])
    _report([f"== edges {case} {form}: flags {r['flags']} trajectory L2 {l2:.3e} "
             + " ".join(f"{k} {v:.3e}" for k, v in errs.items())])

    # the form that was asked for is the one that ran
    mk, groups = form in MEGAKERNEL_FORMS, form in ("default", "groups2")
    assert r["route"] == {"query_groups": groups, "megakernel": mk, "unfused_chain": not mk,
                          "dense_value": form == "fp32"}, r["route"]
    assert r["flags"] == 0
    for n, e in errs.items():
        bar = MODE_TOL * (max(1.0, float(np.abs(ref[n]).max())) if n.startswith("gs") else 1.0)
        assert e <= bar, (n, e, bar)
    assert l2 <= WAYPOINT_L2_TOL, l2

    if case == "offmap_l1":
        for s in range(2):
            assert not r[f"gs_s{s}l1"].any(), s
            if FORMS[form][0] == "f16x3":
                assert (r[f"value_taps_s{s}l1"] == -1).all(), s
            if mk:
                assert (r[f"value_cnt_s{s}l1"] == 0).all(), (s, r[f"value_cnt_s{s}l1"])
    if case == "tied_cls":
        cls = r["cls_s1l1"]
        assert (cls.view(np.int32) == cls.view(np.int32)[:, :1]).all(), cls
        assert (r["mode_idx"] == 0).all(), r["mode_idx"]
        assert np.array_equal(r["trajectory"], r["reg_s1l1"][:, 0])
    if case == "equal_modes":
        for s, l in SL:
            for k in ("reg", "cls", "gs"):
                v = r[f"{k}_s{s}l{l}"].view(np.int32)
                bad = np.argwhere((v != v[:, :1]).reshape(B, Q, -1).any(-1))
                assert bad.size == 0, (f"{k}_s{s}l{l}", bad.tolist())
        assert (r["mode_idx"] == 0).all(), r["mode_idx"]

    if mk:
        assert r["flags_after"] == 0
        assert np.array_equal(r["pts_next"], r["reg_s1l0"][..., :2])  # layer 1's points are layer 0's regression
        assert np.array_equal(r["value_taps_s0l0_steps1"], r["value_taps_s0l0"])  # same first step in the steps=1 run
        points = {(0, 0): r["pts_s0"], (0, 1): r["reg_s0l0"][..., :2], (1, 0): r["pts"], (1, 1): r["pts_next"]}
        seen = {}
        for s, l in SL:
            sf = f"_s{s}l{l}"
            seen[(s, l)] = check_gathered_taps(points[(s, l)], r["value_taps" + sf], r["value_slots" + sf],
                                               r["value_cnt" + sf], r["value_rows" + sf].astype(np.float64),
                                               r[f"dense_l{l}"].astype(np.float64), B, TAP_TOL)
        if case == "clamp_noise":  # the helper saw zero-padded and live taps (the start points: scene 1's corners)
            assert seen[(0, 0)][0] > 0 and seen[(0, 0)][1] > 0, seen
        if case == "offmap_l1":
            assert seen[(0, 1)][1] == 0 and seen[(1, 1)][1] == 0, seen


def test_equal_modes_query_groups_are_bit_equal(gpu, seeded_sd):
    """equal_modes through 1, 2 and 4 query groups per scene: the same taps and trajectory to the bit."""
    runs = {f: _run(seeded_sd, "equal_modes", f) for f in MEGAKERNEL_FORMS}
    names = ["trajectory", "mode_idx"] + [f"{k}_s{s}l{l}" for k in ("reg", "cls", "gs") for s, l in SL]
    for f in ("groups2", "default"):
        for n in names:
            assert np.array_equal(runs[f][n].view(np.int32), runs["groups1"][n].view(np.int32)), (f, n)


@pytest.mark.parametrize("site", sorted(OVERFLOW_SITES))
def test_overflow_is_never_silent(gpu, seeded_sd, site):
    """One weight edit puts the input of one f16x3 site beyond the fp16 range (test_decoder_edges.py shows it on the
    oracle): the f16x3 forward raises DD_NUM_F16_OVERFLOW_BIT and no other bit, forward(safe=True) returns what the
    same handle's fp32 forward returns, to the bit, and leaves the flags clear."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(B, 7)
    feats = {k: torch.from_numpy(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}
    nz = torch.from_numpy(inp["noise"])
    m = DiffusionDriveModel(state_dict=make_overflow_sd(seeded_sd, site), device=0, gemm="f16x3")
    try:
        m.numerics_flags(clear=True)
        m.forward(feats, noise=nz)
        flags = m.numerics_flags(clear=True)
        _report([f"== edges overflow at {site}: f16x3 flags {flags:#x}"])
        assert flags == F16_OVERFLOW_BIT, (site, flags)
        with pytest.warns(UserWarning, match="re-running the forward in fp32"):
            safe = m.forward(feats, noise=nz, safe=True)
        assert m.numerics_flags(clear=False) == 0
        m.set_gemm_mode("fp32")
        ref = m.forward(feats, noise=nz)
        assert m.numerics_flags(clear=True) == 0
        assert set(safe) == set(ref)
        for k in ref:
            assert torch.equal(safe[k], ref[k]), (site, k)
    finally:
        m.close()
