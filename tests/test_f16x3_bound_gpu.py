"""The f16x3 kernels held to a per-element bound under uneven channel scales, and the whole forward on state dicts
rescaled channel by channel ("Uneven channel scales").

Part 1, per kernel family: every output element against float64 with

    |out - ref64| <= rho D + 2^-25 sum_k |w_k| [|a_k| < 2^-2],     D = sum_k |a_k| |w_k| + |bias| + |res|

(f16x3_emul.py: the documented arithmetic on the CPU, the metric, and how rho is measured - from the emulation and plain
fp32 on the same inputs, never from the device; rho <= 1e-6 is a condition). The families (f16x3_cases.py) are the op
tests' uniform inputs, output rows scaled by 2^-20 .. 2^10 (the per-row weight scale and its index in every epilogue,
small channels the max-norm bar of test_ops_gpu.close() cannot see) and input channels scaled down by up to 2^6 / 2^12
with the weights compensated (subnormal activation lo parts: a kernel that flushes them or loses a lo image is 8 - 79
times over the bound, the documented arithmetic stays under it), and output rows over the whole of fp32 (rowrange:
2^-140 .. 2^110, a zero row and the rows either side of the split's threshold 2^-113, with a flush allowance FLOOR
added to the bound; see test_weight_range.py). The CPU companion test_f16x3_bound.py shows that the
emulation meets the bound on every case and that four mutants of it do not.

Part 2: fresh handles on rescale_util's dicts (hidden channels of every BasicBlock and ReLU MLP scaled by 2^-U{0..SPREAD},
through the weights, through running_var, and with negative near-zero bn2 scales), B = 2 and B = 33, f16x3 and fp32,
every output and tap against the float64 oracle on the same dict at the unchanged bars.

Measured on the MI355X: see the table in DESIGN.md section 5.
"""
import numpy as np
import pytest
import torch

import batch_sweep_util as U
import f16x3_cases as C
import f16x3_emul as E
import rescale_util as R
from test_batch_sweep_gpu import BARS, _check_batch, _run, _unequal
from test_ops_gpu import DEV, g, ok
from test_parity_gpu import WAYPOINT_L2_TOL, _report

pytestmark = pytest.mark.gpu


def _note(tag, case, ratio):
    line = (f"== f16x3 bound {tag}: rho {case.rho:.3e} (emulation {case.rho_emul:.2e}, fp32 {case.rho_fp32:.2e}) "
            f"gpu ratio {ratio:.3f}")
    print(line)
    _report([line])


# --------------------------------------------------------------------------- part 1: the kernels
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name,shape,env,route", C.CONV_CASES, ids=[c[0] for c in C.CONV_CASES])
def test_conv_bound(gpu, monkeypatch, name, shape, env, route, family):
    B, H, W, Cin, Cout, k, s, p, relu, res = shape
    case = C.conv_case(shape, family)
    assert case.rho <= E.RHO_MAX, case.rho
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    Ho, Wo = E.out_hw(H, W, k, s, p)
    out = torch.full((B, Ho, Wo, Cout), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, win, bin_ = g(case.x.permute(0, 2, 3, 1)), g(case.w.permute(0, 2, 3, 1)), g(case.b)
    rin = g(case.r.permute(0, 2, 3, 1)) if res else None
    ok(gpu.dd_op_conv2d_x3(xin.data_ptr(), B, H, W, Cin, win.data_ptr(), bin_.data_ptr(),
                           rin.data_ptr() if res else None, out.data_ptr(), Cout, k, k, s, p, int(relu), 0,
                           flags.data_ptr(), None), gpu)
    assert gpu.dd_op_last_kernel().decode() == route
    assert int(flags.item()) == 0
    got = out.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    ratio = case.ratio(got)
    _note(f"{name} {family}", case, ratio)
    assert ratio <= 1.0, (name, family, ratio)


@pytest.mark.parametrize("family", C.STEM_FAMILIES)
@pytest.mark.parametrize("B,H,W", C.STEM_NHWC)
def test_stem_pool_bound(gpu, B, H, W, family):
    """The fused stem on NHWC4 pixels: the bound of the 7 x 7 conv carried through ReLU and the 3 x 3 max."""
    case = C.stem_case(B, 4, H, W, family)
    assert case.rho <= E.RHO_MAX, case.rho
    Hp, Wp = E.out_hw(*E.out_hw(H, W, 7, 2, 3), 3, 2, 1)
    out = torch.full((B, Hp, Wp, 64), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, win, bin_ = g(case.x_in.permute(0, 2, 3, 1)), g(case.w4.permute(0, 2, 3, 1)), g(case.b)
    ok(gpu.dd_op_stem_pool_x3(xin.data_ptr(), B, H, W, win.data_ptr(), bin_.data_ptr(), out.data_ptr(),
                              flags.data_ptr(), None), gpu)
    assert gpu.dd_op_last_kernel().decode() == "stem_pool<f16x3>"
    assert int(flags.item()) == 0
    got = out.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    ratio = case.pooled_ratio(got)
    _note(f"stem NHWC4 {(B, H, W)} {family}", case, ratio)
    assert ratio <= 1.0, (family, ratio)


@pytest.mark.parametrize("family", C.STEM_FAMILIES)
@pytest.mark.parametrize("B,Cc,H,W", C.STEM_NCHW)
def test_stem_pool_nchw_bound(gpu, monkeypatch, B, Cc, H, W, family):
    """The fused stem reading the caller's NCHW tensor in place (C = 1 and 3), default form."""
    monkeypatch.setenv("DDMI_STEM1", "0")
    case = C.stem_case(B, Cc, H, W, family)
    assert case.rho <= E.RHO_MAX, case.rho
    Hp, Wp = E.out_hw(*E.out_hw(H, W, 7, 2, 3), 3, 2, 1)
    out = torch.full((B, Hp, Wp, 64), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, win, bin_ = g(case.x_in), g(case.w4.permute(0, 2, 3, 1)), g(case.b)
    ok(gpu.dd_op_stem_pool_nchw(xin.data_ptr(), B, Cc, H, W, win.data_ptr(), bin_.data_ptr(), out.data_ptr(), 0,
                                flags.data_ptr(), None), gpu)
    assert gpu.dd_op_last_kernel().decode() == "stem_pool<f16x3>"
    assert int(flags.item()) == 0
    got = out.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    ratio = case.pooled_ratio(got)
    _note(f"stem NCHW {(B, Cc, H, W)} {family}", case, ratio)
    assert ratio <= 1.0, (family, ratio)


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("K,N", C.MK_CASES)
def test_mk_linear_bound(gpu, K, N, family):
    """The megakernels' GEMM core, whose weights pack_mk_weights scales and packs with a table of its own (the op has no
    flag word and no route string)."""
    case = C.mk_case(K, N, family)
    assert case.rho <= E.RHO_MAX, case.rho
    out = torch.full((32, N), float("nan"), device=DEV)
    ad, wd, bd = g(case.x), g(case.w), g(case.b)
    ok(gpu.dd_op_mk_linear(ad.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), N, None), gpu)
    got = out.cpu()
    assert torch.isfinite(got).all()
    ratio = case.ratio(got)
    _note(f"mk_linear {(K, N)} {family}", case, ratio)
    assert ratio <= 1.0, (family, ratio)


# --------------------------------------------------------------------------- part 2: the forward on rescaled dicts
INPUT_SEED = 7


@pytest.fixture(scope="module")
def scenes(gpu):
    """B = 2: synthetic_inputs(2, 7); B = 33: the sweep's five distinct scenes repeated."""
    from diffusiondrive_amd.weights import synthetic_inputs
    two = synthetic_inputs(2, INPUT_SEED)
    five = synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED)
    return two, five


@pytest.fixture(scope="module")
def dicts(seeded_sd):
    return {name: make(seeded_sd) for name, make in R.VARIANTS.items()}


@pytest.fixture(scope="module")
def truths(dicts, scenes):
    """The float64 oracle on each dict, for both sets of scenes; computed on first use, then shared."""
    cache = {}

    def get(name, which):
        if (name, which) not in cache:
            cache[(name, which)] = U.oracle_run(dicts[name], scenes[which])
        return cache[(name, which)]
    return get


@pytest.fixture(scope="module")
def record():
    rec = {}
    yield rec
    lines = [f"== rescaled forward summary, {grp}: " + " ".join(f"{k} {v:.3e}" for k, v in sorted(e.items()))
             for grp, e in rec.items()]
    if lines:
        _report(lines)


def _forward_checks(m, mode, dev, idx, chunks, ref, tag, record):
    m.set_gemm_mode(mode)
    m.numerics_flags(clear=True)
    last_n = chunks[-1][1]
    out1, taps1 = _run(m, dev, last_n)
    out2, taps2 = _run(m, dev, last_n)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    assert not _unequal(out1, out2) and not _unequal(taps1, taps2), (_unequal(out1, out2), _unequal(taps1, taps2))
    _check_batch(out2, taps2, idx, chunks, ref, tag, record, tag.split(" B=")[0])
    return out2


@pytest.mark.parametrize("B", [2, 33])
@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_forward_on_rescaled_dict(gpu, dicts, scenes, truths, record, variant, mode, B):
    """A fresh handle on the dict, B = 2 (synthetic_inputs(2, 7)) or B = 33 (five scenes repeated), f16x3 or fp32: first call = replay to the bit, no flag, every
    output and tap within the unchanged bars of the float64 oracle on the same dict, replicas bit-equal.

    Measured on the MI355X, f16x3 at B = 2 / 33: waypoint L2 1.0e-5 / 1.2e-5 (rescaled), 8.8e-6 / 1.5e-5 (rescaled_var),
    1.2e-5 / 1.2e-5 (rescaled_signed); query_out, the largest tap, 4.0e-6 / 4.9e-6, 4.1e-6 / 4.7e-6, 3.5e-6 / 4.7e-6;
    fp32 the same class.

    What the B = 33 cases found: with P.V of the tf-decoder megakernel on unscaled probabilities, rescaled_var read
    query_out 7.3e-5 (bar 2e-5; agent_states 3.2e-3, bar 2e-3) and rescaled_signed 2.04e-5 - one decoded query row 2.7e-4 /
    7.7e-5 absolute off, the unfused chain on the same keyval bits inside, the function well conditioned there
    (test_f16x3_bound.py). Against the unfused chain over 320 scenes the one-workgroup kernel had 4 of 9920 query rows
    more than 4e-5 off on the seeded dict as well (largest 1.24e-4); a six-product P.V and nine-product scores changed
    nothing, the probabilities split as P * 2^12 (tfdec_mk.hip, attn_pv_t) left none above 7.2e-6 (1.3e-5 on
    rescaled_var): small probabilities' fp16 parts are subnormal, the subnormal-lo regime of DESIGN.md section 5 at a
    site where the other operand is large."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=dicts[variant], device=0, gemm="f16x3")
    try:
        which = 0 if B == 2 else 1
        idx = np.arange(2) if B == 2 else U.replica_index(B)
        dev = {k: torch.from_numpy(np.ascontiguousarray(scenes[which][k][idx])).cuda() for k in U.INPUT_KEYS}
        _forward_checks(m, mode, dev, idx, U.chunk_ranges(B), truths(variant, which),
                        f"{variant}({R.SPREAD}) {mode} B={B}", record)
    finally:
        m.close()


def test_rescaling_preserves_the_trajectory(gpu, gpu_model, dicts, scenes):
    """The metamorphic relation itself, without the oracle: in fp32 mode the trajectories of rescaled(SPREAD) and of the
    seeded dict agree within the waypoint bar."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    dev = {k: torch.from_numpy(scenes[0][k]).cuda() for k in U.INPUT_KEYS}
    feats = {k: dev[k] for k in U.INPUT_KEYS[:3]}
    gpu_model.set_gemm_mode("fp32")
    try:
        base = gpu_model.forward(feats, noise=dev["noise"])["trajectory"].double().cpu().numpy()
    finally:
        gpu_model.set_gemm_mode("f16x3")
    m = DiffusionDriveModel(state_dict=dicts["rescaled"], device=0, gemm="fp32")
    try:
        got = m.forward(feats, noise=dev["noise"])["trajectory"].double().cpu().numpy()
        assert m.numerics_flags() == 0
    finally:
        m.close()
    d = (got[..., :2] - base[..., :2]).reshape(got.shape[0], -1)
    l2 = float(np.sqrt((d ** 2).sum(-1)).max())
    line = f"== rescaled({R.SPREAD}) vs seeded, fp32 mode, B=2: waypoint L2 {l2:.3e}"
    print(line)
    _report([line])
    assert l2 <= WAYPOINT_L2_TOL, l2
