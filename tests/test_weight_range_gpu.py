"""Dead and tiny weight rows on the device ("Dead and tiny rows"): what the kernels make of the
images test_weight_range.py holds to the emulation on the CPU.

Op level, f16x3: the ``rowrange`` family of f16x3_cases.py runs through test_f16x3_bound_gpu.py on every conv route, both
stems and mk_linear. Here: the fused bev_proj on rowrange rows, the uint8 stem on the same images as the float stem, and
bf16 (conv_x6, conv_x5, the stem), where the bf16 image is the one that overflowed.

Forward: fresh handles on rescale_util.dead_rows (BatchNorm gammas at 0, 2^-100, 2^-118, 2^-130 and -2^-120, running
variances at 0 and 1e6, rows of every Linear and plain conv scaled by 2^-118 and 2^-135 or zeroed, biases untouched) at
B = 2 and B = 33, f16x3 and fp32, every output and tap within the unchanged bars of the float64 oracle on the same dict;
bf16 at B = 2 under its own bar. With the split's exponent unbounded a dead row's channel was NaN in f16x3 and bf16 and
the next contraction spread it over the whole forward; fp32 mode never reads the images.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import batch_sweep_util as U
import f16x3_cases as C
import f16x3_emul as E
import rescale_util as R
from test_f16x3_bound_gpu import _forward_checks
from test_ops_gpu import DEV, close, g, ok, rnd
from test_parity_gpu import _bf16_bar, _report

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- op level
def test_bevproj_on_rowrange_rows(gpu):
    """bevproj.hip (pack_mk_weights' image of the 256 x 64 p3 columns) with rowrange rows, B = 1, against the float64
    decomposition of test_bevproj_fused at its bar. The normal rows' exponents stop at 0: the op ends in a LayerNorm
    over the 256 channels, whose variance squares them (2^110 squared is not an fp32 number in any implementation)."""
    B, H, W = 1, 64, 64
    cat = rnd(B * H * W, 320, seed=101)
    p3 = cat[:, 256:]
    kvp = rnd(B, 8, 8, 256, seed=102)
    w, bias, _ = C._row_range_apply(rnd(256, 64, seed=103, scale=1.0 / 8.0), rnd(256, seed=104), None, 107, emax=0)
    tiny = C.tiny_rows(256, 107)
    assert tiny[255] and tiny[31] and (w[tiny].abs().amax(1) < 2.0 ** -112).all() and (w[tiny] == 0).all(1).any()
    lg, lb = 1.0 + 0.1 * rnd(256, seed=105), rnd(256, seed=106)
    bil = F.interpolate(kvp.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    v = F.relu(p3.double() @ w.double().T + bias.double() + bil.permute(0, 2, 3, 1).reshape(-1, 256))
    ref = F.layer_norm(v, (256,), lg.double(), lb.double(), 1e-5)
    out = torch.full((B * H * W, 256), float("nan"), device=DEV)
    cd, kd, wd, bd, gd, ld = g(cat), g(kvp), g(w), g(bias), g(lg), g(lb)
    ok(gpu.dd_op_bevproj(cd.data_ptr() + 256 * 4, 320, kd.data_ptr(), wd.data_ptr(), bd.data_ptr(), gd.data_ptr(),
                         ld.data_ptr(), out.data_ptr(), B, H, W, 8, 8, None), gpu)
    assert bool(torch.isfinite(out).all())
    err = close(out, ref, 3e-5)
    _report([f"== weight range bevproj rowrange B=1: max err {err:.3e} (max |ref| {float(ref.abs().max()):.2f})"])


def test_u8_stem_reads_the_same_rowrange_images(gpu, monkeypatch):
    """dd_op_stem_pool_u8 on HWC bytes equals dd_op_stem_pool_nchw on the widened tensor bit for bit with rowrange
    rows in the stem's weights, and both are finite."""
    from diffusiondrive_amd import _lib
    monkeypatch.setenv("DDMI_STEM1", "0")
    B, Cc, H, W = 1, 3, 40, 72
    case = C.stem_case(B, Cc, H, W, "rowrange")
    gen = torch.Generator().manual_seed(261)
    x = torch.randint(0, 256, (B, H, W, Cc), generator=gen, dtype=torch.uint8)
    lut = torch.arange(256).float().div(255)
    wide = lut[x.long()].permute(0, 3, 1, 2).contiguous()
    Hp, Wp = E.out_hw(*E.out_hw(H, W, 7, 2, 3), 3, 2, 1)
    xd, fd, ld = x.to(DEV), wide.to(DEV), lut.to(DEV)
    wd, bd = g(case.w4.permute(0, 2, 3, 1)), g(case.b)
    out_u = torch.full((B, Hp, Wp, 64), float("nan"), device=DEV)
    out_f = torch.full((B, Hp, Wp, 64), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _lib.check(gpu.dd_op_stem_pool_nchw(fd.data_ptr(), B, Cc, H, W, wd.data_ptr(), bd.data_ptr(), out_f.data_ptr(), 0,
                                        flags.data_ptr(), None), gpu, op=True)
    _lib.check(gpu.dd_op_stem_pool_u8(xd.data_ptr(), 0, B, Cc, H, W, ld.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                      out_u.data_ptr(), 0, flags.data_ptr(), None), gpu, op=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_f).all()) and float(out_f.abs().max()) > 0
    assert torch.equal(out_u, out_f)
    assert int(flags.item()) == 0
    # and the float call is the truth's: the same weights on these pixels, per element
    wide_case = C.StemCase(wide, case.w, case.b, None, 2, 3, True, tiny=case.tiny)
    ratio = wide_case.pooled_ratio(out_f.cpu().permute(0, 3, 1, 2))
    _report([f"== weight range stem u8 rowrange {(B, Cc, H, W)}: rho {wide_case.rho:.3e} gpu ratio {ratio:.3f}"])
    assert wide_case.rho <= E.RHO_MAX and ratio <= 1.0, (wide_case.rho, ratio)


def _bf16_truth(case):
    """The float64 conv on bf16-rounded operands, as test_conv2d_bf16 takes it: activations rounded to bf16, weights
    the bf16 image of w s scaled back by 1 / s (s the split's, a power of two), bias and residual in fp32; ReLU."""
    _, _, sinv = E.split_weights(E.weight_rows(case.w))
    s = (1.0 / sinv.double()).view(-1, 1, 1, 1)
    wb = (case.w.double() * s).float().bfloat16().double() / s
    ref = F.conv2d(case.x.bfloat16().double(), wb, case.b.double(), case.stride, case.padding)
    if case.r is not None:
        ref = ref + case.r.double()
    return F.relu(ref) if case.relu else ref


def _per_channel_ok(tag, got, ref, floor, tol=1e-4):
    """|got - ref| <= tol x the channel's max |ref| + floor on every element, channels on axis 1 (test_conv2d_bf16's
    1e-4, taken per output channel: a 2^110 row would own a bar on the tensor's maximum)."""
    assert bool(torch.isfinite(got).all()), tag
    err = (got.double() - ref).abs().amax((0, 2, 3))
    lim = tol * ref.abs().amax((0, 2, 3)) + floor
    worst = float((err / lim.clamp_min(torch.finfo(torch.float64).tiny)).max())
    _report([f"== weight range bf16 {tag}: worst channel err / (1e-4 max|ref_c| + FLOOR) {worst:.3f}"])
    assert (err <= lim).all(), (tag, worst, int((err / lim.clamp_min(1e-300)).argmax()))


# x6-8x32-res and x5-256x64-3x3: in bf16 the 1 x 1 / stride 2 x5 case of the f16x3 list goes to conv_x3
BF16_CONVS = [(C.CONV_CASES[2], "conv_x6<"), (C.CONV_CASES[9], "conv_x5<")]


@pytest.mark.parametrize("entry,kernel", BF16_CONVS, ids=[e[0][0] for e in BF16_CONVS])
def test_conv_bf16_on_rowrange(gpu, monkeypatch, entry, kernel):
    name, shape, env, _ = entry
    B, H, W, Cin, Cout, k, s, p, relu, res = shape
    case = C.conv_case(shape, "rowrange")
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    Ho, Wo = E.out_hw(H, W, k, s, p)
    out = torch.full((B, Ho, Wo, Cout), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, win, bin_ = g(case.x.permute(0, 2, 3, 1)), g(case.w.permute(0, 2, 3, 1)), g(case.b)
    rin = g(case.r.permute(0, 2, 3, 1)) if res else None
    ok(gpu.dd_op_conv2d_x3(xin.data_ptr(), B, H, W, Cin, win.data_ptr(), bin_.data_ptr(),
                           rin.data_ptr() if res else None, out.data_ptr(), Cout, k, k, s, p, int(relu), 1,
                           flags.data_ptr(), None), gpu)
    route = gpu.dd_op_last_kernel().decode()
    assert route.startswith(kernel) and route.endswith("bf16>"), route
    assert int(flags.item()) == 0
    _per_channel_ok(f"{name} {route}", out.cpu().permute(0, 3, 1, 2), _bf16_truth(case), case.floor)


def test_stem_bf16_on_rowrange(gpu):
    B, H, W = C.STEM_NHWC[1]
    case = C.stem_case(B, 4, H, W, "rowrange")
    Hp, Wp = E.out_hw(*E.out_hw(H, W, 7, 2, 3), 3, 2, 1)
    out = torch.full((B, Hp, Wp, 64), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, win, bin_ = g(case.x_in.permute(0, 2, 3, 1)), g(case.w4.permute(0, 2, 3, 1)), g(case.b)
    ok(gpu.dd_op_stem_pool(xin.data_ptr(), B, H, W, win.data_ptr(), bin_.data_ptr(), out.data_ptr(), 1,
                           flags.data_ptr(), None), gpu)
    assert gpu.dd_op_last_kernel().decode() == "stem_pool<bf16>"
    assert int(flags.item()) == 0
    _per_channel_ok(f"stem NHWC4 {(B, H, W)}", out.cpu().permute(0, 3, 1, 2),
                    F.max_pool2d(_bf16_truth(case), 3, 2, 1), case.floor)


# --------------------------------------------------------------------------- the forward on dead_rows
INPUT_SEED = 7


@pytest.fixture(scope="module")
def scenes(gpu):
    from diffusiondrive_amd.weights import synthetic_inputs
    return synthetic_inputs(2, INPUT_SEED), synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED)


@pytest.fixture(scope="module")
def dead(seeded_sd):
    return R.dead_rows(seeded_sd)[0]


@pytest.fixture(scope="module")
def truths(dead, scenes):
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = U.oracle_run(dead, scenes[which])
        return cache[which]
    return get


@pytest.fixture(scope="module")
def record():
    rec = {}
    yield rec
    lines = [f"== dead_rows forward summary, {grp}: " + " ".join(f"{k} {v:.3e}" for k, v in sorted(e.items()))
             for grp, e in rec.items()]
    if lines:
        _report(lines)


@pytest.mark.parametrize("B", [2, 33])
@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
def test_forward_on_dead_rows(gpu, dead, scenes, truths, record, mode, B):
    """A fresh handle on dead_rows: B = 2 (four query groups, gpt_tail, four tfdec workgroups) and B = 33 (five scenes
    repeated): first call = replay to the bit, no numerics flag, replicas bit-equal, every output, every per-(step,
    layer) reg / cls / gs and the dense taps within the unchanged bars of the float64 oracle on the same dict. fp32
    mode is the control: it reads no split image."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=dead, device=0, gemm="f16x3")
    try:
        which = 0 if B == 2 else 1
        idx = np.arange(2) if B == 2 else U.replica_index(B)
        dev = {k: torch.from_numpy(np.ascontiguousarray(scenes[which][k][idx])).cuda() for k in U.INPUT_KEYS}
        out = _forward_checks(m, mode, dev, idx, U.chunk_ranges(B), truths(which), f"dead_rows {mode} B={B}", record)
        for k, v in out.items():
            assert bool(torch.isfinite(v).all()), k
    finally:
        m.close()


def test_forward_bf16_on_dead_rows(gpu, dead, scenes):
    """bf16 mode at B = 2 on dead_rows, held to the bf16 bar of test_parity_gpu (the pre-argmax tensors against the
    fp32 oracle on the same dict, no worse than the reference path's own bf16 autocast)."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    from oracle.model import OracleModel
    inp = scenes[0]
    args = tuple(inp[k] for k in U.INPUT_KEYS)
    feats = {k: torch.from_numpy(inp[k]) for k in U.INPUT_KEYS[:3]}
    m = DiffusionDriveModel(state_dict=dead, device=0, gemm="f16x3")
    try:
        m.set_gemm_mode("bf16")
        m.numerics_flags(clear=True)
        out = m.forward(feats, noise=torch.from_numpy(inp["noise"]), modes=True)
        assert m.numerics_flags() == 0
    finally:
        m.close()
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    _bf16_bar(out, OracleModel(dead), args, 2, "dead_rows bf16 B=2")
