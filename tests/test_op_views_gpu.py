"""The conv / GEMM family, LayerNorm and the bilinear resize on the operand forms the forward launches - strided views
into token slabs, row groups, K slices, channel windows, fused LayerNorm / pooling - through dd_op_conv_view,
dd_op_layernorm_ld and dd_op_bilinear_view, every operand inside poisoned guards (tests/guard_util.py).

Each case checks four things:
* the body against the same operation in float64 on the CPU at test_ops_gpu.py's bars for the family: 2e-5 (fp32
  conv_gemm), 3e-5 (f16x3), 1e-4 against the bf16-rounded-operand reference (bf16), each of 1 + max|ref|;
* flags == 0 in the f16x3 and bf16 modes;
* independence of what lies outside the operands: the call repeated with every input guard and gap word holding 3e38
  (beyond fp16) instead of NaN gives the same bits and flags == 0; and every guard and gap word of every output still
  holds its sentinel after both calls;
* the route string (dd_op_last_kernel), so each case is known to run the kernel it was written for.

DESIGN.md ("Operand views under guards") has one row per case with the measured error; each test prints its row
(pytest -s).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffusiondrive_amd import _lib
from guard_util import POISON, SENTINEL, dense_strides, guarded
from test_ops_gpu import DEV, close, g, ok, rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
BAR = {0: 2e-5, 1: 3e-5, 2: 1e-4}
MODE = {0: "fp32", 1: "f16x3", 2: "bf16"}
T = 320  # tokens per scene of the GPT slab: 256 image rows, then 64 LiDAR rows


# ------------------------------------------------------------------------------------------------ helpers
def V(p, sn=0, sh=0, sw=0):
    return _lib.DDOpView(p, sn, sh, sw, 1)


def gv(t, start=0):
    """dd_op_view of a 4-D guarded operand (or of the window `start` floats into it)."""
    sn, sh, sw, sc = t.strides
    assert sc == 1
    return V(t.ptr() + 4 * start, sn, sh, sw)


def G_in(values, strides, poison):
    return guarded(tuple(values.shape), strides, poison, values=values, device=DEV)


def G_out(shape, strides, base=None):
    return guarded(shape, strides, SENTINEL, values=base, device=DEV)


class Ran:
    def __init__(self, route, flags, ln, pool):
        self.route, self.flags, self.ln, self.pool, self.bodies = route, flags, ln, pool, {}


def launch(gpu, mode, x, w, out, *, N, H, W, Cin, Cout, k=1, s=1, p=0, res=None, bias=None, relu=False, ldb=None,
           k0=0, route_rows=0, ln=None, pool=None):
    """One dd_op_conv_view call. x / out / res: dd_op_view; w: device fp32 [Cout][ldb]; ln: (out ptr, g, b) device
    pointers; pool: (out view, p, add view or None)."""
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = _lib.DDOpConvDesc()
    d.in_, d.out = x, out
    if res is not None:
        d.res = res
    d.N, d.H, d.W, d.Cin, d.KH, d.KW, d.stride, d.pad, d.Cout = N, H, W, Cin, k, k, s, p, Cout
    d.wgt, d.ldb, d.k0 = w.data_ptr(), ldb if ldb is not None else k * k * Cin, k0
    assert w.numel() == Cout * d.ldb and w.is_contiguous()
    d.bias = bias.data_ptr() if bias is not None else None
    d.relu, d.mode, d.flags, d.route_rows = int(relu), mode, flags.data_ptr(), route_rows
    if ln is not None:
        d.ln_out, d.ln_g, d.ln_b = ln
    if pool is not None:
        d.pool_out, d.pool_p = pool[0], pool[1]
        if pool[2] is not None:
            d.pool_add = pool[2]
    d.fused_ln = d.fused_pool = -1
    ok(gpu.dd_op_conv_view(ctypes.byref(d), None), gpu)
    return Ran(gpu.dd_op_last_kernel().decode(), int(flags.item()), d.fused_ln, d.fused_pool)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice(run):
    """run(poison) -> Ran with .bodies (name -> dense tensor, every output checked). The NaN run and the 3e38 run
    must agree bit for bit with no flag raised; returns the NaN run."""
    a, b = run(NAN), run(POISON)
    assert a.flags == 0 and b.flags == 0, (a.flags, b.flags)
    assert a.route == b.route and (a.ln, a.pool) == (b.ln, b.pool)
    assert a.bodies.keys() == b.bodies.keys()
    for name in a.bodies:
        assert bits_equal(a.bodies[name], b.bodies[name]), f"{name} depends on what lies outside the operands"
    return a


def report(name, shape, form, route, err, bar, ref, words):
    lim = bar * (1.0 + ref.abs().max().item())
    print(f"\nVIEWCASE | {name} | {shape} | {form} | {route} | {err:.2e} / {lim:.2e} | {words}")


def b16(t):
    return t.to(torch.bfloat16).double()


def ops(mode, x, w):
    """The operands as the reference takes them: bf16 rounds x and w (the bf16 image of w 2^e is exact scaling)."""
    return (b16(x), b16(w)) if mode == 2 else (x.double(), w.double())


# ------------------------------------------------------------------------------- ragged dense shapes in guards
@functools.lru_cache(maxsize=None)
def _dense_case(B, H, W, Cin, Cout, k, s, p, relu, res, rounded):
    x = rnd(B, Cin, H, W, seed=201)
    w = rnd(Cout, Cin, k, k, seed=202, scale=1.0 / np.sqrt(Cin * k * k))
    b = rnd(Cout, seed=203)
    xr, wr = ops(2 if rounded else 1, x, w)
    ref = F.conv2d(xr, wr, b.double(), s, p)
    r = rnd(*ref.shape, seed=204) if res else None
    if res:
        ref = ref + r.double()
    if relu:
        ref = F.relu(ref)
    return x, w, b, r, ref.permute(0, 2, 3, 1).contiguous()


DENSE = [
    # mode, (B, H, W, Cin, Cout, k, s, p, relu, res), env, route
    (0, (3, 5, 7, 320, 40, 1, 1, 0, True, True), {}, "conv_gemm"),
    (0, (1, 40, 70, 4, 64, 7, 2, 3, True, False), {}, "conv_gemm"),          # the 7 x 7 / s2 stem
    (1, (3, 5, 7, 320, 40, 1, 1, 0, True, True), {}, "conv_x3<64,64,f16x3>"),
    (1, (1, 9, 11, 36, 24, 3, 1, 1, False, False), {}, "conv_x3<64,64,f16x3>"),  # Cin % 32 != 0: K tail
    (1, (1, 5, 7, 1056, 200, 1, 1, 0, True, True), {}, "conv_x3<64,64,f16x3,ksplit>"),
    # conv_x5 needs a grid that fills the chip: the smallest M at which these two Cout route there
    (1, (15, 66, 66, 36, 200, 3, 1, 1, True, False), {}, "conv_x5<256,256>"),  # generic K, ragged M and N
    (1, (1, 255, 129, 160, 400, 1, 1, 0, False, True), {}, "conv_x5<256,256>"),  # 1 x 1, ragged M and N
    # the shape test_conv2d_f16x3 lists as a conv_x5 one: 36 x 2 tiles of 256 are too few, it runs on conv_x3
    (1, (1, 70, 130, 160, 400, 1, 1, 0, False, True), {}, "conv_x3<64,64,f16x3>"),
    (1, (1, 12, 70, 64, 100, 3, 1, 1, False, True), {"DDMI_X6_SMALL": "0"}, "conv_x6<8,32,64,4,1>"),
    (1, (1, 12, 70, 64, 100, 3, 1, 1, False, True), {}, "conv_x6<8,8,64,2,2>"),  # the small-grid 8 x 8 form
    (2, (3, 5, 7, 320, 40, 1, 1, 0, True, True), {}, "conv_x3<64,64,bf16>"),
    (2, (15, 66, 66, 36, 200, 3, 1, 1, True, False), {}, "conv_x5<256,256,bf16>"),
    (2, (1, 12, 70, 64, 100, 3, 1, 1, False, True), {"DDMI_X6_SMALL": "0"}, "conv_x6<8,32,64,4,2,bf16>"),
    (2, (1, 12, 70, 64, 100, 3, 1, 1, False, True), {}, "conv_x6<8,8,64,2,2,bf16>"),
]


@pytest.mark.parametrize("mode,shape,env,route", DENSE,
                         ids=[f"{MODE[m]}-{'x'.join(map(str, s[:7]))}{'-routed' if e else ''}" for m, s, e, _ in DENSE])
def test_ragged_dense_shapes_inside_guards(gpu, monkeypatch, mode, shape, env, route):
    """Contiguous NHWC operands, each in its own guarded allocation: a K tail or ragged-M row read past the operand
    meets NaN / 3e38, a store past the last row or channel meets the sentinel."""
    B, H, W, Cin, Cout, k, s, p, relu, res = shape
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    x, w, b, r, ref = _dense_case(*shape, mode == 2)
    Ho, Wo = ref.shape[1:3]
    wd, bd = g(w.permute(0, 2, 3, 1)).reshape(Cout, -1), g(b)

    def run(poison):
        X = G_in(x.permute(0, 2, 3, 1), dense_strides((B, H, W, Cin)), poison)
        R = G_in(r.permute(0, 2, 3, 1), dense_strides((B, Ho, Wo, Cout)), poison) if res else None
        O = G_out((B, Ho, Wo, Cout), dense_strides((B, Ho, Wo, Cout)))
        ran = launch(gpu, mode, gv(X), wd, gv(O), N=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p,
                     res=gv(R) if res else None, bias=bd, relu=relu)
        ran.bodies["out"] = O.check()
        ran.words = O.guard_words
        return ran

    ran = twice(run)
    assert ran.route == route
    err = close(ran.bodies["out"], ref, BAR[mode])
    report("dense", shape[:9], f"{MODE[mode]} NHWC in guards", ran.route, err, BAR[mode], ref, ran.words)


# ------------------------------------------------------------------------------------------ the forward's forms
def lin_case(M, K, N, seed, mode, bias=True):
    a = rnd(M, K, seed=seed)
    w = rnd(N, K, seed=seed + 1, scale=1.0 / np.sqrt(K))
    b = rnd(N, seed=seed + 2) if bias else None
    ar, wr = ops(mode, a, w)
    ref = ar @ wr.T + (b.double() if bias else 0)
    return a, w, b, ref


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,C", [(2, 64), (2, 256), (3, 128)])
def test_f1_token_slab_write(gpu, mode, B, C):
    """fuse(): the 1 x 1 conv of the 8 x 8 LiDAR map into rows [256, 320) of every scene's (T, C) token slab, plus the
    position rows broadcast over the batch (res.sn = 0). The 256 image rows of every scene - the front guard and the
    gaps between the scenes - are live sentinel."""
    a, w, b, ref = lin_case(B * 64, C, C, 211, mode)
    pos = rnd(T, C, seed=214)
    ref = (ref.view(B, 64, C) + pos[256:].double()).reshape(B, 8, 8, C)
    wd, bd = g(w), g(b)

    def run(poison):
        X = G_in(a.view(B, 8, 8, C), dense_strides((B, 8, 8, C)), poison)
        P = G_in(pos.view(1, 1, T, C), dense_strides((1, 1, T, C)), poison)
        O = G_out((B, 8, 8, C), (T * C, 8 * C, C, 1))
        ran = launch(gpu, mode, gv(X), wd, gv(O), N=B, H=8, W=8, Cin=C, Cout=C, bias=bd,
                     res=V(P.ptr() + 4 * 256 * C, 0, 8 * C, C))
        ran.bodies["out"], ran.words = O.check(), O.guard_words
        return ran

    ran = twice(run)
    assert ran.route == ("conv_gemm", "conv_x3<64,64,f16x3>", "conv_x3<64,64,bf16>")[mode]
    err = close(ran.bodies["out"], ref, BAR[mode])
    report("F1", (B, 8, 8, C, C), f"{MODE[mode]} out = slab rows 256.., res.sn = 0", ran.route, err, BAR[mode], ref,
           ran.words)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,C", [(2, 64), (2, 256), (3, 128)])
def test_f2_token_slab_read(gpu, mode, B, C):
    """fuse(): the 1 x 1 conv reading rows [256, 320) of every scene's slab into a dense 8 x 8 map; the image rows
    hold NaN / 3e38."""
    a, w, b, ref = lin_case(B * 64, C, C, 221, mode)
    ref = ref.view(B, 8, 8, C)
    wd, bd = g(w), g(b)

    def run(poison):
        X = G_in(a.view(B, 8, 8, C), (T * C, 8 * C, C, 1), poison)
        O = G_out((B, 8, 8, C), dense_strides((B, 8, 8, C)))
        ran = launch(gpu, mode, gv(X), wd, gv(O), N=B, H=8, W=8, Cin=C, Cout=C, bias=bd)
        ran.bodies["out"], ran.words = O.check(), O.guard_words
        return ran

    ran = twice(run)
    assert ran.route == ("conv_gemm", "conv_x3<64,64,f16x3>", "conv_x3<64,64,bf16>")[mode]
    err = close(ran.bodies["out"], ref, BAR[mode])
    report("F2", (B, 8, 8, C, C), f"{MODE[mode]} in = slab rows 256..", ran.route, err, BAR[mode], ref, ran.words)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,C", [(2, 64), (3, 128), (2, 256)])
def test_f3_row_groups_in_place(gpu, mode, B, C):
    """The last GPT block's x = x + proj(y) over the 64 LiDAR rows of every scene: B groups T C floats apart, out
    aliasing res, route_rows = B T. Against fp64, and bit-identical to the same rows of the full B T-row launch."""
    nl, off = 64, 256
    y, w, b, _ = lin_case(B * T, C, C, 231, mode)
    x0 = rnd(B * T, C, seed=234)
    yr, wr = ops(mode, y, w)
    ref = (yr @ wr.T + b.double() + x0.double()).view(B, T, C)
    wd, bd = g(w), g(b)
    gs = T * C

    def run(poison):
        Y = G_in(y.view(B, T, C)[:, off:].reshape(B, nl, 1, C), (gs, C, 0, 1), poison)
        Xs = G_out((B, nl, 1, C), (gs, C, 0, 1), base=x0.view(B, T, C)[:, off:].reshape(B, nl, 1, C))
        ran = launch(gpu, mode, gv(Y), wd, gv(Xs), N=B, H=nl, W=1, Cin=C, Cout=C, bias=bd, res=gv(Xs),
                     route_rows=B * T)
        ran.bodies["rows"], ran.words = Xs.check(), Xs.guard_words
        # the full launch: one group of B T dense rows, in place
        Yf = G_in(y.view(1, B * T, 1, C), (B * gs, C, 0, 1), poison)
        Xf = G_out((1, B * T, 1, C), (B * gs, C, 0, 1), base=x0.view(1, B * T, 1, C))
        full = launch(gpu, mode, gv(Yf), wd, gv(Xf), N=1, H=B * T, W=1, Cin=C, Cout=C, bias=bd, res=gv(Xf))
        assert full.flags == 0
        ran.bodies["full"], ran.full_route = Xf.check(), full.route
        return ran

    ran = twice(run)
    assert ran.route == ("conv_gemm", "conv_x3<64,64,f16x3>", "conv_x3<64,64,bf16>")[mode]
    err = close(ran.bodies["rows"].view(B, nl, C), ref[:, off:], BAR[mode])
    close(ran.bodies["full"].view(B, T, C), ref, BAR[mode])
    assert ran.full_route == ran.route
    assert bits_equal(ran.bodies["rows"].view(B, nl, C), ran.bodies["full"].view(B, T, C)[:, off:])
    report("F3", (B, nl, C, C), f"{MODE[mode]} groups T C apart, out = res, route_rows", ran.route, err, BAR[mode],
           ref, ran.words)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B", [2, 3])
def test_f4_kv_groups_of_65_rows(gpu, mode, B):
    """The keyval slab (B, 65, d): the 1 x 1 conv of the 8 x 8 x 512 BEV map writes rows 0..63 of every group (+ the
    embedding rows, broadcast), then the G = B, R = 1 status GEMM fills row 64. Each launch leaves the other's rows
    as they were."""
    d, Cin, Ks = 256, 512, 8
    a, w, b, ref = lin_case(B * 64, Cin, d, 241, mode)
    st, ws, bs, ref_s = lin_case(B, Ks, d, 245, mode)
    emb = rnd(65, d, seed=249)
    ref = ref.view(B, 64, d) + emb[:64].double()
    ref_s = ref_s + emb[64].double()
    wd, bd, wsd, bsd = g(w), g(b), g(ws), g(bs)

    def run(poison):
        X = G_in(a.view(B, 8, 8, Cin), dense_strides((B, 8, 8, Cin)), poison)
        S = G_in(st.view(B, 1, 1, Ks), (Ks, Ks, 0, 1), poison)
        E = G_in(emb.view(1, 1, 65, d), dense_strides((1, 1, 65, d)), poison)
        slab = G_out((B, 65, 1, d), dense_strides((B, 65, 1, d)))
        KV = slab.window((B, 8, 8, d), (65 * d, 8 * d, d, 1))  # row 64 of every group: the slab's NaN, bit for bit
        ran = launch(gpu, mode, gv(X), wd, gv(KV), N=B, H=8, W=8, Cin=Cin, Cout=d, bias=bd, res=V(E.ptr(), 0, 8 * d, d))
        ran.bodies["kv"], ran.words = KV.check(), KV.guard_words  # row 64 of every group untouched
        row = slab.window((B, 1, 1, d), (65 * d, d, 0, 1), start=64 * d)
        r2 = launch(gpu, mode, gv(S), wsd, gv(row), N=B, H=1, W=1, Cin=Ks, Cout=d, bias=bsd,
                    res=V(E.ptr() + 4 * 64 * d, 0, d, 0))
        assert r2.flags == 0
        ran.bodies["row64"], ran.route2 = row.check(), r2.route  # rows 0..63 still the first launch's bits
        return ran

    ran = twice(run)
    assert ran.route == ("conv_gemm", "conv_x3<64,64,f16x3>")[mode]
    assert ran.route2 == ("conv_gemm", "conv_x3<64,64,f16x3>")[mode]
    err = close(ran.bodies["kv"].view(B, 64, d), ref, BAR[mode])
    err2 = close(ran.bodies["row64"].view(B, d), ref_s, BAR[mode])
    report("F4", (B, 8, 8, Cin, d), f"{MODE[mode]} out groups 65 d apart, res.sn = 0", ran.route, err, BAR[mode], ref,
           ran.words)
    report("F4 row 64", (B, 1, Ks, d), f"{MODE[mode]} G = B, R = 1 into row 64", ran.route2, err2, BAR[mode], ref_s,
           ran.words)


@pytest.mark.parametrize("mode", [0, 1])
def test_f5_k_slice_of_a_channel_window(gpu, mode):
    """bev_proj's split projection: the K slice [k0, k0 + 64) of a weight whose rows are 128 floats, A a 64-channel
    window (channels 256..319) of a 320-channel map whose other channels hold NaN / 3e38. Each half against fp64, and
    the second half accumulated onto the first (res = out, in place) against the full-K product."""
    M, kn, ldb, N, CC = 161, 64, 128, 256, 320
    a, w, b, ref = lin_case(M, ldb, N, 251, mode)
    ar, wr = ops(mode, a, w)
    half = [ar[:, :kn] @ wr[:, :kn].T + b.double(), ar[:, kn:] @ wr[:, kn:].T]
    wd, bd = g(w), g(b)

    def run(poison):
        O = G_out((1, M, 1, N), dense_strides((1, M, 1, N)))
        ran = None
        for h, k0 in enumerate((0, 64)):
            A = G_in(a[:, k0:k0 + kn].reshape(1, M, 1, kn), (M * CC, CC, 0, 1), poison)
            H = G_out((1, M, 1, N), dense_strides((1, M, 1, N)))
            r1 = launch(gpu, mode, gv(A), wd, gv(H), N=1, H=M, W=1, Cin=kn, Cout=N, ldb=ldb, k0=k0,
                        bias=bd if h == 0 else None)
            # the forward's chain: the second half adds to the first in place
            r2 = launch(gpu, mode, gv(A), wd, gv(O), N=1, H=M, W=1, Cin=kn, Cout=N, ldb=ldb, k0=k0,
                        bias=bd if h == 0 else None, res=gv(O) if h else None)
            assert r1.flags == 0 and r2.flags == 0 and r1.route == r2.route
            ran = ran or r1
            ran.bodies[f"half{h}"] = H.check()
        ran.bodies["sum"], ran.words = O.check(), O.guard_words
        return ran

    ran = twice(run)
    assert ran.route == ("conv_gemm", "conv_x3<64,64,f16x3>")[mode]
    for h in (0, 1):
        err = close(ran.bodies[f"half{h}"].view(M, N), half[h], BAR[mode])
        report(f"F5 k0 = {64 * h}", (M, kn, N), f"{MODE[mode]} slice_k of ldb 128, A = channels 256.. of 320",
               ran.route, err, BAR[mode], half[h], ran.words)
    err = close(ran.bodies["sum"].view(M, N), ref, BAR[mode])
    report("F5 sum", (M, ldb, N), f"{MODE[mode]} both halves, second in place", ran.route, err, BAR[mode], ref,
           ran.words)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,Cout", [(2, 1), (3, 1), (2, 7)])
def test_f6_narrow_output_rows(gpu, mode, B, Cout):
    """The agent heads: A = rows 1..30 of every 31-row query group, Cout = 1 (labels) or 7 with the output row stride
    equal to Cout - no row is 16-byte aligned, the element-wise epilogue."""
    R, K, NQ = 30, 256, 31
    a, w, b, ref = lin_case(B * R, K, Cout, 261, mode)
    wd, bd = g(w), g(b)

    def run(poison):
        A = G_in(a.view(B, R, 1, K), (NQ * K, K, 0, 1), poison)
        O = G_out((B, R, 1, Cout), (R * Cout, Cout, 0, 1))
        ran = launch(gpu, mode, gv(A), wd, gv(O), N=B, H=R, W=1, Cin=K, Cout=Cout, bias=bd)
        ran.bodies["out"], ran.words = O.check(), O.guard_words
        return ran

    ran = twice(run)
    assert ran.route == ("conv_gemm", "conv_x3<64,64,f16x3>")[mode]
    err = close(ran.bodies["out"].view(B * R, Cout), ref, BAR[mode])
    report("F6", (B, R, K, Cout), f"{MODE[mode]} A groups 31 d apart, out row stride = Cout", ran.route, err,
           BAR[mode], ref, ran.words)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M,C", [(64, 64), (161, 64), (64, 128), (161, 128), (161, 256)])
def test_f7_fused_layernorm(gpu, mode, M, C):
    """gemm_ln: x = x + proj(y) with Y = LayerNorm(x) from the same launch where one N tile spans the row (Cout 64 /
    128 on conv_x3). C against fp64; the fused flag; ln_out bit-identical to dd_op_layernorm on the op's own C (the
    claim common.h makes). Not fused (Cout = 256, or the fp32 kernel): flag 0 and ln_out untouched."""
    y, w, b, _ = lin_case(M, C, C, 271, mode)
    x0 = rnd(M, C, seed=274)
    lg, lb = 1.0 + 0.1 * rnd(C, seed=275), rnd(C, seed=276)
    yr, wr = ops(mode, y, w)
    ref = yr @ wr.T + b.double() + x0.double()
    wd, bd, lgd, lbd = g(w), g(b), g(lg), g(lb)
    fused = mode != 0 and C in (64, 128)

    def run(poison):
        Y = G_in(y.view(1, M, 1, C), dense_strides((1, M, 1, C)), poison)
        X = G_out((1, M, 1, C), dense_strides((1, M, 1, C)), base=x0.view(1, M, 1, C))
        L = G_out((1, M, 1, C), dense_strides((1, M, 1, C)))
        ran = launch(gpu, mode, gv(Y), wd, gv(X), N=1, H=M, W=1, Cin=C, Cout=C, bias=bd, res=gv(X),
                     ln=(L.ptr(), lgd.data_ptr(), lbd.data_ptr()))
        ran.bodies["x"], ran.bodies["ln"], ran.words = X.check(), L.check(), X.guard_words + L.guard_words
        return ran

    ran = twice(run)
    assert ran.ln == int(fused)
    assert ran.route == ("conv_gemm", f"conv_x3<64,{C if fused else 64},f16x3>",
                         f"conv_x3<64,{C if fused else 64},bf16>")[mode]
    xb = ran.bodies["x"].view(M, C)
    err = close(xb, ref, BAR[mode])
    if fused:
        sep = torch.full((M, C), NAN, device=DEV)
        xd = xb.contiguous()
        ok(gpu.dd_op_layernorm(xd.data_ptr(), None, 1, lgd.data_ptr(), lbd.data_ptr(), None, None, sep.data_ptr(), M,
                               C, None), gpu)
        assert bits_equal(ran.bodies["ln"].view(M, C), sep)
    else:
        assert torch.isnan(ran.bodies["ln"]).all()  # the body still NaN, its guards still sentinel (check())
    report("F7", (M, C, C), f"{MODE[mode]} fold_ln, out = res" + ("" if fused else " (not fused)"), ran.route, err,
           BAR[mode], ref, ran.words)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_f8_fused_token_pooling(gpu, mode):
    """A stage's final 3 x 3 conv (+ residual, ReLU) on a 16 x 64 map that also writes the 8 x 32 GPT tokens - the
    2 x 2 window means plus the position rows - into rows [0, 256) of every scene's slab (conv_x6). Without the add,
    the tokens are bit-identical to dd_op_avgpool of the op's own output. The fp32 kernel does not fuse: flag 0,
    pool_out untouched."""
    B, H, W, C = 2, 16, 64, 64
    x = rnd(B, C, H, W, seed=281)
    w = rnd(C, C, 3, 3, seed=282, scale=1.0 / np.sqrt(C * 9))
    b, r, pos = rnd(C, seed=283), rnd(B, C, H, W, seed=284), rnd(T, C, seed=285)
    xr, wr = ops(mode, x, w)
    ref = F.relu(F.conv2d(xr, wr, b.double(), 1, 1) + r.double())
    ref_tok = (F.avg_pool2d(ref, 2).permute(0, 2, 3, 1) + pos[:256].double().view(8, 32, C)).contiguous()
    ref = ref.permute(0, 2, 3, 1).contiguous()
    wd, bd = g(w.permute(0, 2, 3, 1)).reshape(C, -1), g(b)
    fused = mode != 0

    def run(poison):
        X = G_in(x.permute(0, 2, 3, 1), dense_strides((B, H, W, C)), poison)
        R = G_in(r.permute(0, 2, 3, 1), dense_strides((B, H, W, C)), poison)
        P = G_in(pos.view(1, 1, T, C), dense_strides((1, 1, T, C)), poison)
        ran = None
        for add in (True, False):
            O = G_out((B, H, W, C), dense_strides((B, H, W, C)))
            Tk = G_out((B, 8, 32, C), (T * C, 32 * C, C, 1))
            one = launch(gpu, mode, gv(X), wd, gv(O), N=B, H=H, W=W, Cin=C, Cout=C, k=3, s=1, p=1, bias=bd, res=gv(R),
                         relu=True, pool=(gv(Tk), 2, V(P.ptr(), 0, 32 * C, C) if add else None))
            ran = ran or one
            assert one.flags == 0 and one.route == ran.route and one.pool == ran.pool
            ran.bodies["out" if add else "out_plain"] = O.check()
            ran.bodies["tok" if add else "tok_plain"] = Tk.check()
            ran.words = O.guard_words + Tk.guard_words
        return ran

    ran = twice(run)
    assert ran.pool == int(fused)
    assert ran.route == ("conv_gemm", "conv_x6<8,8,64,2,2>", "conv_x6<8,8,64,2,2,bf16>")[mode]
    err = close(ran.bodies["out"], ref, BAR[mode])
    assert bits_equal(ran.bodies["out"], ran.bodies["out_plain"])
    if fused:
        errt = close(ran.bodies["tok"], ref_tok, BAR[mode])
        sep = torch.full((B, 8, 32, C), NAN, device=DEV)
        od = ran.bodies["out"].contiguous()
        ok(gpu.dd_op_avgpool(od.data_ptr(), B, H, W, C, 8, 32, sep.data_ptr(), None), gpu)
        assert bits_equal(ran.bodies["tok_plain"], sep)
        report("F8 tokens", (B, 8, 32, C), f"{MODE[mode]} pool_into slab rows 0..255 + pos", ran.route, errt, BAR[mode],
               ref_tok, ran.words)
    else:
        assert torch.isnan(ran.bodies["tok"]).all() and torch.isnan(ran.bodies["tok_plain"]).all()
    report("F8", (B, H, W, C, C), f"{MODE[mode]} 3 x 3 + res + ReLU" + (", pooled" if fused else " (not pooled)"),
           ran.route, err, BAR[mode], ref, ran.words)


# ------------------------------------------------------------------------------------- LayerNorm, bilinear
@pytest.mark.parametrize("film_div", [0, 20])
def test_layernorm_ld(gpu, film_div):
    """LayerNorm over rows of a slab (ldx = ldy = 320 > C = 256) with a residual row per res_div rows and FiLM - one
    pair for every row, or (film_div) one pair per 20 rows, film_ld floats apart - against F.layer_norm in fp64 at
    test_layernorm's bar, and bit-identical to dd_op_layernorm on the same values in dense buffers."""
    rows, C, ld, res_div, ldres, film_ld = 77, 256, 320, 20, 288, 512
    ng = -(-rows // res_div)
    x = rnd(rows, C, seed=291, scale=3.0) + 0.5
    res = rnd(ng, C, seed=292)
    gam, bet = rnd(C, seed=293), rnd(C, seed=294)
    nf = ng if film_div else 1
    fs, fb = rnd(nf, C, seed=295), rnd(nf, C, seed=296)
    rep = lambda t: t.double().repeat_interleave(res_div, 0)[:rows]  # noqa: E731
    ref = F.layer_norm(x.double() + rep(res), (C,), gam.double(), bet.double(), 1e-5)
    ref = ref * (1 + (rep(fs) if film_div else fs.double())) + (rep(fb) if film_div else fb.double())
    gd, bd = g(gam), g(bet)

    def run(poison):
        X = G_in(x.view(1, rows, 1, C), (rows * ld, ld, 0, 1), poison)
        Rz = G_in(res.view(1, ng, 1, C), (ng * ldres, ldres, 0, 1), poison)
        Fs = G_in(fs.view(1, nf, 1, C), (nf * film_ld, film_ld, 0, 1), poison)
        Fb = G_in(fb.view(1, nf, 1, C), (nf * film_ld, film_ld, 0, 1), poison)
        Y = G_out((1, rows, 1, C), (rows * ld, ld, 0, 1))
        ok(gpu.dd_op_layernorm_ld(X.ptr(), ld, Rz.ptr(), ldres, res_div, gd.data_ptr(), bd.data_ptr(), Fs.ptr(),
                                  Fb.ptr(), film_div, film_ld if film_div else 0, Y.ptr(), ld, rows, C, None), gpu)
        ran = Ran("layernorm", 0, 0, 0)
        ran.bodies["y"], ran.words = Y.check(), Y.guard_words
        return ran

    ran = twice(run)
    yb = ran.bodies["y"].view(rows, C)
    err = close(yb, ref, 1e-5)
    # the dense op: one FiLM pair per call, so the per-group form is compared group by group
    xd, rd, fsd, fbd = g(x), g(res), g(fs), g(fb)
    dense = torch.full((rows, C), NAN, device=DEV)
    for k in range(ng if film_div else 1):
        r0, r1 = (k * res_div, min(rows, (k + 1) * res_div)) if film_div else (0, rows)
        ok(gpu.dd_op_layernorm(xd[r0:].data_ptr(), rd[k:].data_ptr(), res_div, gd.data_ptr(), bd.data_ptr(),
                               fsd[k:].data_ptr(), fbd[k:].data_ptr(), dense[r0:].data_ptr(), r1 - r0, C, None), gpu)
    assert bits_equal(yb, dense)
    report("layernorm_ld", (rows, C), f"ld 320, res_div 20 ldres 288, film_div {film_div}", "layernorm_v4", err, 1e-5,
           ref, ran.words)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,C,ldo", [(2, 256, 320), (3, 7, 9)])
def test_bilinear_view(gpu, B, C, ldo, accumulate):
    """concat_cross_bev's resize: the input is rows 0..63 of every 65-row keyval group as an 8 x 8 map, the output the
    first C channels of a wider map; the float4 form (C = 256) and the scalar form (C % 4 != 0), plain and
    accumulating, at test_bilinear's bar and bit-identical to the dense op."""
    Hi = Wi = 8
    Ho, Wo = 16, 24
    x = rnd(B, C, Hi, Wi, seed=301)
    base = rnd(B, Ho, Wo, C, seed=302)
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    if accumulate:
        ref = ref + base.double()
    xh = x.permute(0, 2, 3, 1).contiguous()

    def run(poison):
        X = G_in(xh, (65 * C, Wi * C, C, 1), poison)
        O = G_out((B, Ho, Wo, C), (Ho * Wo * ldo, Wo * ldo, ldo, 1), base=base if accumulate else None)
        vi, vo = gv(X), gv(O)
        ok(gpu.dd_op_bilinear_view(ctypes.byref(vi), B, Hi, Wi, C, ctypes.byref(vo), Ho, Wo, accumulate, None), gpu)
        ran = Ran("bilinear", 0, 0, 0)
        ran.bodies["out"], ran.words = O.check(), O.guard_words
        return ran

    ran = twice(run)
    err = close(ran.bodies["out"], ref, 1e-6)
    xd = g(xh)
    dense = g(base) if accumulate else torch.full((B, Ho, Wo, C), NAN, device=DEV)
    fn = gpu.dd_op_bilinear_add if accumulate else gpu.dd_op_bilinear
    ok(fn(xd.data_ptr(), B, Hi, Wi, C, dense.data_ptr(), Ho, Wo, None), gpu)
    assert bits_equal(ran.bodies["out"], dense)
    report("bilinear_view", (B, Hi, Wi, C, Ho, Wo), f"in groups 65 C apart, out ld {ldo}, accumulate {accumulate}",
           "bilinear", err, 1e-6, ref, ran.words)


# ------------------------------------------------------------------------------------------ negative control
def test_harness_reports_a_channel_outside_the_declared_view(gpu):
    """The file can fail: the output declared one channel narrower than the launch's Cout (row stride 8, 6 channels
    declared, 7 written) - the seventh channel lands in a gap word and check() raises."""
    B, R, K, Cout = 2, 30, 256, 7
    a, w, b, ref = lin_case(B * R, K, Cout, 311, 1)
    wd, bd = g(w), g(b)
    A = G_in(a.view(B, R, 1, K), dense_strides((B, R, 1, K)), NAN)
    O = G_out((B, R, 1, Cout - 1), (R * 8, 8, 0, 1))
    ran = launch(gpu, 1, gv(A), wd, gv(O), N=B, H=R, W=1, Cin=K, Cout=Cout, bias=bd)
    assert ran.flags == 0
    assert O.dirty() == [m * 8 + 6 for m in range(B * R)]
    with pytest.raises(AssertionError, match="overwritten"):
        O.check()
    close(O.view().reshape(B * R, Cout - 1), ref[:, :Cout - 1], BAR[1])  # the declared channels are right
