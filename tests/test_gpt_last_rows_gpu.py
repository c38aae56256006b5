"""The last block of the last fusion scale's GPT computes only the 64 LiDAR-token rows of every scene after its K / V
projection (nothing downstream reads the image tokens there; DESIGN.md section 4, GPT rows): the attention kernel over
a query window, the LayerNorm over row groups, and the forward with the path on (default) against
DDMI_GPT_LAST_ROWS=0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, HEADS = 320, 4
NAN_BITS = 0x7FC00BAD  # a quiet NaN with a payload no kernel produces


def ok(rc, lib):
    from diffusiondrive_amd import _lib
    _lib.check(rc, lib, op=True)


def nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def qkv_inputs():
    """One packed q | k | v per head size, shared by every window / precision case (never written)."""
    out = {}
    for C in (64, 256, 512):
        gen = torch.Generator().manual_seed(1000 + C)
        out[C] = torch.randn(2, T, 3 * C, generator=gen).cuda()
    return out


@pytest.fixture(scope="module")
def full_attention(gpu, qkv_inputs):
    """The full launches the windows are compared with, computed once per (C, prec)."""
    ref = {}
    for C, qkv in qkv_inputs.items():
        for prec in (0, 1, 2):
            y = nan_filled(2, T, C)
            ok(gpu.dd_op_gpt_attention(qkv.data_ptr(), y.data_ptr(), 2, T, C, HEADS, prec, None), gpu)
            ref[C, prec] = bits(y)
    torch.cuda.synchronize()
    return ref


@pytest.mark.parametrize("window", [(256, 64), (64, 64)])
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("C", [64, 256, 512])
def test_attention_window_rows_equal_full_launch(gpu, qkv_inputs, full_attention, C, prec, window):
    """Head sizes 16 / 64 / 128 (double and single LDS stages, every wave-count branch of the f16x3 form), the fp32
    and both f16x3 forms: the rows of the window are the full launch's bit for bit, every other row of y keeps the
    NaN pattern it was filled with."""
    q0, nq = window
    full = full_attention[C, prec]
    assert not np.any(full == NAN_BITS)  # the full launch wrote every row
    y = nan_filled(2, T, C)
    ok(gpu.dd_op_gpt_attention_rows(qkv_inputs[C].data_ptr(), y.data_ptr(), 2, T, C, HEADS, prec, q0, nq, 0, None),
       gpu)
    got = bits(y)
    assert np.array_equal(got[:, q0:q0 + nq], full[:, q0:q0 + nq])
    outside = np.ones(T, bool)
    outside[q0:q0 + nq] = False
    assert np.all(got[:, outside] == NAN_BITS)


def test_attention_window_rejects_partial_blocks(gpu, qkv_inputs):
    """The f16x3 form takes whole 32-row blocks, the fp32 form whole 64-row blocks, inside [0, T)."""
    y = nan_filled(2, T, 64)
    p = qkv_inputs[64].data_ptr()
    for prec, q0, nq in ((1, 16, 32), (1, 256, 48), (0, 32, 64), (0, 256, 32), (1, 288, 64), (1, 0, 0)):
        assert gpu.dd_op_gpt_attention_rows(p, y.data_ptr(), 2, T, 64, HEADS, prec, q0, nq, 0, None) != 0
    torch.cuda.synchronize()
    assert np.all(bits(y) == NAN_BITS)


@pytest.mark.parametrize("C", [512, 64])
def test_layernorm_groups_equal_dense_rows(gpu, C):
    """3 groups of 64 rows, 320 rows apart: the rows of the groups are dd_op_layernorm's bit for bit, the rows between
    them keep the fill."""
    G, R, S = 3, 64, 320
    gen = torch.Generator().manual_seed(7 + C)
    x = torch.randn(G * S, C, generator=gen).cuda()
    g = torch.randn(C, generator=gen).cuda()
    b = torch.randn(C, generator=gen).cuda()
    full = nan_filled(G * S, C)
    ok(gpu.dd_op_layernorm(x.data_ptr(), None, 1, g.data_ptr(), b.data_ptr(), None, None, full.data_ptr(), G * S, C,
                           None), gpu)
    y = nan_filled(G * S, C)
    off = 256 * C  # the groups start at row 256 of every 320, as the GPT's LiDAR tokens do
    ok(gpu.dd_op_layernorm_groups(x.data_ptr() + 4 * off, g.data_ptr(), b.data_ptr(), y.data_ptr() + 4 * off, G, R,
                                  S * C, C, None), gpu)
    full, got = bits(full).reshape(G, S, C), bits(y).reshape(G, S, C)
    assert not np.any(full == NAN_BITS)
    assert np.array_equal(got[:, 256:], full[:, 256:])
    assert np.all(got[:, :256] == NAN_BITS)


@pytest.mark.parametrize("mode,B", [("f16x3", 3), ("f16x3", 17), ("fp32", 3), ("bf16", 3)])
def test_forward_equals_full_row_block(seeded_sd, monkeypatch, mode, B):
    """Fresh handles with the live-row block (default) and with DDMI_GPT_LAST_ROWS=0, on either side of the B <= 16
    small-batch forms: every output, the bev_feature tap and the LiDAR rows of ln_f (gpt_h) are bit-identical - a
    row's K walk does not depend on how many rows the GEMM has - with no numerics flag raised; and the profiler's
    attention FLOPs drop by exactly the 256 image-token query rows of the C = 512 block, so the path ran."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(B, 61)
    feats = {k: torch.from_numpy(inp[k]).cuda() for k in ("camera_feature", "lidar_feature", "status_feature")}
    nz = torch.from_numpy(inp["noise"]).cuda()

    def run(flag):
        if flag is None:
            monkeypatch.delenv("DDMI_GPT_LAST_ROWS", raising=False)
        else:
            monkeypatch.setenv("DDMI_GPT_LAST_ROWS", flag)
        m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm=mode)
        try:
            m.set_profiling(True)
            m.reset_stats()
            out = {k: v.cpu().numpy() for k, v in m.forward(feats, noise=nz, modes=True).items()}
            flops = m.kernel_stats("attn")["flops"]
            m.set_profiling(False)
            taps = {"bev_feature": m.tap("bev_feature").cpu().numpy()[: B * 64 * 512],
                    "gpt_h": m.tap("gpt_h").cpu().numpy()[: B * T * 512].reshape(B, T, 512)[:, 256:]}
            assert m.numerics_flags() == 0
            return out, taps, flops
        finally:
            m.close()

    on, on_taps, on_flops = run(None)
    off, off_taps, off_flops = run("0")
    print(f"[gpt_last_rows] {mode} B={B}: attn flops {off_flops:.6g} -> {on_flops:.6g}")
    assert off_flops - on_flops == 4 * B * 256 * T * 512  # 0.8 * 4 B T^2 C at C = 512
    assert set(on) == set(off)
    for k in off:
        assert np.array_equal(on[k], off[k]), (mode, B, k)
    for k in off_taps:
        assert np.array_equal(on_taps[k], off_taps[k]), (mode, B, k)
