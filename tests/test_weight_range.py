"""The host's f16x3 / bf16 weight split over the whole range of fp32 rows ("Dead and tiny rows").

Two routines scale every weight row by a power of two and split it into fp16 images: prep_split (weights.cpp: every
conv and Linear, the stems, the GPT q | k | v, the tf decoder's K | V) and pack_mk_weights (decoder_mk.hip: the
megakernels' fragment-ordered images). Both are reached here on host pointers through dd_op_split_weights and
dd_op_pack_mk_weights, without a GPU, and held

  - bit for bit to f16x3_emul.split_weights, the arithmetic every bound test rests on, on rows of the seeded dict and on
    the rowrange family's rows (f16x3_cases.py);
  - to range properties on rows down to fp32's smallest subnormal and on an all-zero row: finite images, a finite,
    normal power-of-two 1 / s, hi + lo = w s to fp16's rounding of lo;
  - at the threshold itself: a row whose largest |weight| is 2^-113, the fp32 number below it, and the smallest
    subnormal.

Without the bound |e| <= 126 on the scale's exponent, as both routines and the emulation were before these tests: a row with 0 < max|w_r| < 2^-113 needs
s = 2^128 = inf in fp32, every nonzero weight of it becomes inf in hi and in the bf16 image, lo = inf - inf = NaN, and
its zeros 0 * inf = NaN; a row at 2^-113 exactly gets s = 2^127 and the subnormal 1 / s = 2^-127.

The rest is the CPU premise of test_weight_range_gpu.py: the census of the split's call sites against the ``dead_rows``
dict (rescale_util.py), and the fp32 and emulated-f16x3 oracles on that dict inside half of every bar.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import batch_sweep_util as U
import f16x3_cases as C
import f16x3_emul as E
import rescale_util as R
from test_ops_gpu import rnd
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)
F32_TINY = 2.0 ** -126


# --------------------------------------------------------------------------- the two routines on host pointers
@pytest.fixture(scope="module")
def lib():
    from diffusiondrive_amd import _lib
    return _lib.load()


def cpp_split(lib, w):
    """prep_split of a (rows, K) fp32 matrix: (hi, lo, b16) as (rows, ldh) fp16 / fp16 / bf16 tensors and sinv."""
    w = np.ascontiguousarray(w.numpy(), np.float32)
    rows, K = w.shape
    ldh = (K + 7) // 8 * 8
    hi, lo, b16 = (np.full((rows, ldh), 0x7e7e, np.uint16) for _ in range(3))
    sinv = np.full(rows, np.nan, np.float32)
    got = ctypes.c_int(-1)
    rc = lib.dd_op_split_weights(w.ctypes.data, rows, K, hi.ctypes.data, lo.ctypes.data, b16.ctypes.data,
                                 sinv.ctypes.data, ctypes.byref(got))
    assert rc == 0, lib.dd_op_last_error()
    assert got.value == ldh
    t = [torch.from_numpy(a.view(np.int16)) for a in (hi, lo, b16)]
    return t[0].view(torch.float16), t[1].view(torch.float16), t[2].view(torch.bfloat16), torch.from_numpy(sinv)


def cpp_pack(lib, w):
    """pack_mk_weights of a (nout, nin) fp32 matrix: the packed halfs (nout / 32, nin / 16, 64, 16) and sinv."""
    w = np.ascontiguousarray(w.numpy(), np.float32)
    nout, nin = w.shape
    pk = np.full(nout * nin * 2, 0x7e7e, np.uint16)
    sinv = np.full(nout, np.nan, np.float32)
    rc = lib.dd_op_pack_mk_weights(w.ctypes.data, nout, nin, pk.ctypes.data, sinv.ctypes.data)
    assert rc == 0, lib.dd_op_last_error()
    return torch.from_numpy(pk.view(np.int16)).view(torch.float16).view(nout // 32, nin // 16, 64, 16), \
        torch.from_numpy(sinv)


def packed_layout(hi, lo):
    """(nout, nin) halfs in the order runtime.cpp documents for an MkLin image: block (nt, ks) of 64 lanes x (8 hi, 8
    lo), lane = col % 32 + 32 ((k % 16) / 8)."""
    nout, nin = hi.shape

    def lanes(h):  # [nt, col % 32, ks, (k % 16) / 8, k % 8] -> [nt, ks, lane, k % 8]
        return h.view(nout // 32, 32, nin // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(nout // 32, nin // 16, 64, 8)
    return torch.cat([lanes(hi), lanes(lo)], -1)


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def folded_conv_rows(sd, conv, bn):
    """prep_conv's matrix of a conv with its BatchNorm folded: scale in double, rounded to fp32, OHWI rows."""
    s = np.asarray(sd[bn + ".weight"], np.float64) / np.sqrt(np.asarray(sd[bn + ".running_var"], np.float64) + 1e-5)
    w = (np.asarray(sd[conv + ".weight"], np.float64) * s[:, None, None, None]).astype(np.float32)
    return E.weight_rows(torch.from_numpy(w))


def _seeded_rows(sd, name):
    if name == "conv3x3-bn":
        return folded_conv_rows(sd, "_backbone.image_encoder.layer1.0.conv1", "_backbone.image_encoder.layer1.0.bn1")
    if name == "linear-k8":
        return torch.from_numpy(np.asarray(sd["_status_encoding.weight"]))
    if name == "linear-k13":
        return rnd(40, 13, seed=241, scale=13 ** -0.5)             # K % 8 != 0: five padding columns
    if name == "mk-k64":
        return torch.from_numpy(np.ascontiguousarray(np.asarray(sd["bev_proj.0.weight"])[:, 256:]))
    layer = "_trajectory_head.diff_decoder.layers.0.ffn."
    return torch.from_numpy(np.asarray(sd[layer + ("0" if name == "mk-k256" else "2") + ".weight"]))


def _rowrange_rows(name):
    if name == "rowrange-conv-k324":                                # K = 9 * 36, K % 8 = 4
        return E.weight_rows(C.conv_case(C.CONV_CASES[4][1], "rowrange").w).contiguous()
    return C.mk_case(*{"rowrange-mk-k256": (256, 256), "rowrange-mk-k1024": (1024, 256)}[name], "rowrange").w


SPLIT_INPUTS = ["conv3x3-bn", "linear-k8", "linear-k13", "mk-k64", "mk-k256", "mk-k1024",
                "rowrange-conv-k324", "rowrange-mk-k256", "rowrange-mk-k1024"]
PACK_INPUTS = ["mk-k64", "mk-k256", "mk-k1024", "rowrange-mk-k256", "rowrange-mk-k1024"]
RANGE_INPUTS = [n for n in SPLIT_INPUTS if n.startswith("rowrange")]


def _rows(seeded_sd, name):
    return _rowrange_rows(name) if name.startswith("rowrange") else _seeded_rows(seeded_sd, name)


# --------------------------------------------------------------------------- images against the emulation, bit for bit
@pytest.mark.parametrize("name", SPLIT_INPUTS)
def test_prep_split_equals_the_emulation_bit_for_bit(lib, seeded_sd, name):
    w = _rows(seeded_sd, name)
    rows, K = w.shape
    hi, lo, b16, sinv = cpp_split(lib, w)
    eh, el, es = E.split_weights(w)
    assert same_bits(hi[:, :K], eh), name
    assert same_bits(lo[:, :K], el), name
    assert torch.equal(sinv.view(torch.int32), es.view(torch.int32)), name
    want = (w.float() * (1.0 / es.double()).float()[:, None]).bfloat16()     # bf16(w s), s = 1 / sinv exactly
    assert same_bits(b16[:, :K], want), name
    for img in (hi, lo, b16):                                                 # padding columns: +0
        assert not bits(img[:, K:]).any(), name


@pytest.mark.parametrize("name", PACK_INPUTS)
def test_pack_mk_weights_equals_the_emulation_bit_for_bit(lib, seeded_sd, name):
    w = _rows(seeded_sd, name)
    pk, sinv = cpp_pack(lib, w)
    eh, el, es = E.split_weights(w)
    assert torch.equal(sinv.view(torch.int32), es.view(torch.int32)), name
    assert same_bits(pk, packed_layout(eh, el)), name


def test_packed_layout_is_the_documented_one():
    """The permutation itself, spelled out element by element on a small matrix of distinct values."""
    nout, nin = 64, 32
    hi = torch.arange(nout * nin, dtype=torch.float32).view(nout, nin).half()       # < 2048: exact in fp16
    lo = -hi
    pk = packed_layout(hi, lo)
    for col, k in ((0, 0), (31, 7), (5, 8), (33, 15), (63, 31), (40, 16)):
        nt, ks, lane = col // 32, k // 16, col % 32 + 32 * ((k % 16) // 8)
        assert pk[nt, ks, lane, k % 8] == hi[col, k] and pk[nt, ks, lane, 8 + k % 8] == lo[col, k]


# --------------------------------------------------------------------------- range properties
def _check_range(w, hi, lo, sinv, b16=None):
    """Every row of ``w`` (rows, K), images as (rows, K) tensors: finite, 1 / s a normal power of two, hi + lo = w s to
    the rounding of lo, hi = w s to the rounding of hi, an all-zero row all zero with 1 / s = 1."""
    for name, img in (("hi", hi), ("lo", lo), ("b16", b16)):
        if img is not None:
            bad = (~torch.isfinite(img.float())).any(1).nonzero().flatten().tolist()
            assert not bad, f"{name} image not finite on rows {bad[:8]}: max|w| {w[bad[0]].abs().max():.3e}"
    m, _ = torch.frexp(sinv)
    assert torch.isfinite(sinv).all() and (m == 0.5).all(), sinv[(m != 0.5)][:8]
    assert (sinv >= F32_TINY).all(), f"1 / s subnormal on rows {(sinv < F32_TINY).nonzero().flatten().tolist()[:8]}"
    v = w.double() / sinv.double()[:, None]                 # w s exactly: s a power of two with 2^-126 <= 1 / s
    d = v - hi.double()
    assert (d.abs() <= torch.maximum(2.0 ** -11 * v.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all()
    assert ((d - lo.double()).abs() <= torch.maximum(2.0 ** -11 * d.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all()
    zero = (w == 0).all(1)
    for img in (hi, lo, b16):
        if img is not None:
            assert not bits(img[zero]).any()
    assert (sinv[zero] == 1.0).all()
    # a row that is not tiny fills the fp16 range: max |hi| in [2^14, 2^15]
    full = w.abs().amax(1) >= 2.0 ** -111
    top = hi.float().abs().amax(1)[full]
    assert ((top >= 2.0 ** 14) & (top <= 2.0 ** 15)).all()


@pytest.mark.parametrize("name", RANGE_INPUTS)
def test_prep_split_range_properties(lib, name):
    w = _rowrange_rows(name)
    K = w.shape[1]
    assert (w == 0).all(1).any() and (w.abs().amax(1) < 2.0 ** -126).any() and (w.abs().amax(1) > 2.0 ** 100).any()
    hi, lo, b16, sinv = cpp_split(lib, w)
    _check_range(w, hi[:, :K], lo[:, :K], sinv, b16[:, :K])


@pytest.mark.parametrize("name", [n for n in RANGE_INPUTS if "-mk-" in n])
def test_pack_mk_weights_range_properties(lib, name):
    w = _rowrange_rows(name)
    pk, sinv = cpp_pack(lib, w)
    nout, nin = w.shape
    # undo the documented permutation: [nt, ks, half, col % 32, e] -> (nout, nin)
    hi, lo = (pk[..., s].reshape(nout // 32, nin // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(nout, nin)
              for s in (slice(0, 8), slice(8, 16)))
    _check_range(w, hi, lo, sinv)


@pytest.mark.parametrize("name", RANGE_INPUTS)
def test_emulated_split_range_properties(name):
    """The same properties of f16x3_emul.split_weights: the bound tests' arithmetic is itself sound on these rows."""
    w = _rowrange_rows(name)
    hi, lo, sinv = E.split_weights(w)
    _check_range(w, hi, lo, sinv)


def test_row_range_places_tiny_rows_at_the_tile_ends():
    """rowrange: every item of the cycle occurs; the last channel and every 32-column tile's last channel are tiny or
    zero with a normal row on either side; the two threshold rows hold exactly the values they are named for."""
    for N, seed in ((24, 215), (36, 215), (40, 215), (64, 225), (128, 215), (192, 215), (200, 215), (256, 235)):
        items = C.row_range(N, seed)
        assert set(items) == set(C.ROWRANGE), (N, set(C.ROWRANGE) - set(items))
        tiny = C.tiny_rows(N, seed)
        for n in sorted({N - 1} | set(range(31, N, 32))):
            assert tiny[n], (N, n)
            for m in (n - 1, n + 1):
                if 0 <= m < N:
                    assert not tiny[m], (N, n, m)
    case = C.mk_case(256, 256, "rowrange")
    items = C.row_range(256, 235)
    amax = case.w.abs().amax(1).double()
    for n, item in enumerate(items):
        if item == "zero":
            assert amax[n] == 0 and case.b[n] != 0
        elif isinstance(item, str):
            assert amax[n] == C.EDGE[item], (n, item)
    unit = C.mk_case(256, 256, "uniform")
    assert torch.equal(case.b[case.tiny], unit.b[case.tiny])                # the bias survives on the dead rows
    n110 = items.index(110)
    assert torch.equal(case.b[n110], unit.b[n110] * 2.0 ** 110) and torch.equal(case.w[n110], unit.w[n110] * 2.0 ** 110)


# --------------------------------------------------------------------------- the finding, pinned
def _boundary_rows():
    """32 rows of K = 16 (the smallest pack_mk_weights takes): row 0 with max|w| = 2^-113, row 1 with the fp32 number
    below it, row 2 with fp32's smallest subnormal as its only nonzero, the rest unit-scale."""
    w = rnd(32, 16, seed=251)
    tail = torch.tensor([0.5, -0.75, 0.0, 0.375])
    for r, top in ((0, 2.0 ** -113), (1, 2.0 ** -113 * (1 - 2.0 ** -24))):
        w[r] = 0.0
        w[r, 3] = top
        w[r, 4:8] = tail * 2.0 ** -113
    w[2] = 0.0
    w[2, 9] = 2.0 ** -149
    assert w[0].abs().max() == 2.0 ** -113 and w[1].abs().max() < 2.0 ** -113 and w[2, 9] > 0
    return w


# what the bounded scale 2^126 gives, exactly: (1 / s, hi, lo) at the columns 3 .. 7 (row 2: column 9)
BOUNDARY = {
    0: (2.0 ** -126, [2.0 ** 13, 2.0 ** 12, -0.75 * 2.0 ** 13, 0.0, 0.375 * 2.0 ** 13], [0.0] * 5),
    1: (2.0 ** -126, [2.0 ** 13, 2.0 ** 12, -0.75 * 2.0 ** 13, 0.0, 0.375 * 2.0 ** 13], [-2.0 ** -11, 0, 0, 0, 0]),
    2: (2.0 ** -126, [2.0 ** -23], [0.0]),
}


@pytest.mark.parametrize("routine", ["prep_split", "pack_mk_weights", "emulation"])
@pytest.mark.parametrize("row", [0, 1, 2], ids=["at-2^-113", "below-2^-113", "smallest-subnormal"])
def test_rows_at_the_threshold(lib, routine, row):
    """max|w_r| = 2^-113 would take s = 2^127 (1 / s subnormal), anything smaller s >= 2^128 = inf: with the exponent
    bounded at 126 all three rows split exactly (every value below is a small multiple of fp16's spacing)."""
    w = _boundary_rows()
    if routine == "prep_split":
        hi, lo, b16, sinv = cpp_split(lib, w)
        assert torch.isfinite(b16[row].float()).all(), b16[row]
        assert torch.equal(b16[row, :16].double(), hi[row, :16].double())       # 3 significant bits: exact in bf16
    elif routine == "pack_mk_weights":
        pk, sinv = cpp_pack(lib, w)
        hi, lo = (pk[0, 0, :, s].reshape(2, 32, 8).permute(1, 0, 2).reshape(32, 16) for s in (slice(0, 8), slice(8, 16)))
    else:
        hi, lo, sinv = E.split_weights(w)
    cols = slice(9, 10) if row == 2 else slice(3, 8)
    want_sinv, want_hi, want_lo = BOUNDARY[row]
    assert torch.isfinite(hi[row].float()).all() and torch.isfinite(lo[row].float()).all(), (hi[row], lo[row])
    assert float(sinv[row]) == want_sinv, float(sinv[row])
    assert hi[row, cols].tolist() == want_hi and lo[row, cols].tolist() == want_lo, (hi[row, cols], lo[row, cols])
    rest = torch.ones(16, dtype=torch.bool)
    rest[cols] = False
    assert not bits(hi[row, rest]).any() and not bits(lo[row, rest]).any()        # the row's zeros stay +0
    assert torch.equal(hi[row].double() + lo[row].double(), w[row].double() / want_sinv)


# --------------------------------------------------------------------------- site census
# Every call of prep_split and pack_mk_weights in the Weights constructor (runtime.cpp: build_trunk, prep_qkv, build,
# pack_mk), by the parameter it reads. pack_mk packs Linears that prep_linear has split already, so its sites are among
# these; the fused bev_proj image is bev_proj.0's columns 256 .. 319 (all rows), tf_cakv the multihead_attn rows d .. 3d.
SPLIT_CALL_SITES = [
    r"_backbone\.(image|lidar)_encoder\.conv1\.weight",                                  # the stems, bn1 folded
    r"_backbone\.(image|lidar)_encoder\.layer\d\.\d\.conv[12]\.weight",                  # BasicBlocks
    r"_backbone\.(image|lidar)_encoder\.layer\d\.0\.downsample\.0\.weight",
    r"_backbone\.transformers\.\d\.blocks\.\d\.attn\.(query|key|value)\.weight",         # prep_qkv
    r"_backbone\.transformers\.\d\.blocks\.\d\.attn\.proj\.weight",
    r"_backbone\.transformers\.\d\.blocks\.\d\.mlp\.[02]\.weight",
    r"_backbone\.(lidar_channel_to_img|img_channel_to_lidar)\.\d\.weight",
    r"_backbone\.(up_conv5|up_conv4|c5_conv)\.weight",
    r"_bev_downscale\.weight", r"_status_encoding\.weight", r"_bev_semantic_head\.[02]\.weight",
    r"_tf_decoder\.layers\.\d\.(self_attn|multihead_attn)\.in_proj_weight",              # sa_in; ca_q, ca_kv, tf_cakv
    r"_tf_decoder\.layers\.\d\.(self_attn|multihead_attn)\.out_proj\.weight",
    r"_tf_decoder\.layers\.\d\.linear[12]\.weight",
    r"_agent_head\._mlp_states\.[02]\.weight", r"_agent_head\._mlp_label\.0\.weight",
    r"_trajectory_head\.plan_anchor_encoder\.[03]\.weight", r"_trajectory_head\.time_mlp\.[13]\.weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.cross_bev_attention\.(attention_weights|output_proj|value_proj\.0)\.weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.cross_(agent|ego)_attention\.in_proj_weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.cross_(agent|ego)_attention\.out_proj\.weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.ffn\.[02]\.weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.time_modulation\.scale_shift_mlp\.1\.weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.task_decoder\.plan_cls_branch\.[036]\.weight",
    r"_trajectory_head\.diff_decoder\.layers\.\d\.task_decoder\.plan_reg_branch\.[024]\.weight",
    r"bev_proj\.0\.weight",
]
# Sites dead_rows leaves alone, each with its reason.
EXEMPT = [
    # one row: the logits of all 20 modes would become the bias, the argmax over them a 20-way tie and the selected
    # trajectory arbitrary - no truth to hold the device to. The rowrange op cases cover a dead last row.
    r"_trajectory_head\.diff_decoder\.layers\.\d\.task_decoder\.plan_cls_branch\.6\.weight",
    # one row: every agent's label logit would be the bias; nothing of the site would be left to compare.
    r"_agent_head\._mlp_label\.0\.weight",
]
# the sites the forward tests must reach at the least
REQUIRED = ["blocks.0.mlp.0.", "blocks.1.attn.proj.", "attn.query.", "attn.key.", "attn.value.",
            "_tf_decoder.layers.0.linear1.", "_tf_decoder.layers.2.self_attn.in_proj_weight",
            "_tf_decoder.layers.1.multihead_attn.in_proj_weight", "diff_decoder.layers.0.ffn.0.",
            "plan_reg_branch.0.", "value_proj.0.", "bev_proj.0.", "_bev_downscale."]


@pytest.fixture(scope="module")
def dead(seeded_sd):
    return R.dead_rows(seeded_sd)


def test_dead_rows_reach_every_split_site(seeded_sd, dead):
    """Every weight tensor of the dict that a split reads is one of the constructor's call sites and the other way round
    (2 x 36 trunk convs and all), and ``dead_rows`` edits at least one row the forward reads at each, the exemptions
    aside; the edits are the stated ones and touch no bias."""
    sd, edits = dead
    sites = R.split_sites(seeded_sd)
    keys = [k for k, _, _, _ in sites]
    for k in keys:
        assert sum(bool(re.fullmatch(p, k)) for p in SPLIT_CALL_SITES) == 1, k
    for p in SPLIT_CALL_SITES + EXEMPT:
        assert any(re.fullmatch(p, k) for k in keys), p
    assert sum(".conv" in k and "_encoder.layer" in k for k in keys) == 64 and len(R.basic_blocks(seeded_sd)) == 32
    for k, bn, row0, rows in sites:
        if any(re.fullmatch(p, k) for p in EXEMPT):
            assert k not in edits and np.array_equal(sd[k], seeded_sd[k]), k
            continue
        assert edits.get(k), k
        assert all(row0 <= r < row0 + rows for r, _ in edits[k]), (k, edits[k])
        if bn is not None:
            g, v = sd[bn + ".weight"], sd[bn + ".running_var"]
            assert sorted(g[[r for r, what in edits[k] if what.startswith("gamma")]].tolist()) == sorted(
                np.float32(R.DEAD_GAMMAS).tolist()), k
            var = v[[r for r, what in edits[k] if what.startswith("var")]].tolist()
            assert sorted(set(var)) == sorted(np.float32(R.DEAD_VARS).tolist()), k
            assert len(var) == 2 + k.endswith(R.DEAD_LIVE_VAR0), (k, var)        # a live var = 0 channel where listed
            assert np.array_equal(sd[k], seeded_sd[k])
        else:
            scales = {what for _, what in edits[k]}
            assert len(scales) == len(R.DEAD_ROW_SCALES), (k, scales)
            for r, what in edits[k]:
                c = np.float32(float(what.split(" x ")[1]))
                assert np.array_equal(sd[k][r], np.asarray(seeded_sd[k])[r] * c), (k, r)
                assert (np.abs(sd[k][r]).max() < 2.0 ** -113) and np.abs(np.asarray(seeded_sd[k])[r]).max() > 2.0 ** -20
    for k in seeded_sd:
        if k.endswith("bias") or k.endswith(".running_mean"):
            assert np.array_equal(sd[k], seeded_sd[k]), k
    for need in REQUIRED:
        assert any(need in k for k in edits), need


def test_dead_rows_fold_below_the_threshold(seeded_sd, dead):
    """What prep_conv hands the split at a BasicBlock: the 2^-118, 2^-130 and -2^-120 gammas fold to rows under
    2^-113, the zero gamma to a zero row, 2^-100 (the control) to a row above it."""
    sd, edits = dead
    conv = "_backbone.image_encoder.layer1.0.conv1"
    rows = folded_conv_rows(sd, conv, conv[:-5] + "bn1").abs().amax(1)
    by = {what: r for r, what in edits[conv + ".weight"]}
    assert rows[by["gamma 0.0"]] == 0
    assert 2.0 ** -113 < rows[by[f"gamma {2.0 ** -100!r}"]] < 2.0 ** -95
    for g in (2.0 ** -118, 2.0 ** -130, -2.0 ** -120):
        assert 0 < rows[by[f"gamma {g!r}"]] < 2.0 ** -113, g


# --------------------------------------------------------------------------- premise of the forward tests
@pytest.fixture(scope="module")
def five():
    from diffusiondrive_amd.weights import synthetic_inputs
    return synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED)


@pytest.fixture(scope="module")
def dead_truth(dead, five):
    return U.oracle_run(dead[0], five)


def _worst(got, ref):
    e = U.errors({k: got[k] for k in ref}, ref)
    name = max(e, key=lambda k: e[k] / U.bar_of(k, BARS))
    return e, name, e[name] / U.bar_of(name, BARS)


def test_dead_rows_change_the_function_and_stay_finite(seeded_sd, five, dead_truth):
    """The float64 oracle on dead_rows is finite and is not the float64 oracle on the seeded dict: the edits reach
    the trunks' output, the keyval tokens, the decoded queries, the BEV features and the trajectory."""
    base = U.oracle_run(seeded_sd, five)
    for k, v in dead_truth.items():
        assert np.isfinite(v).all(), k
    for k in ("img_l4", "bev_feature", "keyval", "query_out", "cross_bev", "trajectory", "agent_states", "poses_reg"):
        assert np.abs(dead_truth[k] - base[k]).max() > 1e-3, k


def test_fp32_oracle_on_dead_rows_stays_inside_half_of_every_bar(dead, five, dead_truth):
    """The function on dead_rows is as well conditioned as the bars assume: plain fp32 is within half of each.
    DEAD_ROWS_PER_SCALE is the count this holds at."""
    e, name, frac = _worst(U.oracle_run(dead[0], five, dtype=np.float32), dead_truth)
    print(f"dead_rows fp32 oracle vs float64: worst {name} {e[name]:.3e} = {frac:.2f} of its bar; "
          + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert frac <= 0.5, (name, e[name])


def test_emulated_f16x3_oracle_on_dead_rows_stays_inside_half_of_every_bar(dead, five, dead_truth):
    """The documented f16x3 arithmetic, with the split's exponent bounded, on dead_rows: within half of every bar -
    what the device is asked for in test_weight_range_gpu.py is what its arithmetic can give."""
    with E.emulated_f16x3_oracle():
        em = U.oracle_run(dead[0], five, dtype=np.float32)
    for k, v in em.items():
        assert np.isfinite(v).all(), k
    e, name, frac = _worst(em, dead_truth)
    print(f"dead_rows emulated f16x3 vs float64: worst {name} {e[name]:.3e} = {frac:.2f} of its bar; "
          + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert frac <= 0.5, (name, e[name])
