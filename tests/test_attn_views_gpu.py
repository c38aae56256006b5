"""The small MHA, the BEV sampling family and the pooling kernels on the operand forms the forward launches - q | k | v
windows of one buffer, interleaved K | V, K / V shared by kv_div scenes, `samples` scenes per value map, a non-square
map, the pooled tokens stored into the GPT slab plus the position rows - through dd_op_mha_small_view,
dd_op_bev_sample_attn_s, dd_op_bev_taps, dd_op_bev_sample_attn_gathered and dd_op_avgpool_view, and the stem / max
pooling at odd sizes through their dense entries; every operand inside poisoned guards (tests/guard_util.py).

Each case follows the procedure of test_op_views_gpu.py:
* the call runs twice - NaN, then 3e38 in every input guard and gap word - and the two bodies must agree bit for bit;
* check() on every output: no guard or gap word changed;
* the body against a float64 restatement from the plain definition (attn_views_util.py) at test_ops_gpu.py's bars
  through its close(): 1e-5 (MHA, sampling, gathered), 1e-6 (avgpool), 3e-5 (the f16x3 stem; 1e-4 against
  bf16-rounded operands for its bf16 form), exact (maxpool), each of 1 + max|ref|;
* the discrete tables (rows, slots) against the float32 restatement of the tap geometry (decoder_edge_util.py).

tests/test_attn_views.py shows on the CPU that the same inputs and comparisons reject one deliberate fault each.
DESIGN.md §19 has one row per case with the measured error; each test prints its row (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_views_util as U
from decoder_edge_util import check_gathered_taps, tap_pixels
from diffusiondrive_amd import _lib
from guard_util import POISON, SENTINEL, dense_strides, guarded
from test_op_views_gpu import bits_equal
from test_ops_gpu import DEV, _mha_lds_bytes, close, g, nans, ok

pytestmark = pytest.mark.gpu

NAN = float("nan")


def twice(run):
    """run(poison) -> {name: dense body, every output checked}. The NaN run and the 3e38 run must agree bit for bit;
    returns the NaN run."""
    a, b = run(NAN), run(POISON)
    assert a.keys() == b.keys()
    for name in a:
        if torch.is_tensor(a[name]):
            assert bits_equal(a[name], b[name]), f"{name} depends on what lies outside the operands"
        else:
            assert a[name] == b[name], name
    return a


def report(name, shape, form, kernel, err, bar, ref, words):
    lim = bar * (1.0 + ref.abs().max().item())
    print(f"\nATTNVIEW | {name} | {shape} | {form} | {kernel} | {err:.2e} / {lim:.2e} | {words}")


def as_int(t):
    """An int32 table stored into a (float32) guarded operand."""
    return t.contiguous().view(torch.int32).cpu().numpy()


# ------------------------------------------------------------------------------------------------------- MHA
def mha_launch(gpu, o, out=None):
    out = o.O if out is None else out
    at = lambda G, off: G.t.data_ptr() + 4 * off  # noqa: E731
    ok(gpu.dd_op_mha_small_view(at(o.Q, o.q_off), o.ldq, o.qbs, at(o.KV, o.k_off), at(o.KV, o.v_off), o.ldkv, o.kvbs,
                                out.ptr(), o.ldo, o.obs, o.B, o.Lq, o.Lk, o.nh, o.hd, o.kv_div, None), gpu)


def mha_twice(gpu, name):
    def run(poison):
        o = U.mha_operands(name, poison, DEV)
        mha_launch(gpu, o)
        run.o = o
        return {"out": o.O.check()}

    return twice(run)["out"], run.o


MHA_FORM = {"M1": "q | k | v windows of (2, 31, 768)", "M2": "q dense, K | V interleaved (3, 65, 512)",
            "M3": "K | V (2, 30, 512) shared by kv_div = 3 scenes", "M1'": "M1 with ld + 8, batch stride + 1 row",
            "M2'": "M2 with ld + 8, batch stride + 1 row", "M4": "nh 3, kv_div 2, K | V ldkv 200",
            "M4-hd48": "hd 48, nh 1, Lk 127, ldq / ldo 56, ldkv 104"}


@pytest.mark.parametrize("name", list(MHA_FORM))
def test_mha_small_on_strided_views(gpu, name):
    """launch_mha_small on the three forms of the forward (M1 - M3), the same with gap words between rows and scenes
    (M1', M2'), and the per-row fallback kernel with an interleaved, shared K | V (M4) and hd = 48 (the d < hd bound of
    its P.V pass, Lk = 127: the second key of a lane partly present), against softmax in float64. M3: scenes 0 and 3
    equal scenes 0 and 1 of the kv_div = 1 launch on the same K / V to the bit."""
    out, o = mha_twice(gpu, name)
    assert (o.ldq, o.ldkv, o.ldo) == U.MHA_LD[name]
    fallback = name.startswith("M4")
    assert (_mha_lds_bytes(o.hd, o.Lq, o.Lk) > 64 * 1024) == fallback
    if name == "M4":  # 786 items: the last workgroup of 4 waves has two inactive ones
        assert o.B * o.nh * o.Lq == 786 and 786 % 4 == 2
    ref = U.mha_ref(o.q, o.k, o.v, o.nh, o.kv_div)
    err = (out.cpu().double() - ref).abs().max().item()
    report(name, (o.B, o.Lq, o.Lk, o.nh, o.hd), MHA_FORM[name], "mha_small_kernel" if fallback else "mha_head_kernel",
           err, 1e-5, ref, o.O.guard_words)
    close(out, ref, 1e-5)
    if name == "M3":
        one, o1 = mha_twice(gpu, "M3-div1")
        assert torch.equal(o1.k, o.k) and torch.equal(o1.v, o.v) and torch.equal(o1.q, o.q[[0, 3]])
        close(one, U.mha_ref(o1.q, o1.k, o1.v, o1.nh, 1), 1e-5)
        assert bits_equal(out[[0, 3]], one), "a scene's result depends on kv_div"


def test_harness_reports_a_head_outside_the_declared_view(gpu):
    """The file can fail: M2' with the output declared one head narrower than the launch writes (224 of 256 channels,
    row stride 264) - the eighth head lands in gap words and check() raises; the declared heads are right."""
    o = U.mha_operands("M2'", NAN, DEV)
    narrow = guarded((o.B, o.Lq, o.d - o.hd), (o.obs, o.ldo, 1), SENTINEL, device=DEV)
    mha_launch(gpu, o, narrow)
    want = [b * o.obs + i * o.ldo + c for b in range(o.B) for i in range(o.Lq) for c in range(o.d - o.hd, o.d)]
    assert narrow.dirty() == want
    with pytest.raises(AssertionError, match="overwritten"):
        narrow.check()
    close(narrow.view(), U.mha_ref(o.q, o.k, o.v, o.nh, 1)[..., :o.d - o.hd], 1e-5)


# --------------------------------------------------------------------------------------------------- sampling
def G_in(values, poison):
    return guarded(tuple(values.shape), dense_strides(tuple(values.shape)), poison, values=values, device=DEV)


def G_out(shape):
    return guarded(shape, dense_strides(shape), SENTINEL, device=DEV)


@pytest.mark.parametrize("geom,one_map_per_scene", [("forward", False), ("forward", True), ("nonsquare", False),
                                                    ("nonsquare", True)],
                         ids=["forward-S3", "forward-S1", "nonsquare-S2", "nonsquare-S1"])
def test_bev_sampling_family(gpu, geom, one_map_per_scene):
    """bev_sample_attn with `samples` scenes per map against grid_sample in float64; bev_tap_rows against the float32
    restatement of the tap geometry; the dedup's invariants (pixel order, count, -1 tail, slots consistent with rows,
    the row base the decoder scene's while the pixel's image is b / samples); and the gathered form, on rows gathered
    on the host from the dense map by the device's own tables, equal to the dense form bit for bit with and without
    slots (decoder.hip is built without fp contraction; both kernels add the taps in the order nw, ne, sw, se)."""
    c = U.sample_case(geom)
    D, Q, P, Hv, Wv, C, sx, sy = (c[x] for x in ("D", "Q", "P", "Hv", "Wv", "C", "inv_max_x", "inv_max_y"))
    S = 1 if one_map_per_scene else c["S"]
    Dm, n4 = D // S, D * Q * P * 4
    logits, pts, value = c["logits"], c["pts"], c["value"][:Dm].contiguous()
    # the condition the discrete comparisons need (also held on the CPU in test_attn_views.py)
    ix64, iy64 = U.pixel_coords64(pts.numpy(), c)
    away = np.minimum(np.abs(ix64 - np.rint(ix64)), np.abs(iy64 - np.rint(iy64)))
    assert (away[c["random_mask"]] >= U.MIN_PX).all()
    vflat = value.reshape(Dm * Hv * Wv, C)

    def gather(rows):
        v = torch.full((len(rows), C), NAN)
        live = rows >= 0
        v[torch.from_numpy(live)] = vflat[torch.from_numpy(rows[live]).long()]
        return v

    def run(poison):
        L, Pt, Vm = G_in(logits, poison), G_in(pts, poison), G_in(value, poison)
        O = G_out((D, Q, C))
        ok(gpu.dd_op_bev_sample_attn_s(L.ptr(), Pt.ptr(), Vm.ptr(), O.ptr(), D, Q, P, Hv, Wv, C, S, sx, sy, None), gpu)
        res = {"dense": O.check()}
        R, R2, SL = G_out((n4,)), G_out((n4,)), G_out((n4,))
        assert gpu.dd_op_bev_taps(Pt.ptr(), R.ptr(), None, D, Q, P, Hv, Wv, sx, sy, S, None) == 1
        assert gpu.dd_op_bev_taps(Pt.ptr(), R2.ptr(), SL.ptr(), D, Q, P, Hv, Wv, sx, sy, S, None) == 1
        torch.cuda.synchronize()
        res["rows"], res["rows_dedup"], res["slots"] = R.check(), R2.check(), SL.check()
        # the gathered rows: the dense map's own rows (padded slots NaN) in a guarded (n4, C) array
        for key, rows, slots in (("gathered", as_int(res["rows"]), None),
                                 ("gathered_dedup", as_int(res["rows_dedup"]), SL)):
            assert ((rows >= -1) & (rows < Dm * Hv * Wv)).all()
            VR, O2 = G_in(gather(rows), poison), G_out((D, Q, C))
            ok(gpu.dd_op_bev_sample_attn_gathered(L.ptr(), Pt.ptr(), VR.ptr(), slots.ptr() if slots else None,
                                                  O2.ptr(), D, Q, P, Hv, Wv, C, sx, sy, None), gpu)
            res[key] = O2.check()
        res["words"] = O.guard_words + R.guard_words + R2.guard_words + SL.guard_words
        return res

    r = twice(run)
    ref = U.sample_ref(logits, pts, c["value"], S, c)
    err = (r["dense"].cpu().double() - ref).abs().max().item()
    pix, _, _ = tap_pixels(pts.numpy(), D, Q, P, Hv, Wv, S, sx, sy)
    report(f"sampling {geom}", (D, S, Q, P, Hv, Wv, C), f"samples {S}, scales {sx:g} / {sy:g}",
           "bev_sample_attn + tap_rows + tap_dedup + gathered", err, 1e-5, ref, r["words"])
    print(f"    padded taps {int((pix < 0).sum())} of {pix.size}, redrawn points {c['redrawn']}")
    close(r["dense"], ref, 1e-5)
    rows, rows_d, slots = as_int(r["rows"]), as_int(r["rows_dedup"]), as_int(r["slots"])
    assert np.array_equal(rows, pix), "bev_tap_rows differs from the restatement"
    padded, live, _ = check_gathered_taps(pts.numpy(), rows_d, slots, None, None, None, D, 0.0, Q, P, Hv, Wv, S, sx, sy)
    assert padded == int((pix < 0).sum()) and live == int((pix >= 0).sum())
    cap = Q * P * 4
    per_scene = (rows_d.reshape(D, cap) >= 0).sum(1)
    assert per_scene[D - 1] == 0 and per_scene[D - 2] == 4 and (per_scene[:D - 2] > 4).all()
    assert (pix.reshape(D, cap)[D - 1] == -1).all()
    assert bits_equal(r["gathered"], r["dense"]), "the gathered form (own rows) differs from the dense form"
    assert bits_equal(r["gathered_dedup"], r["dense"]), "the gathered form (dedup slots) differs from the dense form"


def test_bev_tap_dedup_refuses_a_map_beyond_its_table(gpu):
    """Hv Wv > 4096: dd_op_bev_taps returns 0 with slots and writes neither table; without slots it launches."""
    D, Q, P, Hv, Wv = 1, 2, 2, 65, 64
    pts = G_in(U.rnd(D, Q, P, 2, seed=441, scale=10.0), NAN)
    R, SL = G_out((D * Q * P * 4,)), G_out((D * Q * P * 4,))
    assert gpu.dd_op_bev_taps(pts.ptr(), R.ptr(), SL.ptr(), D, Q, P, Hv, Wv, 1 / 32, 1 / 32, 1, None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(R.check()).all() and torch.isnan(SL.check()).all()
    assert gpu.dd_op_bev_taps(pts.ptr(), R.ptr(), None, D, Q, P, Hv, Wv, 1 / 32, 1 / 32, 1, None) == 1
    torch.cuda.synchronize()
    pix, _, _ = tap_pixels(pts.view().cpu().numpy(), D, Q, P, Hv, Wv, 1, 1 / 32, 1 / 32)
    assert np.array_equal(as_int(R.check()), pix)


# ---------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("C", [64, 36])
def test_p1_image_tokens_into_the_slab(gpu, C):
    """fuse(): the 16 x 64 image map pooled 8 x 32 into rows 0..255 of every scene's (320, C) slab plus the position
    rows 0..255 of the (320, C) table; rows 256..319 keep the sentinel. Bit-identical to dd_op_avgpool followed by an
    fp32 add of the rows (elementwise.hip is built without fp contraction), and against float64. C = 36: 1152 stores
    per output row in 5 blocks of 256 (the i < n bound); C = 64: 8 full blocks."""
    B, H, W, oh, ow = 2, 16, 64, 8, 32
    x, pos = U.pool_case(B, H, W, C, 451)
    ref = U.pool_ref(x, oh, ow, pos[:oh * ow])

    def run(poison):
        X, Ps = G_in(x, poison), G_in(pos, poison)
        _, Tk = U.token_slab(B, C, oh, ow, DEV)
        v = _lib.DDOpView(Tk.ptr(), U.T * C, ow * C, C, 1)
        ok(gpu.dd_op_avgpool_view(X.ptr(), B, H, W, C, oh, ow, ctypes.byref(v), Ps.ptr(), None), gpu)
        return {"tok": Tk.check(), "words": Tk.guard_words}

    r = twice(run)
    err = (r["tok"].cpu().double() - ref).abs().max().item()
    report("P1", (B, H, W, C, oh, ow), "out = slab rows 0..255 (T C apart), add = position rows", "avgpool", err, 1e-6,
           ref, r["words"])
    close(r["tok"], ref, 1e-6)
    xd, pd, sep = g(x), g(pos), nans(B, oh, ow, C)
    ok(gpu.dd_op_avgpool(xd.data_ptr(), B, H, W, C, oh, ow, sep.data_ptr(), None), gpu)
    assert bits_equal(r["tok"], sep + pd[:oh * ow].view(oh, ow, C))


@pytest.mark.parametrize("Cl", [64, 36])
def test_p2_lidar_tokens_dense(gpu, Cl):
    """fuse(): the 16 x 16 LiDAR map pooled 8 x 8 into a dense buffer, no add, inside guards."""
    B, H, W, oh, ow = 2, 16, 16, 8, 8
    x, _ = U.pool_case(B, H, W, Cl, 461)
    ref = U.pool_ref(x, oh, ow)

    def run(poison):
        X, O = G_in(x, poison), G_out((B, oh, ow, Cl))
        v = _lib.DDOpView(O.ptr(), *dense_strides((B, oh, ow, Cl)))
        ok(gpu.dd_op_avgpool_view(X.ptr(), B, H, W, Cl, oh, ow, ctypes.byref(v), None, None), gpu)
        return {"out": O.check(), "words": O.guard_words}

    r = twice(run)
    err = (r["out"].cpu().double() - ref).abs().max().item()
    report("P2", (B, H, W, Cl, oh, ow), "dense out, no add", "avgpool", err, 1e-6, ref, r["words"])
    close(r["out"], ref, 1e-6)


@pytest.mark.parametrize("B,H,W,C", [(2, 37, 50, 64), (1, 5, 7, 4)])
def test_p3_maxpool_inside_guards(gpu, B, H, W, C):
    """maxpool 3 x 3 / 2 at odd sizes on an all-negative map: a window tap past the image that a 0 or -inf stands in
    for, or a row read past the last image row (NaN / 3e38 there), changes the maximum; exact."""
    x = -(U.rnd(B, H, W, C, seed=471).abs() + 0.1)
    ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = ref.shape[1:3]
    assert (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1) and ref.max().item() < 0

    def run(poison):
        X, O = G_in(x, poison), G_out((B, Ho, Wo, C))
        ok(gpu.dd_op_maxpool3x3s2(X.ptr(), B, H, W, C, O.ptr(), None), gpu)
        return {"out": O.check(), "words": O.guard_words}

    r = twice(run)
    err = (r["out"].cpu().double() - ref).abs().max().item()
    report("P3", (B, H, W, C), "dense in guards, all negative", "maxpool", err, 0.0, ref, r["words"])
    close(r["out"], ref, 0.0)


STEM_SHAPES = [(1, 40, 72), (2, 37, 50)]
STEM_BAR = {0: 3e-5, 1: 1e-4}  # f16x3; bf16 against bf16-rounded operands


def stem_weights(C, seed):
    w = U.rnd(64, 4, 7, 7, seed=seed, scale=1.0 / np.sqrt(49 * C))
    w[:, C:] = 0.0  # the taps of the channels the input does not have
    return w, U.rnd(64, seed=seed + 1)


def stem_ref(x_nchw, w, b, prec):
    xr, wr = (x_nchw.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()) if prec else (x_nchw.double(), w.double())
    ref = F.max_pool2d(F.relu(F.conv2d(xr, wr[:, :x_nchw.shape[1]], b.double(), 2, 3)), 3, 2, 1)
    return ref.permute(0, 2, 3, 1).contiguous()


def stem_case(gpu, name, form, shape, x_nchw, w, b, prec, call):
    """call(poison, out ptr, flags ptr) launches one stem entry on its guarded input; the pooled output sits inside
    guards; flags stay 0 in both runs."""
    ref = stem_ref(x_nchw, w, b, prec)

    def run(poison):
        O = G_out(tuple(ref.shape))
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        call(poison, O.ptr(), flags.data_ptr())
        return {"out": O.check(), "flags": int(flags.item()), "words": O.guard_words,
                "kernel": gpu.dd_op_last_kernel().decode()}

    r = twice(run)
    err = (r["out"].cpu().double() - ref).abs().max().item()
    report(name, shape, form, r["kernel"], err, STEM_BAR[prec], ref, r["words"])
    assert r["flags"] == 0
    close(r["out"], ref, STEM_BAR[prec])


@pytest.mark.parametrize("prec", [0, 1], ids=["f16x3", "bf16"])
@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_p4_stem_pool_nhwc(gpu, B, H, W, prec):
    """dd_op_stem_pool on the fp32 (B, H, W, 4) input (channel 3 zero) at odd sizes."""
    x = U.rnd(B, 4, H, W, seed=481).abs()
    x[:, 3] = 0.0
    w, b = stem_weights(4, 482)
    wd, bd = g(w.permute(0, 2, 3, 1)), g(b)

    def call(poison, out, flags):
        X = G_in(x.permute(0, 2, 3, 1).contiguous(), poison)
        ok(gpu.dd_op_stem_pool(X.ptr(), B, H, W, wd.data_ptr(), bd.data_ptr(), out, prec, flags, None), gpu)

    stem_case(gpu, "P4 stem_pool", "fp32 NHWC in guards", (B, H, W, 4), x, w, b, prec, call)


@pytest.mark.parametrize("prec", [0, 1], ids=["f16x3", "bf16"])
@pytest.mark.parametrize("C,one", [(1, False), (1, True), (2, False), (3, False)])
@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_p4_stem_pool_nchw(gpu, monkeypatch, B, H, W, C, one, prec):
    """dd_op_stem_pool_nchw on the (B, C, H, W) tensor read in place, C = 1..3 (C = 1 also in the opt-in one-channel
    kernel form)."""
    monkeypatch.setenv("DDMI_STEM1", "1" if one else "0")
    x = U.rnd(B, C, H, W, seed=485).abs()
    w, b = stem_weights(C, 486)
    wd, bd = g(w.permute(0, 2, 3, 1)), g(b)

    def call(poison, out, flags):
        X = G_in(x, poison)
        ok(gpu.dd_op_stem_pool_nchw(X.ptr(), B, C, H, W, wd.data_ptr(), bd.data_ptr(), out, prec, flags, None), gpu)

    stem_case(gpu, "P4 stem_pool_nchw", f"fp32 NCHW C = {C} in guards" + (", one-channel form" if one else ""),
              (B, C, H, W), x, w, b, prec, call)


@pytest.mark.parametrize("layout,C", [("hwc", 3), ("planar", 1), ("planar", 3)])
@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_p4_stem_pool_u8(gpu, monkeypatch, B, H, W, layout, C):
    """dd_op_stem_pool_u8 in both layouts: the bytes sit between 64 KiB of 0xFF on either side, the body uses bytes
    0..254 and lut[255] holds NaN / 3e38, so a guard byte that reaches the arithmetic shows."""
    monkeypatch.setenv("DDMI_STEM1", "0")
    gen = torch.Generator().manual_seed(491 + C)
    shape = (B, H, W, C) if layout == "hwc" else (B, C, H, W)
    xb = torch.randint(0, 255, shape, generator=gen, dtype=torch.uint8)
    lut = torch.rand(256, generator=gen)
    wide = lut[xb.long()]
    x = (wide.permute(0, 3, 1, 2) if layout == "hwc" else wide).contiguous()
    w, b = stem_weights(C, 492)
    wd, bd = g(w.permute(0, 2, 3, 1)), g(b)
    guard = 1 << 16

    def call(poison, out, flags):
        raw = torch.full((2 * guard + xb.numel(),), 0xFF, dtype=torch.uint8, device=DEV)
        raw[guard:guard + xb.numel()] = xb.reshape(-1).to(DEV)
        lp = lut.clone()
        lp[255] = poison
        ld = g(lp)
        ok(gpu.dd_op_stem_pool_u8(raw.data_ptr() + guard, 0 if layout == "hwc" else 1, B, C, H, W, ld.data_ptr(),
                                  wd.data_ptr(), bd.data_ptr(), out, 0, flags, None), gpu)

    stem_case(gpu, "P4 stem_pool_u8", f"uint8 {layout} C = {C} between 0xFF bytes", shape, x, w, b, 0, call)
