"""The cases of tests/test_attn_views_gpu.py held to their purpose, on the CPU: numpy restatements of the strided
operations (tests/attn_views_util.py) run on the same guarded operands, each with one deliberate fault - the K / V
batch taken as b % kv_div, the interleaved buffer walked with ldkv = d, v read at k's offset, the value map taken as b
for b / S, the dedup's row base taken from b / S, Hv and Wv exchanged, the two scales exchanged, the position-row
offset dropped, a store one channel past C - and the comparison or check() the GPU file applies must reject every one
and accept the correct form. No device is needed and no kernel is run wrong on purpose: "would this test notice" is
answered here. Also held: the conditions the point sets are built to (1e-3 px from every pixel boundary for the random
points, the hand-placed points exact in fp32), and that the new entries are declared, bound and refuse null
arguments by name before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attn_views_util as U
from decoder_edge_util import check_gathered_taps, tap_pixels
from guard_util import POISON, SENTINEL, guarded
from test_ops_gpu import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
ENTRIES = ("dd_op_mha_small_view", "dd_op_bev_sample_attn_s", "dd_op_bev_taps", "dd_op_bev_sample_attn_gathered",
           "dd_op_avgpool_view")


def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


# ------------------------------------------------------------------------------------------------ the entries
def test_entries_are_declared_bound_and_refuse_null_arguments_by_name():
    from diffusiondrive_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddmi.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        args = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1).split(",")
        res, argtypes = _lib._SIGS[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), (name, args)
        for a, t in zip(args, argtypes):
            want = (ctypes.c_int64 if "int64_t" in a else ctypes.c_float if a.split()[0] == "float" else
                    ctypes.c_int if a.split()[0] == "int" and "*" not in a else None)
            assert want is None or t is want, (name, a, t)
    v = _lib.DDOpView()
    calls = {
        "dd_op_mha_small_view": (None, 8, 8, None, None, 8, 8, None, 8, 8, 1, 1, 1, 1, 8, 1, None),
        "dd_op_bev_sample_attn_s": (None, None, None, None, 1, 1, 1, 4, 4, 4, 1, 1.0, 1.0, None),
        "dd_op_bev_taps": (None, None, None, 1, 1, 1, 4, 4, 1.0, 1.0, 1, None),
        "dd_op_bev_sample_attn_gathered": (None, None, None, None, None, 1, 1, 1, 4, 4, 4, 1.0, 1.0, None),
        "dd_op_avgpool_view": (None, 1, 2, 2, 4, 1, 1, ctypes.byref(v), None, None),
    }
    for name, a in calls.items():
        assert getattr(lib, name)(*a) == -1, name
        msg = lib.dd_op_last_error()
        assert name.encode() in msg and b"null" in msg, msg


# ------------------------------------------------------------------------------------------------------- MHA
@pytest.mark.parametrize("name", [n for n in U.MHA_CASES if n != "M3-div1"])
def test_mha_cases_accept_the_launcher_addressing(name):
    """The correct restatement on the guarded operands equals the plain definition; the leading dimensions are the
    ones the cases were specified with; and what lies outside the operands does not reach the result."""
    o = U.mha_operands(name, NAN)
    assert (o.ldq, o.ldkv, o.ldo) == U.MHA_LD[name]
    assert (U.mha_lds_bytes(o.hd, o.Lq, o.Lk) > 64 * 1024) == name.startswith("M4")
    ref = U.mha_ref(o.q, o.k, o.v, o.nh, o.kv_div)
    out = U.mha_strided(o)
    close(torch.from_numpy(out), ref, 1e-5)
    assert np.array_equal(out, U.mha_strided(U.mha_operands(name, POISON)))
    # distinct per scene and per K / V batch
    assert all(not torch.equal(o.q[0], o.q[b]) for b in range(1, o.B))
    assert all(not torch.equal(o.k[0], o.k[b]) and not torch.equal(o.v[0], o.v[b]) for b in range(1, o.k.shape[0]))


@pytest.mark.parametrize("name,fault", [("M3", "mod"), ("M4", "mod"), ("M2", "ldkv"), ("M3", "ldkv"), ("M2'", "ldkv"),
                                        ("M4", "ldkv"), ("M1", "v_at_k"), ("M2", "v_at_k"), ("M4-hd48", "v_at_k")])
def test_mha_comparison_rejects_a_wrong_address(name, fault):
    o = U.mha_operands(name, NAN)
    ref = U.mha_ref(o.q, o.k, o.v, o.nh, o.kv_div)
    bad = torch.from_numpy(U.mha_strided(o, fault))
    err = (bad - ref).abs().max().item()
    print(f"{name} with {fault}: max err {err:.3e} (NaN: a guard or gap word was read)")
    rejected(lambda: close(bad, ref, 1e-5))
    if fault == "mod" and name == "M3":  # scene 0's batch is the same under both: the fault shows from scene 1 on
        close(bad[0], ref[0], 1e-5)
        rejected(lambda: close(bad[1], ref[1], 1e-5))


def test_m3_shared_batches_line_up_with_the_kv_div_1_launch():
    o, o1 = U.mha_operands("M3", NAN), U.mha_operands("M3-div1", NAN)
    assert torch.equal(o1.k, o.k) and torch.equal(o1.v, o.v) and torch.equal(o1.q, o.q[[0, 3]])
    assert np.array_equal(U.mha_strided(o)[[0, 3]], U.mha_strided(o1))


def test_guards_report_a_head_stored_past_the_declared_view():
    """The negative control of the GPU file: M2' with the output declared one head narrower than what is stored."""
    o = U.mha_operands("M2'", NAN)
    body = U.mha_strided(o)
    narrow = guarded((o.B, o.Lq, o.d - o.hd), (o.obs, o.ldo, 1), SENTINEL)
    U.store_rows(narrow, body, extra_channels=o.hd)
    assert narrow.dirty() == [b * o.obs + i * o.ldo + c for b in range(o.B) for i in range(o.Lq)
                              for c in range(o.d - o.hd, o.d)]
    with pytest.raises(AssertionError, match="overwritten"):
        narrow.check()
    U.store_rows(o.O, body)
    close(o.O.check(), torch.from_numpy(body.astype(np.float32)), 0.0)  # the declared view, stored right: clean


# --------------------------------------------------------------------------------------------------- sampling
@pytest.fixture(scope="module", params=list(U.GEOMS))
def case(request):
    return U.sample_case(request.param)


def test_points_are_built_to_their_conditions(case):
    c = case
    D, Q, P, Hv, Wv, S = (c[x] for x in ("D", "Q", "P", "Hv", "Wv", "S"))
    assert D % S == 0 and D // S >= 2 and S > 1
    pts = c["pts"].numpy()
    assert np.isfinite(pts).all()
    ix64, iy64 = U.pixel_coords64(pts, c)
    away = np.minimum(np.abs(ix64 - np.rint(ix64)), np.abs(iy64 - np.rint(iy64)))
    rm = c["random_mask"]
    assert (away[rm] >= U.MIN_PX).all() and rm.sum() == D * Q * P - len(c["hand"])  # no random point is left out
    pix, ix, iy = tap_pixels(pts, D, Q, P, Hv, Wv, S, c["inv_max_x"], c["inv_max_y"])
    # where the margin holds, the float32 floor is the float64 floor
    assert np.array_equal(np.floor(ix)[rm], np.floor(ix64)[rm]) and np.array_equal(np.floor(iy)[rm], np.floor(iy64)[rm])
    labels = [h[0] for h in c["hand"]]
    for want in ("corner nw", "corner ne", "corner sw", "corner se", "ix = -1", "ix = Wv - 1", "ix = -0.5", "centre",
                 "same pixel a", "same pixel b"):
        assert want in labels
    for u, (label, tx, ty, exact) in enumerate(c["hand"]):
        if exact:
            assert float(ix[u]) == tx and float(iy[u]) == ty, (label, ix[u], iy[u])
            assert ix64[u] == tx and iy64[u] == ty
        else:  # no float32 point gives the target exactly on this map: the nearest one, within an ulp of the grid value
            assert abs(float(ix[u]) - tx) < 1e-6 and abs(float(iy[u]) - ty) < 1e-6, label
    assert (Hv, Wv) != (64, 64) or all(h[3] for h in c["hand"])
    a, b = labels.index("same pixel a"), labels.index("same pixel b")
    assert (np.floor(ix[a]), np.floor(iy[a])) == (np.floor(ix[b]), np.floor(iy[b])) and (ix[a], iy[a]) != (ix[b], iy[b])
    cap = Q * P * 4
    ps = pix.reshape(D, cap)
    assert (ps[D - 1] == -1).all()                                   # one scene wholly off the map
    assert len(np.unique(ps[D - 2])) == 4 and (ps[D - 2] >= 0).all()  # one scene wholly in one pixel
    assert 0 < (ps[:D - 2] < 0).sum() < ps[:D - 2].size              # some zero-padded taps among the rest
    # maps differ per perception scene
    assert all(not torch.equal(c["value"][0], c["value"][m]) for m in range(1, D))


def test_sampling_comparison_rejects_a_wrong_map_and_a_geometry_mix_up(case):
    c = case
    S = c["S"]
    ref = U.sample_ref(c["logits"], c["pts"], c["value"], S, c)
    good = torch.from_numpy(U.sample_restated(c["logits"], c["pts"], c["value"], S, c))
    close(good, ref, 1e-5)
    close(torch.from_numpy(U.sample_restated(c["logits"], c["pts"], c["value"], 1, c)),
          U.sample_ref(c["logits"], c["pts"], c["value"], 1, c), 1e-5)
    bad = {f: torch.from_numpy(U.sample_restated(c["logits"], c["pts"], c["value"], S, c, f))
           for f in ("map_b", "hw", "scales")}
    print(c["name"], {f: f"{(t - ref).abs().max().item():.3e}" for f, t in bad.items()})
    rejected(lambda: close(bad["map_b"], ref, 1e-5))
    close(bad["map_b"][:1], ref[:1], 1e-5)  # scene 0 reads map 0 either way: the fault shows from scene 1 on
    rejected(lambda: close(bad["map_b"][1], ref[1], 1e-5))
    if c["name"] == "nonsquare":
        rejected(lambda: close(bad["hw"], ref, 1e-5))
        rejected(lambda: close(bad["scales"], ref, 1e-5))
    else:  # the square map with equal scales cannot show either mix-up: why the second geometry exists
        close(bad["hw"], ref, 1e-5)
        close(bad["scales"], ref, 1e-5)


def test_tap_table_checks_reject_a_wrong_image_and_a_wrong_row_base(case):
    c = case
    D, Q, P, Hv, Wv, S = (c[x] for x in ("D", "Q", "P", "Hv", "Wv", "S"))
    pts = c["pts"].numpy()
    geo = dict(B=D, tol=0.0, Q=Q, P=P, HB=Hv, WB=Wv, inv_max_x=c["inv_max_x"], inv_max_y=c["inv_max_y"])
    for s_ in (S, 1):
        rows, slots = U.dedup_restated(pts, c, s_)
        padded, live, _ = check_gathered_taps(pts, rows, slots, None, None, None, samples=s_, **geo)
        assert padded + live == D * Q * P * 4 and padded > 0
    rows, slots = U.dedup_restated(pts, c, S)
    for fault in ("row_base", "map_b"):
        r2, s2 = U.dedup_restated(pts, c, S, fault)
        rejected(lambda: check_gathered_taps(pts, r2, s2, None, None, None, samples=S, **geo))
    rejected(lambda: check_gathered_taps(pts, rows, slots, None, None, None, samples=1, **geo))
    # bev_tap_rows: the image of scene b is b // S (scene 1 still reads image 0)
    pix, _, _ = tap_pixels(pts, D, Q, P, Hv, Wv, S, c["inv_max_x"], c["inv_max_y"])
    pix1, _, _ = tap_pixels(pts, D, Q, P, Hv, Wv, 1, c["inv_max_x"], c["inv_max_y"])
    cap = Q * P * 4
    assert np.array_equal(pix[:cap], pix1[:cap]) and not np.array_equal(pix[cap:2 * cap], pix1[cap:2 * cap])
    live = pix[cap:2 * cap] >= 0
    assert (pix[cap:2 * cap][live] < Hv * Wv).all() and (pix1[cap:2 * cap][live] >= Hv * Wv).all()
    # a slot pointing at the right pixel in another scene's block is refused
    s3 = slots.copy()
    first = int(np.argmax(s3[cap:] >= 0)) + cap
    other = np.flatnonzero(rows[:cap] == rows[s3[first]])
    if len(other):
        s3[first] = other[0]
        rejected(lambda: check_gathered_taps(pts, rows, s3, None, None, None, samples=S, **geo))


# ---------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("C", [64, 36])
def test_pooling_checks_reject_a_dropped_row_offset_and_a_store_past_c(C):
    B, H, W, oh, ow = 2, 16, 64, 8, 32
    x, pos = U.pool_case(B, H, W, C, 451)
    ref = U.pool_ref(x, oh, ow, pos[:oh * ow])

    def stored(fault):
        slab, tk = U.token_slab(B, C, oh, ow)
        U.store_rows(tk, U.pool_restated(x, oh, ow, pos, fault), extra_channels=1 if fault == "past_c" else 0)
        return slab, tk

    slab, tk = stored(None)
    close(tk.check(), ref, 1e-6)
    rest = slab.view()[:, oh * ow:].contiguous().view(torch.int32)
    assert (rest == int(np.array([SENTINEL], np.uint32).view(np.int32)[0])).all()  # rows 256..319 keep the sentinel
    _, tk = stored("no_row")
    rejected(lambda: close(tk.check(), ref, 1e-6))
    _, tk = stored("past_c")
    # every token's overshoot is covered by the next token's own store, except the last of each scene: row 256
    assert tk.dirty() == [b * U.T * C + oh * ow * C for b in range(B)]
    with pytest.raises(AssertionError, match="overwritten"):
        tk.check()
    close(tk.view(), ref, 1e-6)  # by value alone the overshoot is invisible
