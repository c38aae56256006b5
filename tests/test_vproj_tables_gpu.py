"""value_proj.hip through dd_op_vproj on built row tables: the union-staged kernel, the gathered kernel
(union_stage = 0) and the union form with umax = 0 (every tile handed to the fallback launch), each against the float64
reference of tests/vproj_tables_util.py under the per-element f16x3 bound with a measured rho.

Every launch (``launch`` below):
* ``map`` sits inside NaN guards, ``out`` inside sentinel guards and is pre-filled with the sentinel: check() on the
  guards, every row at or past its group's count keeps the sentinel, every live row has lost it in every word;
* the fallback flags read between the two launches equal what the table's numpy union sizes and key ranges say, on both
  halves of every tile, and flags and arrival counters are all zero after the call; the numerics word is 0;
* with a K split, the split partials are pre-filled with NaN and the result must equal, in every bit, the run on
  zero-filled partials.

The contracts pinned here for whoever re-tiles the kernel: a value row does not depend on which of the two kernels
computed its tile (umax = 0 against the default, and the tiles that fall back by range or capacity), nor on its
group's place in the batch, nor on what an earlier launch left in the scratch. tests/test_vproj_tables.py shows on the
CPU that the tables hit their numbers and that the comparison rejects one deliberate fault each."""
import ctypes

import numpy as np
import pytest
import torch

import vproj_tables_util as V
from guard_util import dense_strides, guarded
from test_op_views_gpu import bits_equal
from test_ops_gpu import DEV, g, ok
from test_parity_gpu import _report

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAN_WORD, ZERO_WORD = 0x7FC00000, 0
F16_OVERFLOW = 1  # DD_NUM_F16_OVERFLOW_BIT
FORMS = {"union": (1, V.UMAX_OFF), "gathered": (0, V.UMAX_OFF), "fallback": (1, 0)}
NAMES = ("one_row", "exact_256", "257", "corners_edges", "image_seam", "empty_groups", "range_fallback",
         "union_at_capacity", "union_over_capacity", "shared_images", "shared_256")
_DEVICE = {}


def get_case(name, family=None):
    return V.case(name, family, V.limits()[0] if name in V.CAPACITY_CASES else None)


def operands(c, m=None):
    """The case's map (inside NaN guards), weights and bias on the device, made once."""
    key = (id(c), None if m is None else id(m))
    if key not in _DEVICE:
        mm = c.map if m is None else m
        shape = tuple(mm.shape)
        _DEVICE[key] = (guarded(shape, dense_strides(shape), NAN, values=mm, device=DEV), g(c.w), g(c.bias))
    return _DEVICE[key]


class Ran:
    pass


def call(gpu, c, t, form, usplit, umax=None, part_fill=NAN_WORD, ldh_pad=0, second=None, m=None, out_shift=0,
         B=None, nimg=None):
    """One dd_op_vproj call; returns (rc, Ran) without judging either."""
    mg, w, b = operands(c, m)
    union_stage, um = FORMS[form]
    r = Ran()
    r.t, r.form, r.usplit, r.umax = t, form, usplit, um if umax is None else umax
    rows, counts = torch.from_numpy(t.rows).to(DEV), torch.from_numpy(t.counts).to(DEV)
    r.out = V.out_operand(t, DEV)
    r.flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    tiles = -(-t.B * t.cap // 256)
    host = [(ctypes.c_uint * (2 * tiles))(*([0xFFFFFFFF] * (2 * tiles))) for _ in range(3)]
    rows2 = counts2 = None
    r.out2 = None
    if second is not None:
        assert (second.B, second.cap, second.nimg) == (t.B, t.cap, t.nimg)
        rows2, counts2 = torch.from_numpy(second.rows).to(DEV), torch.from_numpy(second.counts).to(DEV)
        r.out2 = V.out_operand(second, DEV)
    rc = gpu.dd_op_vproj(mg.ptr(), w.data_ptr(), b.data_ptr(), rows.data_ptr(), counts.data_ptr(),
                         r.out.ptr() + out_shift, t.B if B is None else B, t.cap, t.nimg if nimg is None else nimg,
                         union_stage, usplit, r.umax, ldh_pad, part_fill, r.flags.data_ptr(),
                         None if second is None else rows2.data_ptr(), None if second is None else counts2.data_ptr(),
                         None if second is None else r.out2.ptr(), host[0], host[1], host[2], None)
    torch.cuda.synchronize()
    r.fb_seen, r.fb_after, r.ucnt_after = (np.array(h[:], np.uint32).reshape(tiles, 2) for h in host)
    return rc, r


def launch(gpu, c, form, usplit, t=None, **kw):
    """A call that must succeed, with the checks every launch gets (module docstring); returns Ran with .body (the
    whole out), .live (the live rows, compacted) and .fell (per tile None / "range" / "union")."""
    t = t or c.table
    rc, r = call(gpu, c, t, form, usplit, **kw)
    ok(rc, gpu)
    r.body = r.out.check()
    r.live = V.live_rows(t, r.body)
    umax_rows, range_keys = V.limits()
    r.fell = t.fallbacks(umax_rows, range_keys, r.umax) if form != "gathered" else [None] * t.tiles
    want = np.zeros_like(r.fb_seen)
    want[:t.tiles] = np.array([[int(f is not None)] * 2 for f in r.fell], np.uint32).reshape(t.tiles, 2)
    assert np.array_equal(r.fb_seen, want), (t.name, form, usplit, r.fb_seen[:t.tiles].tolist(), r.fell, t.union, t.range)
    assert not r.fb_after.any() and not r.ucnt_after.any(), "fallback flags / arrival counters left set"
    if kw.get("m") is None:
        assert int(r.flags.item()) == 0, hex(int(r.flags.item()))
    if form == "union" and usplit > 1 and kw.get("part_fill", NAN_WORD) == NAN_WORD:
        z = launch(gpu, c, form, usplit, t, **dict(kw, part_fill=ZERO_WORD))
        assert bits_equal(r.body, z.body), "the result depends on what the split partials held before the launch"
        assert r.flags.item() == z.flags.item()
    return r


def note(c, t, r, ratio, extra=""):
    fell = ", ".join(f"tile {i} ({why})" for i, why in enumerate(r.fell) if why) or "none"
    _report([f"== vproj tables {t.name} {c.family} {r.form} split {r.usplit}{extra}: live rows {t.total} tiles {t.tiles} "
             f"fell back: {fell}; rho {c.rho:.3e} (emulation {c.rho_emul:.2e}, fp32 {c.rho_fp32:.2e}) "
             f"worst ratio {ratio:.3f}"])


def all_forms(gpu, c, usplit, **kw):
    """The three forms of one case at one split, each under the bound; the umax = 0 run equals the default union run
    in every bit of every live row. Returns {form: Ran}."""
    t = kw.get("t") or c.table
    ran = {}
    for form in FORMS:
        r = ran[form] = launch(gpu, c, form, usplit, **kw)
        ratio = V.check_output(c, r.body, f"{form} split {usplit}")
        note(c, t, r, ratio)
    assert bits_equal(ran["union"].live, ran["fallback"].live), (
        f"{t.name} split {usplit}: a value row depends on which kernel computed its tile")
    return ran


# --------------------------------------------------------------------------------------- every case, every form
@pytest.mark.parametrize("name", NAMES)
def test_named_case_in_all_forms(gpu, name):
    """Every named table x {union, gathered, umax = 0} x its splits against float64, and the fallback contract on each.
    range_fallback and union_over_capacity fall back by the kernel's own decision in the union form; fb_seen says so
    for exactly those tiles."""
    c = get_case(name)
    t = c.table
    umax_rows, range_keys = V.limits()
    fell = t.fallbacks(umax_rows, range_keys)
    if name == "range_fallback":
        assert fell == [None, "range"]
    if name in V.CAPACITY_CASES:
        assert t.union == [umax_rows + (name == "union_over_capacity")]
        assert fell == (["union"] if name == "union_over_capacity" else [None])
    for usplit in t.splits:
        ran = all_forms(gpu, c, usplit)
        assert ran["union"].fell == fell and all(ran["fallback"].fell)


@pytest.mark.parametrize("family", V.FAMILIES)
def test_input_families(gpu, family):
    """The three input families on the 257-row table (a full tile and a one-row tile), splits 1 and 4."""
    c = get_case("257", family)
    for usplit in (1, 4):
        all_forms(gpu, c, usplit)


def test_umax_argument_at_and_below_the_union_size(gpu):
    """The capacity pair again through the launch's umax: umax = U keeps the tile in the union kernel, umax = U - 1
    hands it over; both equal the default run bit for bit."""
    c = get_case("exact_256")
    U = c.table.union[0]
    for usplit in (1, 2):
        base = launch(gpu, c, "union", usplit)
        at = launch(gpu, c, "union", usplit, umax=U)
        below = launch(gpu, c, "union", usplit, umax=U - 1)
        assert at.fell == [None] and below.fell == ["union"]
        for r in (at, below):
            note(c, c.table, r, V.check_output(c, r.body), f" umax {r.umax}")
            assert bits_equal(r.live, base.live)


@pytest.mark.parametrize("pad", [8, 64])
def test_padded_weight_rows(gpu, pad):
    """ldh = 2304 + pad with NaN halfs in the padding: every form unchanged in every bit."""
    c = get_case("257")
    for form in FORMS:
        base = launch(gpu, c, form, 2)
        wide = launch(gpu, c, form, 2, ldh_pad=pad)
        note(c, c.table, wide, V.check_output(c, wide.body), f" ldh 2304 + {pad}")
        assert bits_equal(wide.body, base.body), (form, pad)


# ------------------------------------------------------------------------------------------------ contracts
@pytest.mark.parametrize("name,perm", [("shared_images", (3, 0, 4, 1, 5, 2)), ("empty_groups", (4, 0, 2, 3, 5, 1)),
                                       ("range_fallback", (2, 0, 4, 1, 3))])
def test_a_groups_rows_do_not_depend_on_its_place_in_the_batch(gpu, name, perm):
    """The groups in another order: rows land in other tiles beside other groups' rows (for range_fallback, in tiles
    that fall back where they did not before); each group's rows are bit-identical, union and gathered form."""
    c = get_case(name)
    t = c.table
    q = t.permuted(list(perm))
    assert not np.array_equal(q.live[:256], t.live[:256])
    for form in ("union", "gathered"):
        a = launch(gpu, c, form, 2)
        b = launch(gpu, c, form, 2, t=q)
        for j, p in enumerate(perm):
            n = int(t.counts[p])
            assert bits_equal(b.body[j * t.cap:j * t.cap + n], a.body[p * t.cap:p * t.cap + n]), (form, j, p)
        note(c, q, b, V.check_output(c, a.body))  # (b's rows are a's: one comparison serves both)


def test_second_launch_on_the_scratch_the_first_left(gpu):
    """Table A, then table B within one call on the same flags, counters and partials: B equals its stand-alone result
    bit for bit - with a split (the counters ran), and with A's first tile handed to the fallback (a flag was raised
    and cleared)."""
    c = get_case("shared_images")
    A = c.table
    Bt = A.permuted([5, 1, 3, 0, 2, 4])
    for usplit, umax in ((4, None), (2, A.union[0] - 1), (1, None)):
        alone = launch(gpu, c, "union", usplit, t=Bt, umax=umax)
        rc, r = call(gpu, c, A, "union", usplit, umax=umax, second=Bt)
        ok(rc, gpu)
        assert not r.fb_after.any() and not r.ucnt_after.any() and int(r.flags.item()) == 0
        assert bits_equal(r.out.check(), launch(gpu, c, "union", usplit, umax=umax).body)
        assert bits_equal(r.out2.check(), alone.body), (usplit, umax)
        if umax is not None:
            assert r.fb_seen[0].tolist() == [1, 1]


def test_overflow_flag_follows_the_live_neighbourhoods(gpu):
    """One map value beyond fp16's range: inside a live row's neighbourhood every form raises DD_NUM_F16_OVERFLOW; in no
    live neighbourhood the word stays 0 and no bit of the result changes."""
    c = get_case("exact_256")  # the block rows 10 .. 25, columns 20 .. 35
    inside, outside = c.map.clone(), c.map.clone()
    inside[0, 9, 19, 37] = 1.0e5    # the corner neighbour of the block's first pixel only
    outside[0, 8, 19, 37] = 1.0e5   # one row further: no live row's neighbourhood
    nb = V.neighbours(c.table.live)
    assert (nb == 9 * 64 + 19).sum() == 1 and not (nb == 8 * 64 + 19).any()
    for form in FORMS:
        for usplit in (1, 2):
            r = launch(gpu, c, form, usplit, m=inside)
            assert int(r.flags.item()) & F16_OVERFLOW, (form, usplit)
            clean = launch(gpu, c, form, usplit, m=outside)
            assert int(clean.flags.item()) == 0, (form, usplit)
            assert bits_equal(clean.body, launch(gpu, c, form, usplit).body)


@pytest.mark.parametrize("what,kw,word", [
    ("B = 257", dict(B=257), b"B in [1, 256]"),
    ("usplit = 3", dict(usplit=3), b"power-of-two split"),
    ("usplit = 16", dict(usplit=16), b"power-of-two split"),
    ("nimg > B", dict(nimg=2), b"more images than row groups"),
    ("misaligned out", dict(out_shift=4), b"16-byte aligned"),
], ids=["B257", "usplit3", "usplit16", "nimg-above-B", "misaligned-out"])
def test_refusals_come_back_as_error_codes_and_launch_nothing(gpu, what, kw, word):
    c = get_case("one_row")
    t = c.table
    if "B" in kw:  # rows and counts for 257 groups of this cap; the table itself is read back only for B <= 256
        t = V.Table("refused", [[2080]] + [[]] * 256, t.cap, 1)
        kw = dict(kw, nimg=1)
        rc, r = call(gpu, c, t, "union", 1, **kw)
    else:
        rc, r = call(gpu, c, t, "union", kw.pop("usplit", 1), **kw)
    assert rc == -2, (what, rc)  # DD_ERR_RUNTIME: launch_vproj's own check
    assert word in gpu.dd_op_last_error(), gpu.dd_op_last_error()
    body = r.out.check()
    assert (body.view(torch.int32) == V.SENT_BITS).all(), "something was launched"
    assert int(r.flags.item()) == 0
