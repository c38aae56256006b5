"""CPU: the guard harness (tests/guard_util.py) reports what it is there to report. A correct numpy 'kernel' - rows of
C = A W^T written through the strided output view - passes; three deliberately wrong ones are each caught: a store one
element past a row's Cout, a skipped last row, and a product of an out-of-operand word with zero."""
import numpy as np
import pytest
import torch

from guard_util import GUARD_ROWS, POISON, SENTINEL, dense_strides, guarded

G, R, K, N = 2, 5, 8, 6       # two groups of five rows
LDA, LDC = 12, 10             # row strides wider than the rows: gap columns in A and in C
GSA, GSC = 7 * LDA, 6 * LDC   # group strides wider than the groups: gap rows


def _operands(poison=float("nan")):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((G, R, K)).astype(np.float32)
    w = rng.standard_normal((N, K)).astype(np.float32)
    A = guarded((G, R, K), (GSA, LDA, 1), poison, values=a)
    C = guarded((G, R, N), (GSC, LDC, 1), SENTINEL)
    ref = torch.from_numpy(a.astype(np.float64) @ w.astype(np.float64).T)
    return A, w, C, ref


def _kernel(A, w, C, bug=None):
    """Rows of C = A W^T on the flat allocations, addressed as a kernel does: pointer + strides."""
    a, c = A.t.numpy(), C.t.numpy()
    for g in range(G):
        for r in range(R):
            if bug == "skip_last_row" and g == G - 1 and r == R - 1:
                continue
            ao, co = A.offset + g * GSA + r * LDA, C.offset + g * GSC + r * LDC
            row = a[ao:ao + K] @ w.T
            if bug == "zero_times_gap":  # a K tail read past the row and 'masked' by a zero weight
                row = row + np.float32(0.0) * a[ao + K]
            c[co:co + N] = row
            if bug == "store_past_cout":
                c[co + N] = row[0]


def _close(body, ref):
    err = (body.double() - ref).abs().max().item()
    assert err <= 1e-5 * (1 + ref.abs().max().item()), f"max err {err}"  # NaN fails too


def test_layout_and_alignment():
    A, _, C, _ = _operands()
    for t, rs in ((A, LDA), (C, LDC)):
        assert t.guard >= GUARD_ROWS * rs and t.guard % 128 == 0 and t.offset % 128 == 0
        assert t.total == t.t.numel() and t.total - t.offset - t.extent >= t.guard
    assert C.guard_words == C.total - G * R * N
    words = C.t.view(torch.int32)
    assert (words[~C.mask] == np.array([SENTINEL], np.uint32).view(np.int32)[0]).all()
    assert torch.isnan(C.view()).all() and torch.isnan(A.t[~A.mask]).all()
    assert dense_strides((2, 3, 4)) == (12, 4, 1)


def test_correct_kernel_passes_under_both_poisons():
    A, w, C, ref = _operands()
    _kernel(A, w, C)
    body = C.check()
    _close(body, ref)
    A2, w, C2, _ = _operands(POISON)
    assert (A2.t[~A2.mask] == POISON).all()
    _kernel(A2, w, C2)
    assert torch.equal(C2.check().view(torch.int32), body.view(torch.int32))


def test_store_past_cout_is_reported():
    A, w, C, _ = _operands()
    _kernel(A, w, C, "store_past_cout")
    assert C.dirty() == [g * GSC + r * LDC + N for g in range(G) for r in range(R)]
    with pytest.raises(AssertionError, match="overwritten"):
        C.check()


def test_skipped_row_is_reported():
    A, w, C, ref = _operands()
    _kernel(A, w, C, "skip_last_row")
    body = C.check()  # nothing outside the body was touched ...
    assert torch.isnan(body[-1, -1]).all() and not torch.isnan(body[:-1]).any()
    with pytest.raises(AssertionError):  # ... but the comparison sees the unwritten row
        _close(body, ref)


def test_zero_times_gap_word_is_reported():
    A, w, C, ref = _operands()
    _kernel(A, w, C, "zero_times_gap")
    body = C.check()
    assert torch.isnan(body).all()
    with pytest.raises(AssertionError):
        _close(body, ref)


def test_broadcast_view_and_window():
    """A stride-0 dimension holds one copy; a window re-declares part of the allocation and keeps the rest as it is."""
    pos = torch.arange(12, dtype=torch.float32).reshape(1, 3, 4)
    P = guarded((5, 3, 4), (0, 4, 1), float("nan"), values=pos)
    assert P.extent == 12 and torch.equal(P.view()[4], pos[0])
    C = guarded((G, R, N), (GSC, LDC, 1), SENTINEL)
    C.view()[...] = 1.0
    C.check()
    row = C.window((G, 1, N), (GSC, LDC, 1), start=R * LDC)  # the gap row after each group
    row.view()[...] = 2.0
    row.check()
    C.view()[0, 0, 0] = 3.0  # the first declaration's body is now outside
    with pytest.raises(AssertionError, match="overwritten"):
        row.check()
