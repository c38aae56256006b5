"""The cases of the per-element f16x3 bound tests (test_f16x3_bound.py, test_f16x3_bound_gpu.py): shapes, expected
routes and the five input families, all built from test_ops_gpu.rnd. A case's tensors, its float64 terms and its rho are
computed once per process and shared (never modified).

Families
  uniform      unit-scale randn activations, fan-in-scaled weights, as the op tests always had.
  rowscale     output channel n's weights, bias and residual x 2^e_n, e_n from -20 .. 10; the last channel and the last
               channel of every 32-column tile differ from both neighbours by at least 8. (The residual is scaled with
               its channel: left at unit scale it would put |res| ~ 1 into D and hide the small channels again.)
  chanscale6   input channel k's activations x 2^-c_k and its weights x 2^c_k, c_k from 0 .. 6 (channel 0 keeps 0, the
               last channel takes 6): the function is unchanged, the activation lo parts are subnormal.
  chanscale12  the same with c_k from 0 .. 12.
  rowrange     output channel n's weights x 2^e_n over the whole of fp32: ROWRANGE cycles through tiny rows (2^-140,
               2^-135, 2^-127, 2^-120, 2^-114, and two rows whose largest |weight| is set to 2^-113 and to
               2^-113 (1 - 2^-24), either side of the scale 2^127 the split would need), one exactly-zero row and
               normal rows (2^-60 .. 2^110); the last channel and the last channel of every 32-column tile are tiny
               or zero with normal neighbours. Bias and residual are scaled with the row on the normal rows and stay
               at unit scale on the tiny and zero rows - a folded BatchNorm's shift survives its dead gamma. (A
               weight is the unit-scale draw times a power of two, exact while it stays a normal fp32 number; below
               2^-126 the product rounds to a subnormal, and that stored fp32 value is the case's weight.) The bound
               gains a flush allowance, err <= rho D + T + FLOOR with FLOOR = 2 max |float64 dot product| over the
               case's tiny rows: a kernel that returns exactly the bias for such a row passes, NaN, Inf or a wrong
               bias does not; rho is measured over the normal rows.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import f16x3_emul as E
from test_ops_gpu import rnd

FAMILIES = ("uniform", "rowscale", "chanscale6", "chanscale12", "rowrange")

# (name, (B, H, W, Cin, Cout, k, stride, pad, relu, res), environment, route). The environment switches are the ones
# test_ops_gpu uses to reach conv_x6's routed forms at a small batch (DDMI_X3_SPLIT=1: no K split ahead of conv_x6,
# DDMI_X6_SMALL=0: not the small-grid form).
X6 = {"DDMI_X3_SPLIT": "1", "DDMI_X6_SMALL": "0"}
CONV_CASES = [
    ("x6-16x16-ragged", (1, 20, 20, 96, 36, 3, 1, 1, True, False), X6, "conv_x6<16,16,64,4,2>"),
    ("x6-small-grid", (1, 20, 20, 96, 36, 3, 1, 1, True, False), {}, "conv_x6<8,8,64,2,2>"),
    ("x6-8x32-res", (2, 8, 40, 128, 192, 3, 1, 1, True, True), X6, "conv_x6<8,32,64,4,2>"),
    ("x3-tapwalk-s2", (2, 16, 24, 64, 128, 3, 2, 1, True, False), {}, "conv_x3<64,64,f16x3>"),
    ("x3-generic-k", (1, 9, 11, 36, 24, 3, 1, 1, False, False), {}, "conv_x3<64,64,f16x3>"),
    ("x3-ksplit", (1, 5, 7, 1056, 200, 1, 1, 0, True, True), {}, "conv_x3<64,64,f16x3,ksplit>"),
    ("x3-gemm-ragged", (3, 5, 7, 320, 40, 1, 1, 0, True, True), {}, "conv_x3<64,64,f16x3>"),
    # two shapes test_conv2d_f16x3 lists as conv_x5's: the dispatcher sends the first to conv_x6's 4-wave form (3 x 3 /
    # stride 1 is conv_x6's first) and the second, M = 4 * 65 * 63 = 16380 < 16384, to conv_x3; both stay, at that route
    ("x6-16x16-4wave", (16, 64, 64, 64, 64, 3, 1, 1, True, True), {}, "conv_x6<16,16,64,4,1>"),
    ("x3-1x1-s2", (4, 130, 126, 64, 128, 1, 2, 0, False, False), {}, "conv_x3<64,64,f16x3>"),
    # ... and their nearest neighbours that do reach conv_x5: pad 2 (conv_x6 takes pad 1 only; M = 16 * 66 * 66 fills
    # 273 tiles of 256 rows, two more rows of padding through the out-of-bounds DMA) and W = 130 (M = 16900, ragged)
    ("x5-256x64-3x3", (16, 64, 64, 64, 64, 3, 1, 2, True, True), {}, "conv_x5<256,64>"),
    ("x5-128x128-1x1-s2", (4, 130, 130, 64, 128, 1, 2, 0, False, False), {}, "conv_x5<128,128>"),
]
STEM_NHWC = [(1, 40, 72), (2, 37, 50)]
STEM_NCHW = [(2, 1, 37, 50), (1, 3, 40, 72)]
STEM_FAMILIES = FAMILIES  # chanscale scales the colour channels only
MK_CASES = [(256, 256), (1024, 256)]


def _ints(lo, hi, n, seed):
    return torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed))


def row_exponents(N, seed):
    """e_n of the rowscale family."""
    e = _ints(-20, 10, N, seed).tolist()
    for n in sorted({N - 1} | set(range(31, N, 32))):
        near = [e[m] for m in (n - 1, n + 1) if 0 <= m < N]
        ok = [v for v in range(-20, 11) if all(abs(v - u) >= 8 for u in near)]
        if not all(abs(e[n] - u) >= 8 for u in near):
            e[n] = ok[(seed + n) % len(ok)]
    return torch.tensor(e, dtype=torch.float32)


# the rowrange family's cycle: an exponent, or "zero" / "edge_ok" / "edge_over" (the rows whose largest |weight| is
# 2^-113 / the fp32 number below it). Tiny (T) and normal (N) alternate: T N T N T N T N T N T N T T
EDGE = {"edge_ok": 2.0 ** -113, "edge_over": 2.0 ** -113 * (1.0 - 2.0 ** -24)}
ROWRANGE = (-140, 0, -135, 40, "edge_ok", -60, -127, 90, "zero", -30, -120, 110, "edge_over", -114)
TINY_MAX = -113  # rows at or below 2^-113 are the family's tiny rows


def _is_tiny(item):
    return isinstance(item, str) or item <= TINY_MAX


def row_range(N, seed):
    """The rowrange item of every output channel: ROWRANGE cycled from an offset, then the last channel and the last
    channel of every 32-column tile made tiny or zero and their neighbours normal."""
    items = [ROWRANGE[(n + seed) % len(ROWRANGE)] for n in range(N)]
    tiny = [i for i in ROWRANGE if _is_tiny(i)]
    normal = [i for i in ROWRANGE if not _is_tiny(i)]
    ends = sorted({N - 1} | set(range(31, N, 32)))
    for j, n in enumerate(ends):
        items[n] = tiny[(seed + j) % len(tiny)]
        for m in (n - 1, n + 1):
            if 0 <= m < N and m not in ends:
                items[m] = normal[(seed + j + m) % len(normal)]
    return items


def tiny_rows(N, seed):
    """bool (N,): the tiny and zero rows of ``row_range``."""
    return torch.tensor([_is_tiny(i) for i in row_range(N, seed)])


def _row_range_apply(w, b, r, seed, emax=None):
    """``emax``: the normal rows' exponents above it are replaced by it (an op whose epilogue squares its values)."""
    N = w.shape[0]
    items = [i if emax is None or isinstance(i, str) else min(i, emax) for i in row_range(N, seed)]
    rows = w.double().reshape(N, -1).clone()
    keep = torch.ones(N, dtype=torch.float64)       # the scale of bias and residual
    for n, item in enumerate(items):
        if item == "zero":
            rows[n] = 0.0
        elif isinstance(item, str):
            amax, k = rows[n].abs().max(0)
            _, ex = torch.frexp(amax)               # amax 2^(-113 - ex) in [2^-114, 2^-113)
            rows[n] *= 2.0 ** (-113 - int(ex))
            rows[n, k] = torch.sign(rows[n, k]) * EDGE[item]
        else:
            rows[n] *= 2.0 ** item
            if not _is_tiny(item):
                keep[n] = 2.0 ** item
    w = rows.float().view(w.shape)                  # RNE into fp32's subnormals below 2^-126
    b = None if b is None else (b.double() * keep).float()
    if r is not None:
        r = (r.double() * (keep.view(1, -1, 1, 1) if r.dim() == 4 else keep)).float()
    return w, b, r


def chan_exponents(C, cmax, seed):
    """c_k of the chanscale families."""
    c = _ints(0, cmax, C, seed)
    c[0] = 0
    c[-1] = cmax
    return c.float()


def _apply(family, x, w, b, r, seed):
    """The family's scaling of one case: x (B, C, ...) or (M, K), w (N, C, ...) or (N, K), b (N,), r with channels on
    axis 1 (conv) or -1 (linear). Powers of two: every scaled value is exact."""
    if family == "uniform":
        return x, w, b, r
    if family == "rowrange":
        return (x,) + _row_range_apply(w, b, r, seed)
    if family == "rowscale":
        s = torch.exp2(row_exponents(w.shape[0], seed))
        w = w * s.view(-1, *([1] * (w.dim() - 1)))
        b = None if b is None else b * s
        if r is not None:
            r = r * (s.view(1, -1, 1, 1) if r.dim() == 4 else s)
        return x, w, b, r
    cmax = {"chanscale6": 6, "chanscale12": 12}[family]
    C = x.shape[1]
    c = torch.exp2(chan_exponents(C, cmax, seed))
    cx = c.view(1, C, *([1] * (x.dim() - 2)))
    cw = c.view(1, C, *([1] * (w.dim() - 2)))
    return x / cx, w * cw, b, r


def _tiny(family, N, seed):
    return tiny_rows(N, seed) if family == "rowrange" else None


class Case:
    """One op case: inputs in the oracle's layout, the float64 terms (ref before ReLU, D, T) and the measured rho."""

    def __init__(self, x, w, b, r, stride, padding, relu, tiny=None):
        self.x, self.w, self.b, self.r = x, w, b, r
        self.stride, self.padding, self.relu = stride, padding, relu
        self.terms = E.terms(x, w, b, r, stride, padding)
        # rowrange: ``tiny`` marks its tiny and zero rows; rho over the others, FLOOR from the tiny rows' dot products
        self.tiny = tiny
        self.normal = None if tiny is None else ~tiny
        self.floor = 0.0
        if tiny is not None:
            xd, wd = x.double(), w.double()[tiny]
            dot = F.conv2d(xd, wd, None, stride, padding) if w.dim() == 4 else F.linear(xd, wd)
            self.floor = 2.0 * float(dot.abs().max())
        self.rho, self.rho_emul, self.rho_fp32 = E.measure_rho(x, w, b, r, stride, padding, t=self.terms,
                                                               rows=self.normal)

    def emul(self, **kw):
        if self.w.dim() == 4:
            return E.conv_x3_emul(self.x, self.w, self.b, self.r, self.stride, self.padding, self.relu, **kw)
        return E.linear_x3_emul(self.x, self.w, self.b, self.r, self.relu, **kw)

    def ratio(self, out):
        """Largest err / bound of ``out`` (the oracle's layout)."""
        return E.bound_ratio(out, *self.terms, self.rho, self.relu, self.floor)

    def normal_limit_min(self):
        """Smallest rho D + T over the elements of the normal rows (rowrange: what FLOOR must stay far below)."""
        _, D, T = self.terms
        lim = (self.rho * D + T).movedim(1 if self.w.dim() == 4 else -1, 0)
        return float(lim[self.normal].min())

    def truth(self):
        ref = self.terms[0]
        return F.relu(ref) if self.relu else ref


@functools.lru_cache(maxsize=None)
def conv_case(shape, family):
    B, H, W, Cin, Cout, k, s, p, relu, res = shape
    x = rnd(B, Cin, H, W, seed=211)
    w = rnd(Cout, Cin, k, k, seed=212, scale=1.0 / np.sqrt(Cin * k * k))
    b = rnd(Cout, seed=213)
    Ho, Wo = E.out_hw(H, W, k, s, p)
    r = rnd(B, Cout, Ho, Wo, seed=214) if res else None
    return Case(*_apply(family, x, w, b, r, 215), s, p, bool(relu), tiny=_tiny(family, Cout, 215))


class StemCase(Case):
    """The fused stem: conv 7 x 7 / 2 + bias + ReLU, then max pooling 3 x 3 / 2. The bound is applied to the conv and
    carried through the max: a pooled output lies within the largest bound of its window of the float64 pooled value."""

    def pooled_ratio(self, out):
        ref, D, T = self.terms
        lim = F.max_pool2d(self.rho * D + T + self.floor, 3, 2, 1)
        err = (out.double() - F.max_pool2d(F.relu(ref), 3, 2, 1)).abs()
        ratio = torch.where(err > 0, err / lim, torch.zeros_like(err))
        return float(torch.where(torch.isfinite(err), ratio, torch.full_like(err, float("inf"))).max())

    def emul_pooled(self, **kw):
        return F.max_pool2d(self.emul(**kw), 3, 2, 1)


@functools.lru_cache(maxsize=None)
def stem_case(B, C, H, W, family):
    """C = 4: the NHWC4 entry (three colour channels and a zero fourth); C = 1..3: the NCHW entry. The conv of the case
    is over the live channels; ``w4`` is the (64, 4, 7, 7) tensor the entry point takes."""
    live = 3 if C == 4 else C
    x = rnd(B, C, H, W, seed=221).abs()
    w4 = rnd(64, 4, 7, 7, seed=222, scale=1.0 / np.sqrt(49 * live))
    w4[:, live:] = 0.0
    b = rnd(64, seed=223)
    xs, ws, b, _ = _apply(family, x[:, :live], w4[:, :live], b, None, 225)
    case = StemCase(xs, ws, b, None, 2, 3, True, tiny=_tiny(family, 64, 225))
    case.w4 = torch.cat([ws, torch.zeros(64, 4 - live, 7, 7)], 1)
    case.x_in = torch.cat([xs, torch.zeros(B, 1, H, W)], 1) if C == 4 else xs
    return case


@functools.lru_cache(maxsize=None)
def mk_case(K, N, family):
    a = rnd(32, K, seed=231)
    w = rnd(N, K, seed=232, scale=1.0 / np.sqrt(K))
    b = rnd(N, seed=233)
    return Case(*_apply(family, a, w, b, None, 235), 1, 0, False, tiny=_tiny(family, N, 235))
