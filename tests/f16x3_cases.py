"""The cases of the per-element f16x3 bound tests (test_f16x3_bound.py, test_f16x3_bound_gpu.py): shapes, expected
routes and the four input families, all built from test_ops_gpu.rnd. A case's tensors, its float64 terms and its rho are
computed once per process and shared (never modified).

Families
  uniform      unit-scale randn activations, fan-in-scaled weights, as the op tests always had.
  rowscale     output channel n's weights, bias and residual x 2^e_n, e_n from -20 .. 10; the last channel and the last
               channel of every 32-column tile differ from both neighbours by at least 8. (The residual is scaled with
               its channel: left at unit scale it would put |res| ~ 1 into D and hide the small channels again.)
  chanscale6   input channel k's activations x 2^-c_k and its weights x 2^c_k, c_k from 0 .. 6 (channel 0 keeps 0, the
               last channel takes 6): the function is unchanged, the activation lo parts are subnormal.
  chanscale12  the same with c_k from 0 .. 12.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import f16x3_emul as E
from test_ops_gpu import rnd

FAMILIES = ("uniform", "rowscale", "chanscale6", "chanscale12")

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


class Case:
    """One op case: inputs in the oracle's layout, the float64 terms (ref before ReLU, D, T) and the measured rho."""

    def __init__(self, x, w, b, r, stride, padding, relu):
        self.x, self.w, self.b, self.r = x, w, b, r
        self.stride, self.padding, self.relu = stride, padding, relu
        self.terms = E.terms(x, w, b, r, stride, padding)
        self.rho, self.rho_emul, self.rho_fp32 = E.measure_rho(x, w, b, r, stride, padding, t=self.terms)

    def emul(self, **kw):
        if self.w.dim() == 4:
            return E.conv_x3_emul(self.x, self.w, self.b, self.r, self.stride, self.padding, self.relu, **kw)
        return E.linear_x3_emul(self.x, self.w, self.b, self.r, self.relu, **kw)

    def ratio(self, out):
        """Largest err / bound of ``out`` (the oracle's layout)."""
        return E.bound_ratio(out, *self.terms, self.rho, self.relu)

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
    return Case(*_apply(family, x, w, b, r, 215), s, p, bool(relu))


class StemCase(Case):
    """The fused stem: conv 7 x 7 / 2 + bias + ReLU, then max pooling 3 x 3 / 2. The bound is applied to the conv and
    carried through the max: a pooled output lies within the largest bound of its window of the float64 pooled value."""

    def pooled_ratio(self, out):
        ref, D, T = self.terms
        lim = F.max_pool2d(self.rho * D + T, 3, 2, 1)
        err = (out.double() - F.max_pool2d(F.relu(ref), 3, 2, 1)).abs()
        return float(torch.where(err > 0, err / lim, torch.zeros_like(err)).max())

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
    case = StemCase(xs, ws, b, None, 2, 3, True)
    case.w4 = torch.cat([ws, torch.zeros(64, 4 - live, 7, 7)], 1)
    case.x_in = torch.cat([xs, torch.zeros(B, 1, H, W)], 1) if C == 4 else xs
    return case


@functools.lru_cache(maxsize=None)
def mk_case(K, N, family):
    a = rnd(32, K, seed=231)
    w = rnd(N, K, seed=232, scale=1.0 / np.sqrt(K))
    b = rnd(N, seed=233)
    return Case(*_apply(family, a, w, b, None, 235), 1, 0, False)
