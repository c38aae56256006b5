"""The f16x3 arithmetic of DESIGN.md section 5 and the conv_x3.hip header, restated on the CPU - from the documents, not
from any kernel's code - and the per-element error metric the f16x3 bound tests use (test_f16x3_bound.py on the CPU,
test_f16x3_bound_gpu.py on the device).

Arithmetic: a weight row r is scaled by s_r = 2^e with max|w_r| s_r in [2^14, 2^15) - e <= 126, so that s_r and 1 / s_r
are normal fp32 numbers on the rows below 2^-112 too - and split into hi = f16(w s_r), lo = f16(w s_r - hi); an activation is split unscaled, hi = f16(x), lo = f16(x - hi) (fp16 subnormals kept, as the
hardware's conversion keeps them). A product is al wh + ah wl + ah wh, every f16 x f16 product exact in fp32, summed in
the accumulator's type in steps of 16 along K (K order: tap, then channel); the sum is multiplied by 1 / s_r, then bias,
residual and ReLU follow in fp32.

Metric: per output element, err = |out - ref64| and D = sum_k |a_k| |w_k| + |bias| + |res| in float64, with the bound

    err <= rho D + 2^-25 sum_k |w_k| [|a_k| < 2^-2]

The second term T is the cost of a subnormal activation lo part: |a| < 2^-2 can put the lo part (<= 2^-12 |a|) below
fp16's smallest normal 2^-14, where the spacing is 2^-24 and the rounding error up to 2^-25 absolute, times the weight.
``rho`` covers everything else (split residue, accumulation). It is measured, never taken from the device: 4 x the larger
of the smallest rho with which this emulation (fp32 accumulation) meets the bound, max (err - T)+ / D, and of plain CPU
fp32's max err / D, on the same inputs; the factor 4 is for the MFMA's summation order, which is not the emulation's.
(T is taken off the emulation's error because rho is by definition the part of the bound T does not cover; with the error
taken whole, rho would absorb the subnormal cost and the uneven-channel families could not meet rho <= 1e-6.)
Plain fp32 is the unsplit fp32 operands through the emulation's own K steps and epilogue, so that the two differ by the
split alone and rho does not depend on the host's BLAS: F.conv2d / F.linear in fp32 read 1.3e-7 - 4.3e-7 on the cases of
f16x3_cases.py (long sequential chains at K = 64 and 196), the stepped sum 0.5e-7 - 1.4e-7, which is the tighter rho.
"""
import contextlib

import torch
import torch.nn.functional as F

KSTEP = 16
SUB_LIMIT = 2.0 ** -2   # activations below it may have a subnormal lo part
SUB_ERR = 2.0 ** -25    # half of fp16's subnormal spacing
RHO_MAX = 1e-6
SPLIT_MAX_EXP = 126     # the weight scale's largest exponent: 2^126 and 2^-126 are both normal fp32 numbers


# --------------------------------------------------------------------------- the split
def split_weights(w):
    """(hi, lo, sinv) of a (rows, K) weight matrix: per-row power-of-two scale, two fp16 images, the inverse scale
    (fp32). The scaling is exact in fp32; a zero row keeps scale 1; e <= 126, so a row with max|w_r| < 2^-112 is
    scaled by 2^126 (2^127 would leave 1 / s subnormal, 2^128 is inf) and fills less of the fp16 range."""
    w = w.float()
    amax = w.abs().amax(1)
    _, ex = torch.frexp(amax)                      # amax = f 2^ex, f in [0.5, 1)
    e = torch.where(amax > 0, (15 - ex).clamp_max(SPLIT_MAX_EXP), torch.zeros_like(ex))
    s = torch.ldexp(torch.ones_like(amax), e)
    v = w * s[:, None]
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi, lo, torch.ldexp(torch.ones_like(amax), -e)


def split_act(x):
    """(hi, lo) of an activation tensor, unscaled."""
    x = x.float()
    hi = x.half()
    return hi, (x - hi.float()).half()


def flush_subnormal(h):
    """fp16 tensor with its subnormal values replaced by zero (the flush-to-zero mutant)."""
    return torch.where(h.float().abs() < 2.0 ** -14, torch.zeros_like(h), h)


# --------------------------------------------------------------------------- im2col in the device's K order
def im2col(x, k, stride, padding):
    """(B, C, H, W) -> (B * Ho * Wo, k * k * C), K ordered tap-major (ky, kx, c) as the NHWC kernels walk it."""
    B, C = x.shape[:2]
    if k == 1 and padding == 0:
        xs = x[:, :, ::stride, ::stride]
        return xs.permute(0, 2, 3, 1).reshape(-1, C)
    cols = F.unfold(x, k, padding=padding, stride=stride)           # (B, C * k * k, L), K ordered (c, ky, kx)
    L = cols.shape[-1]
    return cols.view(B, C, k * k, L).permute(0, 3, 2, 1).reshape(B * L, k * k * C)


def weight_rows(w):
    """(Cout, Cin, k, k) -> (Cout, k * k * Cin) in the same K order; a 2-D matrix is returned as it is."""
    return w if w.dim() == 2 else w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def out_hw(H, W, k, stride, padding):
    return (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1


# --------------------------------------------------------------------------- the emulation
def _accumulate(ah, al, wh, wl, acc, kstep, mutant):
    """sum_k (al wh + ah wl + ah wh) over rows of a (M, K) x (N, K)^T product, in ``acc``, K in steps of ``kstep``
    (None: one step, the BLAS order). ``mutant`` "drop_ahwl_last": the ah wl product is left out of the last step."""
    ah, al, wh, wl = (t.to(acc) for t in (ah, al, wh, wl))
    K = ah.shape[1]
    if kstep is None and mutant != "drop_ahwl_last":
        return al @ wh.T + ah @ wl.T + ah @ wh.T
    step = kstep or KSTEP
    out = torch.zeros(ah.shape[0], wh.shape[0], dtype=acc)
    for k0 in range(0, K, step):
        s = slice(k0, min(k0 + step, K))
        last = k0 + step >= K
        part = al[:, s] @ wh[:, s].T
        if not (last and mutant == "drop_ahwl_last"):
            part = part + ah[:, s] @ wl[:, s].T
        out += part + ah[:, s] @ wh[:, s].T
    return out


def gemm_x3_emul(a, w, bias=None, res=None, relu=False, acc=torch.float32, kstep=KSTEP, mutant=None):
    """Rows ``a`` (M, K) times weight rows ``w`` (N, K) in the documented arithmetic; bias (N,), res (M, N).
    Mutants (test_f16x3_bound.py): "drop_ahwl_last", "flush_act_lo" (activation lo parts flushed when subnormal),
    "sinv_neighbour" (the last column scaled back with column N - 2's 1 / s), "no_row_scale" (weights split unscaled).
    "plain_fp32" is no mutant: the unsplit fp32 operands through the same K steps and epilogue (measure_rho)."""
    if mutant == "plain_fp32":
        a32, w32 = a.float(), w.float()
        y = torch.zeros(a32.shape[0], w32.shape[0])
        for k0 in range(0, a32.shape[1], kstep or KSTEP):
            y += a32[:, k0:k0 + (kstep or KSTEP)] @ w32[:, k0:k0 + (kstep or KSTEP)].T
        if bias is not None:
            y = y + bias.float()[None]
        if res is not None:
            y = y + res.float()
        return F.relu(y) if relu else y
    ah, al = split_act(a)
    if mutant == "flush_act_lo":
        al = flush_subnormal(al)
    if mutant == "no_row_scale":
        wf = w.float()
        wh = wf.half()
        wl = (wf - wh.float()).half()
        sinv = torch.ones(w.shape[0])
    else:
        wh, wl, sinv = split_weights(w)
    if mutant == "sinv_neighbour" and w.shape[0] > 1:
        sinv = sinv.clone()
        sinv[-1] = sinv[-2]
    y = _accumulate(ah, al, wh, wl, acc, kstep, mutant).float() * sinv[None]
    if bias is not None:
        y = y + bias.float()[None]
    if res is not None:
        y = y + res.float()
    return F.relu(y) if relu else y


def conv_x3_emul(x, w, bias=None, res=None, stride=1, padding=0, relu=False, acc=torch.float32, kstep=KSTEP,
                 mutant=None):
    """NCHW conv in the documented arithmetic: x (B, Cin, H, W), w (Cout, Cin, k, k), res (B, Cout, Ho, Wo)."""
    B, _, H, W = x.shape
    k = w.shape[-1]
    Ho, Wo = out_hw(H, W, k, stride, padding)
    r = None if res is None else res.permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    y = gemm_x3_emul(im2col(x.float(), k, stride, padding), weight_rows(w), bias, r, relu, acc, kstep, mutant)
    return y.view(B, Ho, Wo, -1).permute(0, 3, 1, 2)


def linear_x3_emul(x, w, bias=None, res=None, relu=False, acc=torch.float32, kstep=KSTEP, mutant=None):
    """x (..., K) times w (N, K)^T in the documented arithmetic."""
    r = None if res is None else res.reshape(-1, w.shape[0])
    y = gemm_x3_emul(x.reshape(-1, x.shape[-1]), w, bias, r, relu, acc, kstep, mutant)
    return y.view(*x.shape[:-1], w.shape[0])


# --------------------------------------------------------------------------- the metric
def terms(x, w, bias=None, res=None, stride=1, padding=0):
    """(ref, D, T) in float64 for a conv (4-D x, w) or a linear (w 2-D): the float64 result before any ReLU, the
    denominator D = conv(|x|, |w|) + |bias| + |res| and the subnormal term T = 2^-25 conv([|x| < 2^-2], |w|)."""
    xd, wd = x.double(), w.double()
    bd = None if bias is None else bias.double()
    small = (xd.abs() < SUB_LIMIT).double()
    if w.dim() == 4:
        ref = F.conv2d(xd, wd, bd, stride, padding)
        D = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride, padding)
        T = F.conv2d(small, wd.abs(), None, stride, padding) * SUB_ERR
    else:
        ref = F.linear(xd, wd, bd)
        D = F.linear(xd.abs(), wd.abs(), None if bd is None else bd.abs())
        T = F.linear(small, wd.abs()) * SUB_ERR
    if res is not None:
        ref = ref + res.double()
        D = D + res.double().abs()
    return ref, D, T


def eta(out, x, w, bias=None, res=None, stride=1, padding=0, relu=False):
    """(err, D): the per-element error of ``out`` (the op's result in the oracle's layout) against float64 and the
    per-element denominator, both float64. With ``relu`` the truth is ReLU of the float64 pre-activation: where that is
    negative the output must be 0 or within the bound of 0, which is |out - 0| <= bound."""
    ref, D, _ = terms(x, w, bias, res, stride, padding)
    if relu:
        ref = F.relu(ref)
    return (out.double() - ref).abs(), D


def measure_rho(x, w, bias=None, res=None, stride=1, padding=0, t=None, rows=None):
    """rho of one case, (rho, emulation's max (err - T)+ / D, plain fp32's max err / D): computed on the CPU from the
    emulation with fp32 accumulation and from PyTorch's fp32 op on the same inputs, before any ReLU. ``t`` may carry
    the case's ``terms`` to spare a second float64 pass; ``rows`` (bool per output channel) restricts the maxima to
    those channels (the rowrange family measures rho over its normal rows)."""
    ref, D, T = t if t is not None else terms(x, w, bias, res, stride, padding)
    if w.dim() == 4:
        em = conv_x3_emul(x, w, bias, res, stride, padding)
        f32 = conv_x3_emul(x, w, bias, res, stride, padding, mutant="plain_fp32")
    else:
        em = linear_x3_emul(x, w, bias, res)
        f32 = linear_x3_emul(x, w, bias, res, mutant="plain_fp32")
    if rows is not None:
        ax = 1 if w.dim() == 4 else -1
        ref, D, T, em, f32 = (v.movedim(ax, 0)[rows] for v in (ref, D, T, em, f32))
    Dp = D.clamp_min(torch.finfo(torch.float64).tiny)
    r_em = float((((em.double() - ref).abs() - T).clamp_min(0) / Dp).max())
    r_32 = float(((f32.double() - ref).abs() / Dp).max())
    return 4.0 * max(r_em, r_32), r_em, r_32


def bound_ratio(out, ref, D, T, rho, relu=False, floor=0.0):
    """Largest err / (rho D + T + floor) over the elements of ``out`` (float64 ``ref`` before ReLU); <= 1 meets the
    bound. An element of ``out`` that is not finite is infinitely far off."""
    truth = F.relu(ref) if relu else ref
    lim = rho * D + T + floor
    err = (out.double() - truth).abs()
    ratio = torch.where(err > 0, err / lim.clamp_min(torch.finfo(torch.float64).tiny), torch.zeros_like(err))
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(err, float("inf")))
    return float(ratio.max())


def old_bar_ok(out, ref, tol=3e-5):
    """test_ops_gpu.close(): one max-norm bar per tensor."""
    return float((out.double() - ref).abs().max()) <= tol * (1.0 + float(ref.abs().max()))


# --------------------------------------------------------------------------- the oracle on emulated f16x3
_BN_OF = ((".conv1", ".bn1"), (".conv2", ".bn2"), (".conv3", ".bn3"), (".downsample.0", ".downsample.1"))


def _bn_prefix(sd, p):
    for c, b in _BN_OF:
        if p.endswith(c):
            q = p[:-len(c)] + b
            if q + ".running_var" in sd:
                return q
    return None


@contextlib.contextmanager
def emulated_f16x3_oracle(acc=torch.float32, kstep=None):
    """While active, ``oracle.model.conv`` and ``oracle.model.linear`` compute in the documented f16x3 arithmetic, at
    the sites where the device does: every conv, with its BatchNorm folded as ``prep_conv`` folds it (scale =
    gamma / sqrt(var + eps) and shift in double, the folded weights rounded to fp32, then split; ``oracle.model.bn``
    passes such a conv's output through), and every ``linear`` (``prep_linear`` splits them all). What the oracle
    computes outside these two functions stays fp32: the attention in-projections and scores, softmax, LayerNorm,
    interpolation, the residual adds and ReLUs, the DDIM glue. Meant for an fp32 state dict and fp32 inputs."""
    import oracle.model as om
    orig = om.conv, om.linear, om.bn

    def conv(x, sd, p, stride=1, padding=0, bias=False):
        w = sd[p + ".weight"]
        b = sd[p + ".bias"].double() if bias else None
        q = _bn_prefix(sd, p)
        if q is not None:
            s = sd[q + ".weight"].double() / torch.sqrt(sd[q + ".running_var"].double() + om.BN_EPS)
            shift = sd[q + ".bias"].double() - sd[q + ".running_mean"].double() * s
            w = (w.double() * s[:, None, None, None]).float()
            b = shift if b is None else b + shift
        y = conv_x3_emul(x, w, None if b is None else b.float(), None, stride, padding, acc=acc, kstep=kstep)
        if q is not None:
            y._f16x3_folded = q
        return y

    def bn(x, sd, p):
        if getattr(x, "_f16x3_folded", None) == p:
            return x
        return orig[2](x, sd, p)

    def linear(x, sd, p, bias=True):
        return linear_x3_emul(x, sd[p + ".weight"], sd[p + ".bias"] if bias else None, acc=acc, kstep=kstep)

    om.conv, om.linear, om.bn = conv, linear, bn
    try:
        yield
    finally:
        om.conv, om.linear, om.bn = orig
