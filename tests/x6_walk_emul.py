"""conv_x6's Winograd F(2,3) walk along W (the conv_x6.hip header) restated on the CPU on top of
f16x3_emul.py - from the documents, not from the kernel's code.

Arithmetic of a 3 x 3 / stride 1 / pad 1 conv, for the output pair p = (2p, 2p + 1) of a row:
  * weights: per (co, ky, ci) the BN-folded fp32 taps g0, g1, g2 along kx become, in double, U0 = g0,
    U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2, rounded to fp32; every Cout row is scaled by one power
    of two over its 12 Cin entries (f16x3_emul.split_weights: the existing rule, the same exponent cap) and split into
    hi / lo fp16;
  * activations: with d_i = in[2p - 1 + i] (zero outside the map), in fp32 and before the hi / lo split,
    V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3; each is split unscaled;
  * four planes M_xi = sum over (ky, ci) of V_xi U_xi in the f16x3 products (al wh + ah wl + ah wh), fp32 accumulation
    in k16 steps, K order (ky, ci);
  * out[2p] = M0 + M1 + M2 and out[2p + 1] = M1 - M2 - M3 in fp32, then the usual epilogue: 1 / s_r, bias, residual,
    ReLU. An odd W drops the second pixel of the last pair.

rho_w of a case is 4 x the larger of this emulation's max (err - T)+ / D and plain fp32's max err / D (the direct walk's
plain fp32, f16x3_emul.measure_rho): the metric, D and T are the direct conv's, unchanged.
"""
import contextlib

import torch
import torch.nn.functional as F

import f16x3_emul as E


def walk_weights(w):
    """(Cout, Cin, 3, 3) fp32 -> (Cout, 3, 4, Cin) fp32: the kx taps transformed in double, K order (ky, xi, ci)."""
    g = w.double()
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]                       # (Cout, Cin, ky)
    u = torch.stack([g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2], -1)   # (Cout, Cin, ky, xi)
    return u.permute(0, 2, 3, 1).float().contiguous()


def walk_rows(x):
    """(B, C, H, W) fp32 -> (B, H + 2, Wp, 4, C) fp32 with Wp = ceil(W / 2): V_xi of every pair of every halo row."""
    x = x.float()
    W = x.shape[-1]
    Wp = (W + 1) // 2
    xp = F.pad(x, (1, 2 * Wp + 1 - W, 1, 1))                            # columns -1 .. 2 Wp
    d0, d1, d2, d3 = (xp[..., i:i + 2 * Wp:2] for i in range(4))
    v = torch.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], -1)           # (B, C, H + 2, Wp, 4)
    return v.permute(0, 2, 3, 4, 1).contiguous()


def conv_walk_emul(x, w, bias=None, res=None, relu=False, acc=torch.float32, kstep=E.KSTEP):
    """NCHW 3 x 3 / stride 1 / pad 1 conv in the walk's arithmetic: x (B, Cin, H, W), w (Cout, Cin, 3, 3), res
    (B, Cout, H, W)."""
    B, C, H, W = x.shape
    N = w.shape[0]
    Wp = (W + 1) // 2
    u = walk_weights(w)                                                 # (N, 3, 4, C)
    wh, wl, sinv = E.split_weights(u.reshape(N, -1))
    wh, wl = wh.view(N, 3, 4, C), wl.view(N, 3, 4, C)
    v = walk_rows(x)                                                    # (B, H + 2, Wp, 4, C)
    planes = []
    for xi in range(4):
        a = torch.cat([v[:, ky:ky + H, :, xi] for ky in range(3)], -1).reshape(B * H * Wp, 3 * C)   # K order (ky, ci)
        ah, al = E.split_act(a)
        planes.append(E._accumulate(ah, al, wh[:, :, xi].reshape(N, -1), wl[:, :, xi].reshape(N, -1), acc, kstep,
                                    None).float())
    m0, m1, m2, m3 = planes
    y = torch.stack([m0 + m1 + m2, m1 - m2 - m3], 1)                    # (B H Wp, 2, N)
    y = y.view(B, H, 2 * Wp, N)[:, :, :W] * sinv
    if bias is not None:
        y = y + bias.float()
    y = y.permute(0, 3, 1, 2)
    if res is not None:
        y = y + res.float()
    return F.relu(y) if relu else y


def measure_rho_w(case):
    """(rho_w, the emulation's max (err - T)+ / D, plain fp32's max err / D) of a f16x3_cases.Case (before any ReLU; the
    rowrange family over its normal rows, as measure_rho)."""
    ref, D, T = case.terms
    em = conv_walk_emul(case.x, case.w, case.b, case.r)
    if case.normal is not None:
        ref, D, T, em = (t.movedim(1, 0)[case.normal] for t in (ref, D, T, em))
    Dp = D.clamp_min(torch.finfo(torch.float64).tiny)
    r_em = float((((em.double() - ref).abs() - T).clamp_min(0) / Dp).max())
    return 4.0 * max(r_em, case.rho_fp32), r_em, case.rho_fp32


def routable(w, stride, padding):
    """The convs the walk's oracle replaces: 3 x 3 / stride 1 / pad 1 with Cin >= 128 and Cin % 32 == 0 (a superset of
    what the forward routes)."""
    return w.dim() == 4 and w.shape[-1] == 3 and stride == 1 and padding == 1 and w.shape[1] >= 128 and \
        w.shape[1] % 32 == 0


@contextlib.contextmanager
def emulated_walk_oracle(acc=torch.float32, kstep=None):
    """f16x3_emul.emulated_f16x3_oracle with every routable conv in the walk's arithmetic instead of the direct one.
    Yields the list that collects the replaced convs' names."""
    import oracle.model as om
    replaced = []
    with E.emulated_f16x3_oracle(acc=acc, kstep=kstep):
        direct = om.conv

        def conv(x, sd, p, stride=1, padding=0, bias=False):
            w = sd[p + ".weight"]
            if not routable(w, stride, padding):
                return direct(x, sd, p, stride, padding, bias)
            b = sd[p + ".bias"].double() if bias else None
            q = E._bn_prefix(sd, p)
            if q is not None:
                s = sd[q + ".weight"].double() / torch.sqrt(sd[q + ".running_var"].double() + om.BN_EPS)
                shift = sd[q + ".bias"].double() - sd[q + ".running_mean"].double() * s
                w = (w.double() * s[:, None, None, None]).float()
                b = shift if b is None else b + shift
            y = conv_walk_emul(x, w, None if b is None else b.float(), None, acc=acc, kstep=kstep)
            if q is not None:
                y._f16x3_folded = q
            replaced.append(p)
            return y

        om.conv = conv
        try:
            yield replaced
        finally:
            om.conv = direct


# --------------------------------------------------------------------------- the cases of the walk's tests
# (B, H, W, Cin, Cout, k, stride, pad, relu, res): the x6 cases of f16x3_cases.py (the small-grid one shares the ragged
# one's tensors), an odd-W case and a Cin = 160 case
CPU_SHAPES = [
    ("x6-16x16-ragged", (1, 20, 20, 96, 36, 3, 1, 1, True, False)),
    ("x6-8x32-res", (2, 8, 40, 128, 192, 3, 1, 1, True, True)),
    ("x6-16x16-4wave", (16, 64, 64, 64, 64, 3, 1, 1, True, True)),
    ("odd-w", (1, 10, 19, 128, 160, 3, 1, 1, False, False)),
    ("cin-160", (2, 8, 34, 160, 128, 3, 1, 1, False, False)),
]


class WalkCase:
    """A f16x3_cases.Case with rho_w in place of rho: the same inputs, float64 terms and flush allowance."""

    def __init__(self, case):
        self.case = case
        self.rho, self.rho_emul, self.rho_fp32 = measure_rho_w(case)

    def emul(self, **kw):
        c = self.case
        return conv_walk_emul(c.x, c.w, c.b, c.r, c.relu, **kw)

    def ratio(self, out):
        c = self.case
        return E.bound_ratio(out, *c.terms, self.rho, c.relu, c.floor)


_CASES = {}


def walk_case(shape, family):
    import f16x3_cases as C
    if (shape, family) not in _CASES:
        _CASES[(shape, family)] = WalkCase(C.conv_case(shape, family))
    return _CASES[(shape, family)]
