"""State dicts with uneven channel scales, built from the seeded dict without changing the network's function.

ReLU is positively homogeneous, so a hidden channel between two linear maps with only a ReLU (and, in a BasicBlock, a
BatchNorm) between them can be scaled by c > 0 on the way in and by 1 / c on the way out:

  BasicBlock (conv1 -> bn1 -> ReLU -> conv2, no residual on the hidden channels):
      bn1.weight *= c, bn1.bias *= c, conv2.weight[:, k] /= c
  ReLU MLP (GPT blocks' mlp.0 / mlp.2, the tf decoder's linear1 / linear2, the trajectory decoder's ffn.0 / ffn.2 - each
  checked in oracle/model.py to be linear -> F.relu -> linear):
      up.weight[k] *= c, up.bias[k] *= c, down.weight[:, k] /= c

With c a power of two every stored fp32 parameter stays exact, so the float64 oracle computes the same function to
rounding level while the f16x3 kernels meet small activations next to large weights in one row - what BN folding does
to a trained checkpoint, and what the seeded dict (variances 0.8 - 1.6, fan-in-scaled weights) never shows.
"""
import numpy as np

BN_EPS = 1e-5
SEED = 431
SPREADS = (4, 6, 8, 10, 12)
# the largest of SPREADS at which the emulated-f16x3 oracle stays within half of every bar (test_f16x3_bound.py
# asserts that it does at SPREAD; the table of every spread is in DESIGN.md section 5)
SPREAD = 8


def basic_blocks(sd):
    """Prefixes of the BasicBlocks of both trunks (a bn1 with a conv2 and no conv3 beside it)."""
    out = []
    for k in sd:
        if k.endswith(".bn1.weight"):
            p = k[:-len(".bn1.weight")]
            if p + ".conv2.weight" in sd and p + ".conv3.weight" not in sd:
                out.append(p)
    return sorted(out)


def relu_mlps(sd):
    """(up, down) parameter prefixes of every ReLU MLP hidden layer."""
    out = []
    for k in sd:
        if k.endswith(".mlp.0.weight") and ".blocks." in k:
            p = k[:-len(".mlp.0.weight")]
            out.append((p + ".mlp.0", p + ".mlp.2"))
        elif k.endswith(".linear1.weight") and k.startswith("_tf_decoder.layers."):
            p = k[:-len(".linear1.weight")]
            out.append((p + ".linear1", p + ".linear2"))
        elif k.endswith(".ffn.0.weight") and ".diff_decoder.layers." in k:
            p = k[:-len(".ffn.0.weight")]
            out.append((p + ".ffn.0", p + ".ffn.2"))
    return sorted(out)


def _copy(sd):
    return {k: np.array(v, copy=True) for k, v in sd.items()}


def _factors(rng, n, spread):
    """2^-U{0..spread} per channel, as float32 (exact)."""
    return np.exp2(-rng.integers(0, spread + 1, n)).astype(np.float32)


def rescaled(seeded_sd, spread=SPREAD, seed=SEED):
    """Every hidden channel listed above scaled by c = 2^-U{0..spread} through the weights."""
    sd = _copy(seeded_sd)
    rng = np.random.default_rng(seed)
    for p in basic_blocks(sd):
        c = _factors(rng, sd[p + ".bn1.weight"].shape[0], spread)
        sd[p + ".bn1.weight"] *= c
        sd[p + ".bn1.bias"] *= c
        sd[p + ".conv2.weight"] /= c[None, :, None, None]
    for up, down in relu_mlps(sd):
        c = _factors(rng, sd[up + ".weight"].shape[0], spread)
        sd[up + ".weight"] *= c[:, None]
        sd[up + ".bias"] *= c
        sd[down + ".weight"] /= c[None, :]
    return sd


def rescaled_var(seeded_sd, spread=SPREAD, seed=SEED):
    """The BasicBlock channels rescaled through ``running_var``: channel k grows by 2^U (U as in ``rescaled``) because
    its variance shrinks, var' = (var + eps) 2^-2U - eps, where that is positive (U <= 8 on the seeded variances) - then
    gamma / sqrt(var' + eps) is 2^U times the seeded scale, with variances down to ~5e-6, where BN's eps is most of the
    sum (on the seeded variances a fold with the wrong eps moves a scale by 5e-6; here it doubles it) - and through
    bn1.weight otherwise; bn1.bias *= 2^U and conv2.weight[:, k] *= 2^-U either way. var' is rounded to fp32, so the
    function is kept to 1e-7 relative, not to the bit; the truth is the float64 oracle on this dict. The MLPs are as
    in ``rescaled``."""
    sd = _copy(seeded_sd)
    rng = np.random.default_rng(seed)
    for p in basic_blocks(sd):
        c = _factors(rng, sd[p + ".bn1.weight"].shape[0], spread)   # 2^-U
        f = (1.0 / c).astype(np.float32)                            # 2^U
        var = sd[p + ".bn1.running_var"].astype(np.float64)
        small = (var + BN_EPS) * c.astype(np.float64) ** 2 - BN_EPS
        by_var = small > 0
        sd[p + ".bn1.running_var"] = np.where(by_var, small, var).astype(np.float32)
        sd[p + ".bn1.weight"] *= np.where(by_var, np.float32(1), f)
        sd[p + ".bn1.bias"] *= f
        sd[p + ".conv2.weight"] *= c[None, :, None, None]
    for up, down in relu_mlps(sd):
        c = _factors(rng, sd[up + ".weight"].shape[0], spread)
        sd[up + ".weight"] *= c[:, None]
        sd[up + ".bias"] *= c
        sd[down + ".weight"] /= c[None, :]
    return sd


def rescaled_signed(seeded_sd, spread=SPREAD, seed=SEED):
    """``rescaled`` with bn2.weight = -2^-10 on a tenth of every BasicBlock's output channels: negative, near-zero
    folded scales. Not function-preserving; the truth is the float64 oracle on this dict."""
    sd = rescaled(seeded_sd, spread, seed)
    rng = np.random.default_rng(seed + 1)
    for p in basic_blocks(sd):
        g = sd[p + ".bn2.weight"]
        pick = rng.permutation(g.shape[0])[: max(1, g.shape[0] // 10)]
        g[pick] = -np.float32(2.0 ** -10)
    return sd


VARIANTS = {"rescaled": rescaled, "rescaled_var": rescaled_var, "rescaled_signed": rescaled_signed}
