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


# --------------------------------------------------------------------------- dead and tiny rows
# What weight decay leaves in a trained checkpoint: BatchNorm gammas at 0 and in fp32's lowest binades (the fold multiplies
# the whole conv row by them; the channel's shift survives) and, at the sites without a BatchNorm, whole rows scaled
# down or zeroed with their bias left alone. Not function-preserving: the truth is the float64 oracle on this dict.
DEAD_SEED = 433
DEAD_GAMMAS = (0.0, 2.0 ** -100, 2.0 ** -118, 2.0 ** -130, -2.0 ** -120)   # 2^-100: the control, above the threshold
DEAD_VARS = (0.0, 1e6)
# Sites whose running_var = 0 sits on a live channel: the first block of both trunks (a hidden channel). Measured,
# worst fraction of a bar, fp32 / emulated-f16x3 oracle against float64 on the five sweep scenes: none 0.11 / 0.09,
# layer1.0 0.17 / 0.19, layer3.5 7.7 / 9.2, layer4.2 3.7 / 7.7 (keyval grows to 1e3 and the tf decoder's softmax
# sharpens: the function itself turns ill-conditioned), every block: not finite. layer1.0 is the count that holds.
DEAD_LIVE_VAR0 = ("layer1.0.conv1.weight",)
DEAD_ROW_SCALES = (2.0 ** -118, 2.0 ** -135, 0.0)
# rows edited per scale at a site without BatchNorm: the largest count tried at which the fp32 oracle stays within half
# of every bar of the float64 oracle (test_weight_range.py asserts it)
DEAD_ROWS_PER_SCALE = 2
_BN_OF = ((".conv1", ".bn1"), (".conv2", ".bn2"), (".conv3", ".bn3"), (".downsample.0", ".downsample.1"))
# 2-D .weight tensors that are looked up, never multiplied: no weight split reads them
NOT_SPLIT = ("_keyval_embedding.weight", "_query_embedding.weight")
# the attention in-projections the forward reads only in part: (first row, rows) of the part it splits. The ego
# cross-attention has one key, its softmax is 1 and only the value rows d .. 3d reach the output.
IN_PROJ_ROWS = {"cross_ego_attention.in_proj_weight": (512, 256)}


def bn_of(sd, conv):
    """BatchNorm prefix folded into the conv with parameter prefix ``conv``, or None."""
    for c, b in _BN_OF:
        if conv.endswith(c) and conv[:-len(c)] + b + ".running_var" in sd:
            return conv[:-len(c)] + b
    return None


def split_sites(sd):
    """Every weight tensor a weight split reads, from the dict alone: (key, BatchNorm prefix or None, first row, rows).
    The matrices and conv kernels named ``.weight`` or ``in_proj_weight``, less NOT_SPLIT."""
    out = []
    for k, v in sd.items():
        if not (k.endswith(".weight") or k.endswith("in_proj_weight")) or np.ndim(v) not in (2, 4) or k in NOT_SPLIT:
            continue
        row0, rows = next((r for s, r in IN_PROJ_ROWS.items() if k.endswith(s)), (0, np.shape(v)[0]))
        out.append((k, bn_of(sd, k[:-len(".weight")]) if k.endswith(".weight") else None, row0, rows))
    return out


def dead_rows(seeded_sd, per_scale=DEAD_ROWS_PER_SCALE, seed=DEAD_SEED):
    """(dict, edits): at every conv with a BatchNorm (the BasicBlocks' conv1 / conv2, the stems, the downsamples) one
    gamma each of DEAD_GAMMAS on distinct channels and the running_var edits described below; at every other site of
    ``split_sites`` with at least 4 rows, ``per_scale`` rows times each of DEAD_ROW_SCALES (one each where the site has
    fewer than 18 rows), biases untouched. ``edits`` maps a site's key to the list of (row, what) it received."""
    sd = _copy(seeded_sd)
    rng = np.random.default_rng(seed)
    edits = {}
    for key, bn, row0, rows in split_sites(sd):
        if bn is not None:
            pick = rng.permutation(rows)[: len(DEAD_GAMMAS) + 2]
            for ch, g in zip(pick, DEAD_GAMMAS):
                sd[bn + ".weight"][ch] = np.float32(g)
            # running_var = 0 multiplies the folded scale by 1 / sqrt(eps) = 316. On a live channel of every block
            # that compounds along the residual stream (measured in float64: 1e4 after layer1.0, 1e38 in layer4, inf
            # in fp32), so it sits on the 2^-130 channel (316 x 2^-130 is still under the threshold) everywhere and
            # on a live channel only at the sites of DEAD_LIVE_VAR0; 1e6 (x 1e-3) is on a live channel everywhere.
            var0 = [pick[DEAD_GAMMAS.index(2.0 ** -130)]] + ([pick[-2]] if key.endswith(DEAD_LIVE_VAR0) else [])
            for ch in var0:
                sd[bn + ".running_var"][ch] = np.float32(DEAD_VARS[0])
            sd[bn + ".running_var"][pick[-1]] = np.float32(DEAD_VARS[1])
            edits[key] = ([(int(ch), f"gamma {g!r}") for ch, g in zip(pick, DEAD_GAMMAS)]
                          + [(int(ch), f"var {DEAD_VARS[0]!r}") for ch in var0]
                          + [(int(pick[-1]), f"var {DEAD_VARS[1]!r}")])
            continue
        if rows < 4:
            continue
        n = max(1, min(per_scale, rows // (3 * len(DEAD_ROW_SCALES))))
        pick = row0 + rng.permutation(rows)[: n * len(DEAD_ROW_SCALES)]
        edits[key] = []
        for i, r in enumerate(pick):
            c = DEAD_ROW_SCALES[i % len(DEAD_ROW_SCALES)]
            sd[key][r] *= np.float32(c)
            edits[key].append((int(r), f"row x {c!r}"))
    return sd, edits


VARIANTS = {"rescaled": rescaled, "rescaled_var": rescaled_var, "rescaled_signed": rescaled_signed}
