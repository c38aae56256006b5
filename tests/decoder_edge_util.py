"""Shared pieces of the decoder / f16x3 edge-case tests (test_decoder_edges_gpu.py and its CPU companion
test_decoder_edges.py): the doctored state dicts and noise tensors that drive the trajectory head's kernels to
their edges, the single-weight edits that overflow one f16x3 site each, a recorder of the CPU oracle's activations,
and the tap-geometry / dedup check of the gathered value_proj rows."""
import contextlib

import numpy as np

DL = "_trajectory_head.diff_decoder.layers."
BATCH, INPUT_SEED = 2, 7
F16_MAX = 65504.0

CASES = ("clamp_noise", "offmap_l1", "tied_cls", "equal_modes")


def clamp_noise(noise):
    """Scene 0 as drawn, scene 1 x 40: every point of scene 1 clamps to a corner of the normalised range
    (x = 55.7 is off the 64 x 64 BEV map, y = 26 / -20 on it)."""
    nz = np.array(noise, dtype=np.float32, copy=True)
    nz[1] *= 40.0
    return nz


def make_case(seeded_sd, name):
    """(state dict, inputs) of an "A" case: a copy of the seeded dict with the named edit, and the B = 2 synthetic
    batch with the case's noise."""
    from diffusiondrive_amd.weights import synthetic_inputs
    sd = {k: np.array(v, copy=True) for k, v in seeded_sd.items()}
    inp = dict(synthetic_inputs(BATCH, INPUT_SEED))
    nz = inp["noise"]
    if name == "clamp_noise":
        nz = clamp_noise(nz)
    elif name == "offmap_l1":
        # layer 0 regresses every point 64 m up (off the map: layer 1's taps are all zero-padded), layer 1 back down
        sd[DL + "0.task_decoder.plan_reg_branch.4.bias"][0::3] += 64.0
        sd[DL + "1.task_decoder.plan_reg_branch.4.bias"][0::3] -= 64.0
        nz = clamp_noise(nz)
    elif name == "tied_cls":
        sd[DL + "1.task_decoder.plan_cls_branch.6.weight"][:] = 0.0
    elif name == "equal_modes":
        a = sd["_trajectory_head.plan_anchor"]
        a[:] = a[7]
        nz = np.array(nz, copy=True)
        nz[:] = nz[:, :1]
    else:
        raise KeyError(name)
    inp["noise"] = np.ascontiguousarray(nz, dtype=np.float32)
    return sd, inp


# One edit per f16x3 site: site -> (key, "mul" | "add", factor, probe kind, probe prefix). The probe names the oracle
# activation that enters the site: ("ln_out", p) the output of layer_norm p, ("in", p) the input of linear / conv p.
OVERFLOW_SITES = {
    "decoder_mk": (DL + "0.norm3.weight", "mul", 1e6, "in", DL + "0.task_decoder.plan_cls_branch.0"),
    "tfdec_mk": ("_tf_decoder.layers.0.norm1.weight", "mul", 1e6, "ln_out", "_tf_decoder.layers.0.norm1"),
    "gpt_tail": ("_backbone.transformers.0.blocks.0.ln2.weight", "mul", 1e6, "in",
                 "_backbone.transformers.0.blocks.0.mlp.0"),
    "value_proj": ("bev_proj.2.weight", "mul", 1e6, "in", DL + "0.cross_bev_attention.value_proj.0"),
    "bevproj": ("_backbone.up_conv4.bias", "add", 1e6, "in", "bev_proj.0"),
    "gpt_attention": ("_backbone.transformers.0.blocks.0.attn.value.bias", "add", 1e6, "in",
                      "_backbone.transformers.0.blocks.0.attn.proj"),
}


def make_overflow_sd(seeded_sd, site):
    key, op, val = OVERFLOW_SITES[site][:3]
    sd = dict(seeded_sd)
    a = np.array(sd[key], dtype=np.float32, copy=True)
    sd[key] = a * np.float32(val) if op == "mul" else a + np.float32(val)
    return sd


@contextlib.contextmanager
def record_oracle_activations(rec):
    """While active, the oracle's layer_norm / linear / conv record max |activation| by parameter prefix into ``rec``:
    ("in", p) the input of linear / conv p, ("ln_out", p) the output of layer_norm p (max over the calls)."""
    import oracle.model as om
    orig = om.layer_norm, om.linear, om.conv

    def note(kind, p, t):
        rec[(kind, p)] = max(rec.get((kind, p), 0.0), float(t.detach().abs().max()))

    def layer_norm(x, sd, p):
        y = orig[0](x, sd, p)
        note("ln_out", p, y)
        return y

    def linear(x, sd, p, *a, **k):
        note("in", p, x)
        return orig[1](x, sd, p, *a, **k)

    def conv(x, sd, p, *a, **k):
        note("in", p, x)
        return orig[2](x, sd, p, *a, **k)

    om.layer_norm, om.linear, om.conv = layer_norm, linear, conv
    try:
        yield rec
    finally:
        om.layer_norm, om.linear, om.conv = orig


def tap_pixels(pts, B, Q=20, P=8, HB=64, WB=None, samples=1, inv_max_x=1.0 / 32.0, inv_max_y=1.0 / 32.0):
    """The map pixel every bilinear tap of every point reads, (B*Q*P*4,) int64 in the order nw, ne, sw, se, -1 where
    zero padding applies: bev_tap_geometry (decoder.hip) restated in float32 numpy in the kernel's operation order -
    grid x = pts[:, 1] * inv_max_x over the map's width WB, grid y = pts[:, 0] * inv_max_y over its height HB, every
    operation a single rounding, so the floor is the kernel's. Scene b reads map image b // samples. Also returns
    (ix, iy) as float32."""
    WB = HB if WB is None else WB
    one, two = np.float32(1), np.float32(2)
    p32 = np.asarray(pts).astype(np.float32).reshape(B * Q * P, 2)
    ix = ((p32[:, 1] * np.float32(inv_max_x) + one) * np.float32(WB) - one) / two
    iy = ((p32[:, 0] * np.float32(inv_max_y) + one) * np.float32(HB) - one) / two
    assert ix.dtype == np.float32 and iy.dtype == np.float32
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    img = np.arange(B * Q * P) // (Q * P) // samples
    pix = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < HB) & (xx >= 0) & (xx < WB)
        pix.append(np.where(ok, (img * HB + yy) * WB + xx, -1))
    return np.stack(pix, 1).reshape(-1), ix, iy


def check_gathered_taps(pts, rows, slots, counts, vals, dense, B, tol, Q=20, P=8, HB=64, WB=None, samples=1,
                        inv_max_x=1.0 / 32.0, inv_max_y=1.0 / 32.0):
    """The gathered value_proj's dedup of one (step, layer) against the points it was made from.

    ``pts`` (B*Q*P, 2) the layer's trajectory points (the device's own), ``rows`` / ``slots`` (B*Q*P*4,) and ``counts``
    (B,) the int32 dedup tables (``counts`` None: not checked), ``vals`` (B*Q*P*4, C) the gathered rows (None: not
    checked), ``dense`` (B/samples*HB*WB, C) the fp32 dense value map of the layer. The tap geometry (tap_pixels)
    follows F.grid_sample's align_corners=False / zero padding in float32 arithmetic; ``samples`` consecutive scenes
    read one map image (pixel index from b // samples) while each scene's row list stays at its own base b * Q*P*4.
    Each scene's row list is exactly its distinct in-map tap pixels in pixel order, -1 past the count; the counts
    match; every tap's slot is -1 exactly where the tap is zero-padded and points to its pixel otherwise, inside its
    own scene's block; every live gathered row equals the dense map at its pixel within ``tol`` (relative to
    max(1, max |map row|)).
    Returns (padded taps, live taps, max relative row error)."""
    cap = Q * P * 4
    pix, _, _ = tap_pixels(pts, B, Q, P, HB, WB, samples, inv_max_x, inv_max_y)
    for s_ in range(B):
        tp = pix[s_ * cap:(s_ + 1) * cap]
        uniq = np.unique(tp[tp >= 0])
        rs = rows[s_ * cap:(s_ + 1) * cap]
        assert np.array_equal(rs[:len(uniq)], uniq) and (rs[len(uniq):] == -1).all(), s_
        if counts is not None:
            assert counts[s_] == len(uniq), (s_, counts[s_], len(uniq))  # the compacted launch's row counts
    assert np.array_equal(slots < 0, pix < 0)
    live = slots >= 0
    assert np.array_equal(slots[live] // cap, np.flatnonzero(live) // cap), "a slot outside its scene's row block"
    assert np.array_equal(rows[slots[live]], pix[live])
    used = rows >= 0
    err = 0.0
    if vals is not None and used.any():
        ref = dense[rows[used]]
        err = float(np.abs(vals[used] - ref).max() / max(1.0, np.abs(ref).max()))
    assert err <= tol, err
    return int((pix < 0).sum()), int((pix >= 0).sum()), err
