"""Shared pieces of tests/test_attn_views_gpu.py and its CPU companion tests/test_attn_views.py (pure torch / numpy:
importable without a GPU): the cases - small MHA on the forward's strided q / k / v forms, the BEV sampling family with
`samples` scenes per map on a square and a non-square map, the pooling into the token slab - as guarded operands
(tests/guard_util.py), their float64 references written from the plain definitions, and numpy restatements of the
strided operations that can be run with one deliberate fault each, so the CPU file can show that the comparisons the
GPU file makes would notice it."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from decoder_edge_util import tap_pixels
from guard_util import SENTINEL, guarded

NAN = float("nan")


def rnd(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


# ------------------------------------------------------------------------------------------------------- MHA
# form "qkv": q | k | v are windows of one (B, L, 3d) buffer (the decoder's self-attention); "kv": q dense, K | V
# interleaved in a (B / kv_div, Lk, 2d) buffer (cross-attention on the keyval slab; the agent K / V shared by kv_div
# scenes). pad: floats every leading dimension is wider than needed; extra: rows every batch stride is longer.
MHA_CASES = {
    "M1": dict(B=2, Lq=31, Lk=31, nh=8, hd=32, kv_div=1, form="qkv", pad=0, extra=0),
    "M2": dict(B=3, Lq=31, Lk=65, nh=8, hd=32, kv_div=1, form="kv", pad=0, extra=0),
    "M3": dict(B=6, Lq=20, Lk=30, nh=8, hd=32, kv_div=3, form="kv", pad=0, extra=0),
    "M3-div1": dict(B=2, Lq=20, Lk=30, nh=8, hd=32, kv_div=1, form="kv", pad=0, extra=0),
    "M1'": dict(B=2, Lq=31, Lk=31, nh=8, hd=32, kv_div=1, form="qkv", pad=8, extra=1),
    "M2'": dict(B=3, Lq=31, Lk=65, nh=8, hd=32, kv_div=1, form="kv", pad=8, extra=1),
    "M4": dict(B=2, Lq=131, Lk=65, nh=3, hd=32, kv_div=2, form="kv", pad=0, extra=0, ldkv=200),
    "M4-hd48": dict(B=2, Lq=131, Lk=127, nh=1, hd=48, kv_div=1, form="kv", pad=8, extra=0),
}
MHA_LD = {"M1": (768, 768, 256), "M2": (256, 512, 256), "M3": (256, 512, 256), "M1'": (776, 776, 264),
          "M2'": (264, 520, 264), "M4": (96, 200, 96), "M4-hd48": (56, 104, 56)}  # (ldq, ldkv, ldo) as the issue sets


def mha_lds_bytes(hd, Lq, Lk):
    """launch_mha_small's LDS need of the whole-head form (decoder.hip); above 64 KiB the per-row fallback runs."""
    return 4 * (Lq * (hd + 1) + Lk * (hd + 1) + Lk * hd + Lq * (Lk + 1))


def mha_values(name):
    """The logical q (B, Lq, d), k, v (B / kv_div, Lk, d) of a case: distinct per scene and per K / V batch. M3 and
    its kv_div = 1 companion share K / V; the companion's queries are scenes 0 and 3 of M3."""
    c = MHA_CASES[name]
    d, key = c["nh"] * c["hd"], {"M3-div1": "M3", "M1'": "M1", "M2'": "M2"}.get(name, name)
    k0 = MHA_CASES[key]
    seed = 400 + 10 * sorted(MHA_CASES).index(key)
    q = rnd(k0["B"], c["Lq"], d, seed=seed)
    k = rnd(k0["B"] // k0["kv_div"], c["Lk"], d, seed=seed + 1)
    v = rnd(k0["B"] // k0["kv_div"], c["Lk"], d, seed=seed + 2)
    if name == "M3-div1":
        q = q[[0, 3]].contiguous()
    return q, k, v


def mha_ref(q, k, v, nh, kv_div):
    """softmax(q_h k_h^T / sqrt(hd)) v_h per (scene, head) in float64; scene b attends K / V batch b // kv_div."""
    B, Lq, d = q.shape
    hd = d // nh
    kk = k.double().repeat_interleave(kv_div, 0).view(B, -1, nh, hd).transpose(1, 2)
    vv = v.double().repeat_interleave(kv_div, 0).view(B, -1, nh, hd).transpose(1, 2)
    qq = q.double().view(B, Lq, nh, hd).transpose(1, 2)
    return (torch.softmax(qq @ kk.transpose(-1, -2) / np.sqrt(hd), -1) @ vv).transpose(1, 2).reshape(B, Lq, d)


def mha_operands(name, poison, device="cpu"):
    """The case as guarded operands. Offsets (floats) are relative to each allocation's flat tensor ``.t`` so the
    ctypes call (data_ptr + 4 off) and the numpy restatement (flat[off + ...]) address the same words."""
    c = MHA_CASES[name]
    B, Lq, Lk, nh, hd, kv_div = (c[x] for x in ("B", "Lq", "Lk", "nh", "hd", "kv_div"))
    d, Bkv, pad, extra = nh * hd, B // kv_div, c["pad"], c["extra"]
    q, k, v = mha_values(name)
    o = types.SimpleNamespace(B=B, Lq=Lq, Lk=Lk, nh=nh, hd=hd, kv_div=kv_div, d=d, q=q, k=k, v=v, name=name)
    if c["form"] == "qkv":
        assert Lq == Lk and kv_div == 1
        ld = 3 * d + pad
        bs = (Lq + extra) * ld
        o.Q = o.KV = guarded((B, Lq, 3 * d), (bs, ld, 1), poison, values=torch.cat([q, k, v], -1), device=device)
        o.ldq = o.ldkv = ld
        o.qbs = o.kvbs = bs
        o.q_off, o.k_off, o.v_off = o.Q.offset, o.Q.offset + d, o.Q.offset + 2 * d
    else:
        o.ldq = d + pad
        o.qbs = (Lq + extra) * o.ldq
        o.Q = guarded((B, Lq, d), (o.qbs, o.ldq, 1), poison, values=q, device=device)
        o.ldkv = c.get("ldkv", 2 * d + pad)
        o.kvbs = (Lk + extra) * o.ldkv
        o.KV = guarded((Bkv, Lk, 2 * d), (o.kvbs, o.ldkv, 1), poison, values=torch.cat([k, v], -1), device=device)
        o.q_off, o.k_off, o.v_off = o.Q.offset, o.KV.offset, o.KV.offset + d
    o.ldo = d + pad
    o.obs = (Lq + extra) * o.ldo
    o.O = guarded((B, Lq, d), (o.obs, o.ldo, 1), SENTINEL, device=device)
    return o


def mha_strided(o, fault=None):
    """launch_mha_small's addressing restated in numpy float64 on the flat allocations of mha_operands (device "cpu").
    Faults: "mod" - K / V batch b % kv_div for b / kv_div; "ldkv" - the key / value row stride taken as d on the
    interleaved buffer; "v_at_k" - v read at k's offset. Returns the (B, Lq, d) result."""
    qf, kvf = o.Q.t.numpy().astype(np.float64), o.KV.t.numpy().astype(np.float64)
    e = np.arange(o.hd)
    out = np.full((o.B, o.Lq, o.d), np.nan)
    ldkv = o.d if fault == "ldkv" else o.ldkv
    v_off = o.k_off if fault == "v_at_k" else o.v_off
    for b in range(o.B):
        kb = b % o.kv_div if fault == "mod" else b // o.kv_div
        for h in range(o.nh):
            qi = o.q_off + b * o.qbs + np.arange(o.Lq)[:, None] * o.ldq + h * o.hd + e
            ki = o.k_off + kb * o.kvbs + np.arange(o.Lk)[:, None] * ldkv + h * o.hd + e
            vi = v_off + kb * o.kvbs + np.arange(o.Lk)[:, None] * ldkv + h * o.hd + e
            s = qf[qi] @ kvf[ki].T / np.sqrt(o.hd)
            with np.errstate(invalid="ignore", over="ignore"):
                p = np.exp(s - s.max(-1, keepdims=True))
                out[b, :, h * o.hd:(h + 1) * o.hd] = (p / p.sum(-1, keepdims=True)) @ kvf[vi]
    return out


def store_rows(G, body, extra_channels=0):
    """Store ``body`` (the view's shape, or ``extra_channels`` wider in the last dim) through the guarded output's
    strides into its flat allocation, as a kernel would: a store past the declared channels lands where the strides
    put it."""
    flat = G.t.numpy()
    body = np.asarray(body, np.float32)
    assert body.shape[:-1] == G.shape[:-1] and body.shape[-1] == G.shape[-1] + extra_channels
    idx = np.zeros(body.shape, np.int64) + G.offset
    for ax, st in enumerate(G.strides):
        shp = [1] * body.ndim
        shp[ax] = body.shape[ax]
        idx = idx + (np.arange(body.shape[ax]) * st).reshape(shp)
    # the overshoot first: the stores of the following rows land on top of it, as the kernel's own would
    C = G.shape[-1]
    flat[idx[..., C:].reshape(-1)] = body[..., C:].reshape(-1)
    flat[idx[..., :C].reshape(-1)] = body[..., :C].reshape(-1)


# --------------------------------------------------------------------------------------------------- sampling
# D decoder scenes, S per perception scene; scales are powers of two so the hand-placed points are exact in fp32
GEOMS = {
    "forward": dict(D=6, S=3, Q=20, P=8, Hv=64, Wv=64, C=256, inv_max_x=1.0 / 32.0, inv_max_y=1.0 / 32.0),
    "nonsquare": dict(D=4, S=2, Q=5, P=3, Hv=6, Wv=10, C=12, inv_max_x=1.0 / 16.0, inv_max_y=1.0 / 64.0),
}
MIN_PX = 1e-3  # every random point lies, in float64, at least this far from an integer in both pixel coordinates


def pixel_coords64(pts, g):
    """(ix, iy) of float32 points in float64 (the scales as the float32 the kernel receives)."""
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    ix = ((p[:, 1] * float(np.float32(g["inv_max_x"])) + 1) * g["Wv"] - 1) / 2
    iy = ((p[:, 0] * float(np.float32(g["inv_max_y"])) + 1) * g["Hv"] - 1) / 2
    return ix, iy


def point_at(ix, iy, g):
    """The float32 point whose pixel coordinates are nearest (ix, iy)."""
    ty = ((2 * ix + 1) / g["Wv"] - 1) / g["inv_max_x"]
    tx = ((2 * iy + 1) / g["Hv"] - 1) / g["inv_max_y"]
    return np.array([tx, ty], np.float32)


def hand_targets(g):
    """[(label, ix, iy, exact)] of the hand-placed points of scene 0. ``exact``: the target has a float32 point whose
    ix, iy come out exactly in the kernel's fp32 arithmetic - always for a power-of-two map side; on the 6 x 10 map
    only where (2 ix + 1) / Wv is dyadic (the corners, ix = -0.5, the centres ix in {2, 7}, iy in {1, 4}): ix = -1 and
    ix = Wv - 1 need grid x = -1.1 and 0.9 there, so those two are placed at the nearest float32 point."""
    Hv, Wv = g["Hv"], g["Wv"]
    corners = [("corner nw", -0.5, -0.5, True), ("corner ne", Wv - 0.5, -0.5, True),
               ("corner sw", -0.5, Hv - 0.5, True), ("corner se", Wv - 0.5, Hv - 0.5, True)]
    if (Hv, Wv) == (64, 64):
        return corners + [("ix = -1", -1.0, 9.5, True), ("ix = Wv - 1", 63.0, 9.5, True), ("ix = -0.5", -0.5, 9.5, True),
                          ("iy = -1", 9.5, -1.0, True), ("iy = Hv - 1", 9.5, 63.0, True),
                          ("centre", 5.0, 9.0, True), ("centre 2", 40.0, 17.0, True),
                          ("same pixel a", 20.25, 30.25, True), ("same pixel b", 20.75, 30.5, True)]
    assert (Hv, Wv) == (6, 10)  # grid x = k / 16: ix = 4.5 + 0.3125 k; grid y = k / 16: iy = 2.5 + 0.1875 k
    return corners + [("ix = -1", -1.0, 2.5, False), ("ix = Wv - 1", 9.0, 2.5, False), ("ix = -0.5", -0.5, 2.5, True),
                      ("centre", 2.0, 1.0, True), ("centre 2", 7.0, 4.0, True),
                      ("same pixel a", 4.5, 2.5, True), ("same pixel b", 4.8125, 2.6875, True)]


def sample_case(name):
    """logits (D, Q, P), pts (D, Q, P, 2) float32, value (D, Hv, Wv, C) NHWC (one map per decoder scene: a launch with
    `samples` = S reads the first D / S of them). Scene 0 starts with the hand-placed points; scene D - 2 has every
    point in one pixel; scene D - 1 has every point off the map; every other point is uniform within 1.15 of the map's
    half extent, redrawn (fixed seed) until it lies MIN_PX from an integer in both pixel coordinates."""
    g = dict(GEOMS[name])
    D, Q, P, Hv, Wv, C = (g[x] for x in ("D", "Q", "P", "Hv", "Wv", "C"))
    rng = np.random.default_rng(20 + len(name))
    half = np.array([1.0 / g["inv_max_y"], 1.0 / g["inv_max_x"]])

    def clear(p):
        ix, iy = pixel_coords64(p, g)
        return (np.abs(ix - np.rint(ix)) >= MIN_PX) & (np.abs(iy - np.rint(iy)) >= MIN_PX)

    pts = (rng.uniform(-1.15, 1.15, (D * Q * P, 2)) * half).astype(np.float32)
    redrawn = 0
    while not clear(pts).all():
        bad = np.flatnonzero(~clear(pts))
        redrawn += len(bad)
        pts[bad] = (rng.uniform(-1.15, 1.15, (len(bad), 2)) * half).astype(np.float32)
    pts = pts.reshape(D, Q * P, 2)
    # scene D - 2: one pixel; scene D - 1: off the map (grid x in [1.3, 1.6): ix >= 1.15 Wv - 0.5 >= Wv)
    px, py = Wv - 3, 1
    for u in range(Q * P):
        pts[D - 2, u] = point_at(px + rng.uniform(0.1, 0.9), py + rng.uniform(0.1, 0.9), g)
        pts[D - 1, u, 1] = np.float32(rng.uniform(1.3, 1.6) / g["inv_max_x"])
    hand = hand_targets(g)
    for u, (_, ix, iy, _) in enumerate(hand):
        pts[0, u] = point_at(ix, iy, g)
    random_mask = np.ones((D, Q * P), bool)
    random_mask[0, :len(hand)] = False
    g.update(logits=rnd(D, Q, P, seed=431, scale=2.0), pts=torch.from_numpy(pts.reshape(D, Q, P, 2).copy()),
             value=rnd(D, Hv, Wv, C, seed=433), hand=hand, random_mask=random_mask.reshape(-1), redrawn=redrawn,
             one_pixel=(py, px), name=name)
    return g


def sample_ref(logits, pts, value, S, g):
    """sum_p softmax(logits)_p grid_sample(value[b // S], pts_p) in float64 (zero padding, align_corners=False):
    grid x = pts[..., 1] inv_max_x, grid y = pts[..., 0] inv_max_y."""
    D = logits.shape[0]
    sx, sy = float(np.float32(g["inv_max_x"])), float(np.float32(g["inv_max_y"]))
    grid = torch.stack([pts[..., 1].double() * sx, pts[..., 0].double() * sy], -1)
    maps = value[:D // S].double().repeat_interleave(S, 0).permute(0, 3, 1, 2)
    s = F.grid_sample(maps, grid, mode="bilinear", padding_mode="zeros", align_corners=False)  # (D, C, Q, P)
    return (torch.softmax(logits.double(), -1).unsqueeze(1) * s).sum(-1).permute(0, 2, 1).contiguous()


def sample_restated(logits, pts, value, S, g, fault=None):
    """bev_sample_attn_kernel's indexing restated in numpy float64. Faults: "map_b" - scene b reads map b for b / S;
    "hw" - Hv and Wv exchanged in the pixel coordinates, the bounds and the row pitch; "scales" - the two scales
    exchanged."""
    lg, p, val = logits.double().numpy(), pts.double().numpy(), value.double().numpy()
    D, Q, P = lg.shape
    Hv, Wv, C = value.shape[1:]
    sx, sy = float(np.float32(g["inv_max_x"])), float(np.float32(g["inv_max_y"]))
    if fault == "scales":
        sx, sy = sy, sx
    H, W = (Wv, Hv) if fault == "hw" else (Hv, Wv)
    w = np.exp(lg - lg.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    ix = ((p[..., 1] * sx + 1) * W - 1) / 2
    iy = ((p[..., 0] * sy + 1) * H - 1) / 2
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    out = np.zeros((D, Q, C))
    for b in range(D):
        m = val[b if fault == "map_b" else b // S].reshape(Hv * Wv, C)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            yy, xx = y0[b] + dy, x0[b] + dx
            wt = (1 - np.abs(ix[b] - xx)) * (1 - np.abs(iy[b] - yy))
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            rows = m[np.where(ok, yy * W + xx, 0)]  # (Q, P, C)
            out[b] += ((w[b] * wt * ok)[..., None] * rows).sum(1)
    return out


def dedup_restated(pts, g, S, fault=None):
    """bev_tap_dedup_kernel's tables built by a plain per-scene loop from tap_pixels. Faults: "row_base" - the row
    block of scene b taken from b / S; "map_b" - the pixel's map image taken as b."""
    D, Q, P, Hv, Wv = (g[x] for x in ("D", "Q", "P", "Hv", "Wv"))
    cap = Q * P * 4
    pix, _, _ = tap_pixels(pts, D, Q, P, Hv, Wv, 1 if fault == "map_b" else S, g["inv_max_x"], g["inv_max_y"])
    rows = np.full(D * cap, -1, np.int32)
    slots = np.full(D * cap, -1, np.int32)
    for b in range(D):
        base = (b // S if fault == "row_base" else b) * cap
        tp = pix[b * cap:(b + 1) * cap]
        uniq = np.unique(tp[tp >= 0])
        rows[base:base + cap] = -1
        rows[base:base + len(uniq)] = uniq
        where = {int(p_): base + i for i, p_ in enumerate(uniq)}
        slots[b * cap:(b + 1) * cap] = [where.get(int(t), -1) for t in tp]
    return rows, slots


# ---------------------------------------------------------------------------------------------------- pooling
T = 320  # tokens per scene of the GPT slab: 256 image rows, then 64 LiDAR rows


def token_slab(B, C, oh, ow, device="cpu"):
    """A guarded (B, T, C) slab whose every word - guards and body - holds the sentinel, and the window of its first
    oh ow rows per scene (body NaN) as the (B, oh, ow, C) pooled-token view: rows oh ow .. T - 1 of every scene lie
    outside the window and must keep the sentinel."""
    slab = guarded((B, T, C), (T * C, C, 1), SENTINEL, device=device)
    slab.t.view(torch.int32)[slab.mask] = int(np.array([SENTINEL], np.uint32).view(np.int32)[0])
    tk = slab.window((B, oh, ow, C), (T * C, ow * C, C, 1))
    tk.view()[...] = NAN
    tk.expect = tk.t.view(torch.int32).clone()
    return slab, tk


def pool_case(B, H, W, C, seed):
    """in (B, H, W, C) NHWC and the (T, C) position table."""
    return rnd(B, H, W, C, seed=seed), rnd(T, C, seed=seed + 1)


def pool_ref(x, oh, ow, add=None):
    """adaptive_avg_pool2d in float64 (+ the position rows) -> (B, oh, ow, C)."""
    r = F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), (oh, ow)).permute(0, 2, 3, 1)
    if add is not None:
        r = r + add.double().view(oh, ow, -1)
    return r.contiguous()


def pool_restated(x, oh, ow, pos, fault=None):
    """avgpool_kernel's arithmetic in numpy float32 (window sum in (dy, dx) order, * 1 / (kh kw), + the position row).
    Faults: "no_row" - the position row's offset (y ow + x) C dropped, every token gets row 0; "past_c" - one channel
    more than C stored per token (a plain 1.0). Returns (B, oh, ow, C) or, for "past_c", (B, oh, ow, C + 1)."""
    xn = x.numpy().astype(np.float32)
    B, H, W, C = xn.shape
    kh, kw = H // oh, W // ow
    s = np.zeros((B, oh, ow, C), np.float32)
    for dy in range(kh):
        for dx in range(kw):
            s = s + xn[:, dy::kh, dx::kw]
    v = s * np.float32(1.0 / (kh * kw))
    if pos is not None:
        add = pos.numpy().astype(np.float32)[:oh * ow].reshape(oh, ow, C)
        v = v + (add[:1, :1] if fault == "no_row" else add)
    if fault == "past_c":
        v = np.concatenate([v, np.ones((B, oh, ow, 1), np.float32)], -1)
    return v
