"""Row tables, float64 reference and comparison for value_proj.hip through dd_op_vproj (pure numpy / torch: importable
without a GPU; tests/test_vproj_tables.py holds this file to its purpose, tests/test_vproj_tables_gpu.py runs it on the
device).

The op: value rows = ReLU(conv3x3(map) + bias) at listed pixels. ``map`` holds nimg images (64, 64, 256) NHWC, a row
key is image * 4096 + pixel, rows[b * cap + l] (l < counts[b]) is group b's l-th key (distinct and ascending within a
group, as the decoder's dedup writes them; -1 past the count) and row b * cap + l of ``out`` receives its 256 values.
The kernels walk the live rows compacted over the groups in order, in tiles of 256.

Tables. ``Table`` derives, in numpy and from the definition alone, what the union-staged kernel has to decide per tile:
the union of the in-map 3 x 3 neighbourhoods of the tile's keys and range = max key - min key + 131 (the bitmap spans
[min - 65, max + 65]). A tile falls back to the gathered kernel when its range exceeds ``range_keys`` ("range") or its
union exceeds min(``umax_rows``, the launch's umax) ("union"); both limits come from dd_op_vproj_limits, never from a
constant here. Every named case asserts on the CPU that it is what its name says.

Reference: float64 from the definition - per live row the 9 x 256 in-map neighbours (zero outside the map) times the
fp32 weights taken to float64, plus bias; ReLU is applied by the comparison. Nothing is read from the device or from
another kernel.

Comparison: per element the f16x3 bound of f16x3_emul.py, err <= rho D + T through terms / measure_rho / bound_ratio
(relu=True) on the gathered im2col rows; rho is measured (4 x the larger of the emulation's and plain fp32's ratio on
the same rows) and must stay <= RHO_MAX. Every element of every live row is compared. ``out`` is pre-filled with
guard_util's sentinel: a row at or past its group's count must keep the sentinel bits, a live row must have lost them
in every element.

Input families: "benign" (unit-scale map, fan-in-scaled weights), "groupscale8" (input-channel group g of 16 has its
map values x 2^-e_g and its weights x 2^e_g, e_g in -8 .. 8 with both extremes present and next to each other: the
function is unchanged, a wrong group-to-split assignment or a swapped hi / lo half is not) and "small" (the map x 2^-5:
every activation below 2^-2, every lo part subnormal in fp16).
"""
import functools

import numpy as np
import torch

import f16x3_cases as C
import f16x3_emul as E
from guard_util import SENTINEL, guarded

HW, CH, TAPS = 64, 256, 9
PIX = HW * HW
KK = TAPS * CH
TILE = 256
RANGE_PAD = 131            # the bitmap covers [min - 65, max + 65]
FAMILIES = ("benign", "groupscale8", "small")
SENT_BITS = int(np.array([SENTINEL], np.uint32).view(np.int32)[0])
SENT_F32 = float(np.array([SENTINEL], np.uint32).view(np.float32)[0])
UMAX_OFF = 1 << 30         # the launch's umax when it is not in play


def limits():
    """(umax_rows, range_keys) of the library: the union kernel's staging capacity and the key range of its bitmap."""
    import ctypes
    from diffusiondrive_amd import _lib
    u, r = ctypes.c_int(), ctypes.c_int()
    assert _lib.load().dd_op_vproj_limits(ctypes.byref(u), ctypes.byref(r)) == 0
    return u.value, r.value


# ------------------------------------------------------------------------------------------------ geometry
def neighbours(keys):
    """(M, 9) keys of the 3 x 3 neighbourhood of each key, tap order (kh, kw), -1 where the tap leaves the map."""
    keys = np.asarray(keys, np.int64)
    n, p = keys // PIX, keys % PIX
    y, x = p // HW, p % HW
    yy = y[:, None] + np.repeat([-1, 0, 1], 3)[None]
    xx = x[:, None] + np.tile([-1, 0, 1], 3)[None]
    ok = (yy >= 0) & (yy < HW) & (xx >= 0) & (xx < HW)
    return np.where(ok, n[:, None] * PIX + yy * HW + xx, -1)


def block(y0, x0, h, w, img=0):
    """Keys of a dense h x w block of image ``img``, ascending."""
    y, x = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    assert y0 >= 0 and x0 >= 0 and y0 + h <= HW and x0 + w <= HW
    return np.sort((img * PIX + y * HW + x).ravel())


class Table:
    """One launch's row table. ``groups``: per group its keys (distinct, ascending). ``splits``: the K splits the case
    is run at."""

    def __init__(self, name, groups, cap, nimg, splits=(1, 8), image_scale=None, border_bump=0.0):
        self.name, self.cap, self.nimg, self.splits = name, int(cap), int(nimg), tuple(splits)
        self.B = len(groups)
        self.groups = [np.asarray(k, np.int64).reshape(-1) for k in groups]
        self.image_scale = tuple(image_scale) if image_scale is not None else (1.0,) * self.nimg
        self.border_bump = float(border_bump)
        assert 1 <= self.nimg <= self.B and len(self.image_scale) == self.nimg
        self.rows = np.full(self.B * self.cap, -1, np.int32)
        self.counts = np.zeros(self.B, np.int32)
        for b, k in enumerate(self.groups):
            assert len(k) <= self.cap and (np.diff(k) > 0).all(), "distinct and ascending within a group"
            assert len(k) == 0 or (k[0] >= 0 and k[-1] < self.nimg * PIX)
            self.rows[b * self.cap:b * self.cap + len(k)] = k
            self.counts[b] = len(k)
        self.live = np.concatenate(self.groups) if self.groups else np.zeros(0, np.int64)
        self.live_idx = np.concatenate([b * self.cap + np.arange(len(k)) for b, k in enumerate(self.groups)])
        self.group_of = np.concatenate([np.full(len(k), b) for b, k in enumerate(self.groups)])
        self.total = len(self.live)
        self.tiles = -(-self.total // TILE)
        self.union, self.range = [], []
        for t in range(self.tiles):
            k = self.live[t * TILE:(t + 1) * TILE]
            nb = neighbours(k)
            self.union.append(len(np.unique(nb[nb >= 0])))
            self.range.append(int(k.max() - k.min()) + RANGE_PAD)

    def tile_groups(self, t):
        return sorted(set(self.group_of[t * TILE:(t + 1) * TILE].tolist()))

    def fallbacks(self, umax_rows, range_keys, umax=UMAX_OFF):
        """Per tile None, "range" or "union": what the union-staged kernel must decide."""
        return ["range" if r > range_keys else "union" if u > min(umax_rows, umax) else None
                for u, r in zip(self.union, self.range)]

    def permuted(self, perm):
        """The same groups in another order in the batch (new group j = old group perm[j])."""
        return Table(self.name + "-perm", [self.groups[p] for p in perm], self.cap, self.nimg, self.splits,
                     self.image_scale, self.border_bump)


# ---------------------------------------------------------------------------------- the capacity pair
def capacity_pixels(N, rows=TILE):
    """``rows`` distinct pixels of one image whose neighbourhood union is exactly N: a spaced lattice of isolated
    pixels (9 union pixels each), then pixel by pixel the candidate whose gain in union size is nearest to what the
    remaining pixels have to bring on average, so that the last one lands on N."""
    sel = np.zeros((HW, HW), bool)
    cov = np.zeros((HW, HW), bool)

    def take(y, x):
        sel[y, x] = True
        cov[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True

    lattice = max(0, (N - 324) // 16)  # 324 = the 18 x 18 union of a dense 16 x 16 block, the least 256 rows can have
    for i in range(min(lattice, rows - 1)):
        take(20 + 3 * (i // 8), 20 + 3 * (i % 8))
    while sel.sum() < rows:
        need, rem = N - int(cov.sum()), rows - int(sel.sum())
        pad = np.pad((~cov).astype(np.int64), 1)
        gain = sum(pad[dy:dy + HW, dx:dx + HW] for dy in range(3) for dx in range(3))
        gain[sel] = -1
        ok = [int(v) for v in np.unique(gain) if v >= 0 and 0 <= need - v <= 9 * (rem - 1)]
        assert ok, f"no pixel brings the union to {N} ({need} short with {rem} to place)"
        v = min(ok, key=lambda g: (abs(g - need / rem), g))
        y, x = np.argwhere(gain == v)[0]
        take(int(y), int(x))
    keys = np.flatnonzero(sel.ravel())
    assert len(keys) == rows and int(cov.sum()) == N
    return keys


# ------------------------------------------------------------------------------------------ named cases
SPLITS_ALL = (1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def table(name, N=None):
    """The named cases. ``N``: the union size of the capacity pair (the GPU test passes the library's limit)."""
    if name == "one_row":
        t = Table(name, [[32 * HW + 32]], 4, 1, SPLITS_ALL)
        assert t.total == 1 and t.tiles == 1 and t.union == [9]
    elif name == "exact_256":
        t = Table(name, [block(10, 20, 16, 16)], 256, 1, SPLITS_ALL)
        assert t.total == 256 and t.tiles == 1 and t.union == [324]
    elif name == "257":
        t = Table(name, [np.concatenate([block(10, 20, 16, 16), [50 * HW + 7]])], 260, 1, SPLITS_ALL)
        assert t.total == 257 and t.tiles == 2 and t.union == [324, 9]
    elif name == "corners_edges":
        # image 0: its two bottom corners (a tap that runs on reads image 1's top row); image 1: the four corners, the
        # whole top row and the whole left column (a tap that runs on past 4095 leaves the map: NaN guard words)
        top_left = sorted(set(range(HW)) | set(range(0, PIX, HW)) | {HW - 1, PIX - HW, PIX - 1})
        t = Table(name, [[PIX - HW, PIX - 1], PIX + np.array(top_left)], 128, 2, border_bump=1.0e3)
        p = t.groups[1] % PIX
        assert {0, 63, 4032, 4095} <= set(p.tolist()) and set(range(64)) <= set(p.tolist())
        assert set(range(0, PIX, HW)) <= set(p.tolist()) and t.tiles == 1
        assert (neighbours(t.live) < 0).any(1).all(), "every row has a tap outside the map"
    elif name == "image_seam":
        t = Table(name, [np.arange(PIX - 32, PIX), PIX + np.arange(0, 32)], 32, 2, image_scale=(1.0, 1.0e3))
        assert t.groups[0][-1] == PIX - 1 and t.groups[1][0] == PIX and t.tiles == 1
        assert t.groups[1][0] - t.groups[0][-1] == 1, "adjacent keys across the seam"
    elif name == "empty_groups":
        t = Table(name, [[], block(5, 5, 9, 10), block(20, 30, 8, 10), [], block(40, 10, 7, 10, 1), []], 90, 2)
        assert t.counts.tolist() == [0, 90, 80, 0, 70, 0] and t.tiles == 1 and t.tile_groups(0) == [1, 2, 4]
    elif name == "range_fallback":
        g0 = np.concatenate([block(8, 8, 16, 16), block(30, 8, 4, 10)])
        t = Table(name, [g0] + [block(10 + b, 12, 4, 10, b) for b in range(1, 5)], len(g0), 5)
        assert t.B >= 5 and t.tiles == 2 and t.tile_groups(0) == [0] and t.tile_groups(1) == [0, 1, 2, 3, 4]
        assert t.range[1] > 3 * PIX + RANGE_PAD and t.range[0] < PIX, "tile 1 spans five images, tile 0 one"
    elif name in ("union_at_capacity", "union_over_capacity"):
        assert N is not None
        want = N if name == "union_at_capacity" else N + 1
        t = Table(name, [capacity_pixels(want)], 256, 1)
        assert t.total == 256 and t.tiles == 1 and t.union == [want]
    elif name == "shared_images":
        g = [block(10 + 2 * b, 10 + 3 * b, 7, 7, 0) for b in range(3)] + \
            [block(30 + 2 * b, 20 + 3 * b, 7, 8, 1) for b in range(3)]
        t = Table(name, g, 56, 2)
        assert t.B == 6 and t.nimg == 2 and t.tiles == 2
        assert (np.diff(t.live[:TILE]) < 0).sum() >= 2, "the pixel order restarts inside tile 0"
        for a, b in ((0, 1), (1, 2), (3, 4), (4, 5)):
            both = set(g[a].tolist()) & set(g[b].tolist())
            assert both and both != set(g[a].tolist()), "overlapping but different pixel sets"
    elif name == "shared_256":
        counts = [(7 * b + 3) % 5 for b in range(256)]
        counts[0], counts[255] = 0, 4
        g = []
        for b, c in enumerate(counts):
            base = (b // 16) * 2 * HW + (b % 16) * 2
            g.append(np.array([base, base + 1, base + HW, base + HW + 1][:c]))
        t = Table(name, g, 4, 1)
        assert t.B == 256 and t.nimg == 1 and set(counts) == {0, 1, 2, 3, 4} and t.tiles >= 2
    else:
        raise KeyError(name)
    return t


# name -> family of the case's sweep over forms and splits (each family on several tables; "257" runs all three)
CASE_FAMILY = {"one_row": "benign", "exact_256": "groupscale8", "257": "small", "corners_edges": "benign",
               "image_seam": "benign", "empty_groups": "groupscale8", "range_fallback": "small",
               "union_at_capacity": "groupscale8", "union_over_capacity": "benign", "shared_images": "small",
               "shared_256": "groupscale8"}
CAPACITY_CASES = ("union_at_capacity", "union_over_capacity")


# ------------------------------------------------------------------------------------------------ inputs
def group_exponents(seed):
    """e_g of the groupscale8 family: 16 channel groups, -8 .. 8, groups 7 and 8 the two extremes."""
    e = C._ints(-8, 8, CH // 16, seed)
    e[7], e[8] = 8, -8
    return e.float()


def make_inputs(t, family, seed=0):
    """(map (nimg, 64, 64, 256), w (256, 3, 3, 256) in K order (kh, kw, ci), bias (256)), fp32."""
    m = C.rnd(t.nimg, HW, HW, CH, seed=701 + seed)
    w = C.rnd(CH, 3, 3, CH, seed=702 + seed, scale=1.0 / np.sqrt(KK))
    bias = C.rnd(CH, seed=703 + seed)
    m = m * torch.tensor(t.image_scale, dtype=torch.float32).view(-1, 1, 1, 1)
    if t.border_bump:
        for s in (0, HW - 1):
            m[:, s, :, :] += t.border_bump
            m[:, 1:HW - 1, s, :] += t.border_bump
    if family == "groupscale8":
        s = torch.exp2(group_exponents(704 + seed)).repeat_interleave(16)
        m, w = m / s, w * s
    elif family == "small":
        assert max(t.image_scale) == 1.0 and not t.border_bump
        m = m * 2.0 ** -5
        assert float(m.abs().max()) < E.SUB_LIMIT
    else:
        assert family == "benign"
    return m.contiguous(), w.contiguous(), bias


def gather_rows(m, keys, fault=None):
    """(M, 2304) im2col rows of ``keys`` from the map, K order (kh, kw, ci), zeros where a tap leaves the map. Faults
    (test_vproj_tables.py): "seam" takes a tap above / below the image from the neighbouring image (only the flat key
    range is checked), "left_edge" takes the tap left of column 0 from the previous map row."""
    keys = np.asarray(keys, np.int64)
    nb = neighbours(keys)
    if fault in ("seam", "left_edge"):
        n, p = keys // PIX, keys % PIX
        y, x = p // HW, p % HW
        yy = y[:, None] + np.repeat([-1, 0, 1], 3)[None]
        xx = x[:, None] + np.tile([-1, 0, 1], 3)[None]
        flat = keys[:, None] + (yy - y[:, None]) * HW + (xx - x[:, None])
        inside = (flat >= 0) & (flat < m.shape[0] * PIX)
        if fault == "seam":
            leak = (nb < 0) & ((yy < 0) | (yy >= HW)) & (xx >= 0) & (xx < HW) & inside
        else:
            leak = (nb < 0) & (xx < 0) & (yy >= 0) & (yy < HW) & inside
        nb = np.where(leak, flat, nb)
    else:
        assert fault is None
    flat = m.reshape(-1, CH)
    a = torch.zeros(len(keys), TAPS, CH, dtype=m.dtype)
    ok = torch.from_numpy(nb >= 0)
    a[ok] = flat[torch.from_numpy(nb[nb >= 0])]
    return a.reshape(len(keys), KK)


class Case:
    """A table with one family's inputs, the float64 terms of its live rows and the measured rho."""

    def __init__(self, t, family, seed=0):
        self.table, self.family = t, family
        self.map, self.w, self.bias = make_inputs(t, family, seed)
        self.w2 = self.w.reshape(CH, KK)
        self.a = gather_rows(self.map, t.live)
        self.terms = E.terms(self.a, self.w2, self.bias)  # (ref before ReLU, D, T), float64, (live rows, 256)
        self.rho, self.rho_emul, self.rho_fp32 = E.measure_rho(self.a, self.w2, self.bias, t=self.terms)

    def ratio(self, rows):
        """Largest err / (rho D + T) over every element of the live rows ``rows`` (total, 256)."""
        return E.bound_ratio(rows, *self.terms, self.rho, relu=True)


@functools.lru_cache(maxsize=None)
def case(name, family=None, N=None):
    return Case(table(name, N), family or CASE_FAMILY[name])


# -------------------------------------------------------------------------------------------- comparison
def out_operand(t, device="cpu"):
    """``out`` (B * cap, 256) inside guards, every word the sentinel."""
    shape = (t.B * t.cap, CH)
    return guarded(shape, (CH, 1), SENTINEL, values=np.full(shape, SENT_F32, np.float32), device=device)


def live_rows(t, body):
    """The live rows of an ``out`` body in compacted order, after the placement checks: a row at or past its group's
    count keeps the sentinel in every word, a live row has lost it in every word."""
    body = body.detach().cpu().contiguous()
    assert tuple(body.shape) == (t.B * t.cap, CH)
    bits = body.view(torch.int32).numpy()
    live = np.zeros(t.B * t.cap, bool)
    live[t.live_idx] = True
    bad = np.flatnonzero((bits[~live] != SENT_BITS).any(1))
    assert len(bad) == 0, f"{len(bad)} row(s) past their group's count were written, first {np.flatnonzero(~live)[bad[:4]]}"
    kept = np.flatnonzero((bits[live] == SENT_BITS).any(1))
    assert len(kept) == 0, f"{len(kept)} live row(s) keep sentinel words, first (compacted) {kept[:4]}"
    return body[torch.from_numpy(t.live_idx)]


def check_output(c, body, what=""):
    """Placement, then every element of every live row under the bound; returns the worst ratio."""
    assert c.rho <= E.RHO_MAX, c.rho
    got = live_rows(c.table, body)
    ratio = c.ratio(got)
    assert ratio <= 1.0, f"{c.table.name} {c.family} {what}: worst err / (rho D + T) = {ratio:.3f} (rho {c.rho:.3e})"
    return ratio


# ------------------------------------------------------------------- the kernel restated (CPU, with faults)
def restated(c, fault=None, mutant=None):
    """The op on the CPU in the documented f16x3 arithmetic (f16x3_emul.py), stored into a guarded, sentinel-filled
    ``out`` as the kernels store. Faults: "seam", "left_edge" (gather_rows), "group_base" (group b's rows written at
    group b + 1's base), "group_twice" (channel group 1 summed twice). ``mutant``: one of f16x3_emul's."""
    t = c.table
    a = gather_rows(c.map, t.live, fault if fault in ("seam", "left_edge") else None)
    if fault == "group_twice":
        a = a.clone().view(-1, TAPS, CH)
        a[:, :, 16:32] *= 2.0
        a = a.view(-1, KK)
    y = E.linear_x3_emul(a, c.w2, c.bias, relu=True, mutant=mutant)
    out = out_operand(t)
    idx = t.live_idx + (t.cap if fault == "group_base" else 0)
    words = out.t.numpy()
    flat = words[out.offset:out.offset + (t.B * t.cap + t.cap) * CH].reshape(-1, CH)
    flat[idx] = y.numpy()
    return out
