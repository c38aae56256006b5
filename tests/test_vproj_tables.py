"""tests/vproj_tables_util.py held to its purpose, on the CPU: the named row tables reach the union sizes, key ranges
and tile counts they are named for (the capacity pair at exactly N and N + 1 for several N), the float64 comparison
accepts the op restated in the documented f16x3 arithmetic and rejects one deliberate fault each - a neighbour taken
across the image seam, the out-of-map zero dropped at a left edge, group b's rows written at group b + 1's base, one
channel group summed twice, subnormal activation lo parts flushed - and the new entries are declared, bound and refuse
null or bad arguments by name before any device work. No device is needed and no kernel is run wrong on purpose."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import f16x3_emul as E
import vproj_tables_util as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dd_op_vproj_limits", "dd_op_vproj")
NAMES = ("one_row", "exact_256", "257", "corners_edges", "image_seam", "empty_groups", "range_fallback",
         "shared_images", "shared_256")


def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


# ------------------------------------------------------------------------------------------------ the entries
def test_entries_are_declared_bound_and_refuse_bad_arguments_by_name():
    from diffusiondrive_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddmi.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(lib, name)
        args = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1).split(",")
        res, argtypes = _lib._SIGS[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), (name, args)
        for a, t in zip(args, argtypes):
            first = a.split()[0]
            want = (ctypes.c_void_p if "*" in a and name == "dd_op_vproj" else
                    ctypes.POINTER(ctypes.c_int) if "*" in a else
                    ctypes.c_uint if first == "unsigned" else ctypes.c_int if first == "int" else None)
            assert want is not None and t is want, (name, a, t)
    names = [a.split()[-1].lstrip("*") for a in
             re.search(r"\bint dd_op_vproj\((.*?)\);", hdr, flags=re.S).group(1).split(",")]
    assert names == ["map", "wgt", "bias", "rows", "counts", "out", "B", "cap", "nimg", "union_stage", "usplit", "umax",
                     "ldh_pad", "part_fill", "flags", "rows2", "counts2", "out2", "fb_seen", "fb_after", "ucnt_after",
                     "stream"]
    assert lib.dd_op_vproj_limits(None, None) == -1
    assert b"dd_op_vproj_limits" in lib.dd_op_last_error() and b"null" in lib.dd_op_last_error()
    umax_rows, range_keys = V.limits()
    assert 256 < umax_rows < 2304 and range_keys % V.PIX == 0 and range_keys >= 2 * V.PIX

    host = (ctypes.c_float * 4)()  # never dereferenced: every call below is refused before any device work
    p = ctypes.addressof(host)
    good = dict(map=p, wgt=p, bias=p, rows=p, counts=p, out=p, B=1, cap=4, nimg=1, union_stage=1, usplit=1,
                umax=V.UMAX_OFF, ldh_pad=0, part_fill=0, flags=None, rows2=None, counts2=None, out2=None, fb_seen=None,
                fb_after=None, ucnt_after=None, stream=None)

    def refused(word, **change):
        a = dict(good, **change)
        assert lib.dd_op_vproj(*[a[n] for n in names]) == -1, change
        msg = lib.dd_op_last_error()
        assert b"dd_op_vproj" in msg and word in msg, msg

    for operand in ("map", "wgt", "bias", "rows", "counts", "out"):
        refused(b"null " + operand.encode(), **{operand: None})
    refused(b"B and cap", B=0)
    refused(b"B and cap", cap=0)
    refused(b"nimg", nimg=-1)
    refused(b"union_stage", union_stage=2)
    refused(b"ldh_pad", ldh_pad=4)
    refused(b"ldh_pad", ldh_pad=-8)
    refused(b"rows2, counts2 and out2", rows2=p)
    refused(b"rows2, counts2 and out2", rows2=p, counts2=p)


# ------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("name", NAMES)
def test_named_tables_hit_what_they_are_named_for(name):
    """Each builder asserts its own purpose (vproj_tables_util.table); here the numbers the kernel has to decide on,
    recomputed pixel by pixel without the vectorised helper, and the fallback each tile must take at the library's
    limits."""
    umax_rows, range_keys = V.limits()
    t = V.table(name)
    assert t.total == int(t.counts.sum()) and t.tiles == -(-t.total // 256)
    assert (t.rows.reshape(t.B, t.cap) >= 0).sum(1).tolist() == t.counts.tolist()
    for tile in range(t.tiles):
        keys = t.live[tile * 256:(tile + 1) * 256]
        union = set()
        for k in keys.tolist():
            n, y, x = k // 4096, (k % 4096) // 64, k % 64
            union |= {n * 4096 + yy * 64 + xx for yy in (y - 1, y, y + 1) for xx in (x - 1, x, x + 1)
                      if 0 <= yy < 64 and 0 <= xx < 64}
        assert t.union[tile] == len(union) and t.range[tile] == int(keys.max() - keys.min()) + 131
    fb = t.fallbacks(umax_rows, range_keys)
    if name == "range_fallback":
        assert fb == [None, "range"]
    elif name != "shared_256":
        assert fb == [None] * t.tiles, (fb, t.union, t.range)
    assert all(f is not None for f in t.fallbacks(umax_rows, range_keys, umax=0))
    u = t.union[0]
    assert t.fallbacks(umax_rows, range_keys, umax=u)[0] == fb[0]
    assert t.fallbacks(umax_rows, range_keys, umax=u - 1)[0] in ("union", "range")
    print(f"{name}: B {t.B} cap {t.cap} nimg {t.nimg} rows {t.total} tiles {t.tiles} union {t.union} range {t.range}")


@pytest.mark.parametrize("N", [330, 401, 512, 703, 704, 705, 1000])
def test_capacity_pair_lands_on_n_and_n_plus_one(N):
    at, over = V.table("union_at_capacity", N), V.table("union_over_capacity", N)
    assert at.union == [N] and over.union == [N + 1] and at.total == over.total == 256 and at.tiles == over.tiles == 1
    assert at.fallbacks(N, 3 * 4096) == [None] and over.fallbacks(N, 3 * 4096) == ["union"]
    assert at.range[0] <= 4096 + 131


def test_the_library_limit_is_reachable_by_the_capacity_pair():
    umax_rows, range_keys = V.limits()
    at, over = V.table("union_at_capacity", umax_rows), V.table("union_over_capacity", umax_rows)
    assert at.fallbacks(umax_rows, range_keys) == [None] and over.fallbacks(umax_rows, range_keys) == ["union"]


def test_a_permuted_table_keeps_every_group_and_moves_it_to_another_tile():
    t = V.table("shared_images")
    perm = [3, 0, 4, 1, 5, 2]
    q = t.permuted(perm)
    assert all(np.array_equal(q.groups[j], t.groups[p]) for j, p in enumerate(perm)) and q.total == t.total
    assert sorted(perm[g] for g in q.tile_groups(0)) != t.tile_groups(0), "other groups share tile 0 now"
    assert not np.array_equal(q.live[:256], t.live[:256])


# --------------------------------------------------------------------------------------------- the comparison
@pytest.mark.parametrize("family", V.FAMILIES)
def test_families_and_measured_rho(family):
    c = V.case("257", family)
    assert c.rho == 4.0 * max(c.rho_emul, c.rho_fp32) and 0 < c.rho <= E.RHO_MAX
    if family == "small":
        assert float(c.map.abs().max()) < E.SUB_LIMIT and float(c.terms[2].min()) > 0
    if family == "groupscale8":
        e = V.group_exponents(704)
        assert e.min() == -8 and e.max() == 8 and abs(float(e[7] - e[8])) == 16
        b = V.case("257", "benign")
        assert torch.equal(c.map * torch.exp2(e).repeat_interleave(16), b.map), "powers of two: the same function"
    print(f"257 {family}: rho {c.rho:.3e} (emulation {c.rho_emul:.2e}, fp32 {c.rho_fp32:.2e})")


@pytest.mark.parametrize("name", ["image_seam", "corners_edges", "empty_groups", "exact_256", "shared_images"])
def test_comparison_accepts_the_documented_arithmetic(name):
    c = V.case(name)
    out = V.restated(c)
    ratio = V.check_output(c, out.check())
    assert 0 < ratio <= 1.0
    print(f"{name} {c.family}: rho {c.rho:.3e} emulation's worst ratio {ratio:.3f}")


@pytest.mark.parametrize("name,fault", [("image_seam", "seam"), ("corners_edges", "seam"), ("corners_edges", "left_edge"),
                                        ("empty_groups", "group_base"), ("shared_images", "group_base"),
                                        ("exact_256", "group_twice"), ("shared_images", "group_twice")])
def test_comparison_rejects_a_geometry_fault(name, fault):
    c = V.case(name)
    out = V.restated(c, fault)
    if fault == "group_base":  # a live last group lands in the back guard; by placement alone it is refused too
        if c.table.counts[-1]:
            assert out.dirty()
            rejected(out.check)
        rejected(lambda: V.live_rows(c.table, out.view()))
    else:
        rejected(lambda: V.check_output(c, out.check()))
        got = V.live_rows(c.table, out.check())  # placement is right: the values are what is refused
        print(f"{name} with {fault}: worst ratio {c.ratio(got):.3e}")


def test_comparison_rejects_flushed_subnormal_lo_parts_on_small_activations():
    c = V.case("257", "small")
    V.check_output(c, V.restated(c).check())
    bad = V.restated(c, mutant="flush_act_lo").check()
    print(f"257 small with flush_act_lo: worst ratio {c.ratio(V.live_rows(c.table, bad)):.3f}")
    rejected(lambda: V.check_output(c, bad))


def test_placement_check_rejects_a_written_dead_row_and_an_unwritten_live_row():
    c = V.case("empty_groups")
    t = c.table
    out = V.restated(c)
    body = out.check()
    dead = body.clone()
    assert t.counts[2] < t.cap
    dead[t.cap * 2 + int(t.counts[2])] = 0.0  # the first row past group 2's count
    rejected(lambda: V.live_rows(t, dead))
    kept = body.clone()
    kept[int(t.live_idx[-1]), 255] = V.SENT_F32  # one word of the last live row never written
    rejected(lambda: V.live_rows(t, kept))
    nan = body.clone()
    nan[int(t.live_idx[0]), 0] = float("nan")
    rejected(lambda: V.check_output(c, nan))
