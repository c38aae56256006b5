"""CPU premises of test_f16x3_bound_gpu.py: the documented f16x3 arithmetic (f16x3_emul.py) meets the per-element bound
on every case the GPU test runs, the bound notices kernels the max-norm bar of test_ops_gpu.close() lets through, rho
stays fp32-class, and the rescaled state dicts (rescale_util.py) keep the network's function while the emulated-f16x3
oracle stays inside half of every bar at the spread the GPU test uses.
"""
import numpy as np
import pytest
import torch

import batch_sweep_util as U
import f16x3_cases as C
import f16x3_emul as E
import rescale_util as R
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)

# Largest emulation error / bound per family, measured over every case below (fp32 and float64 accumulation): uniform and
# rowscale 0.27 (scaling a row by a power of two changes no rounding: the two read the same), chanscale6 0.25 on the
# multi-channel cases and 0.43 on the one-channel stem (its only channel carries the whole 2^-6), chanscale12 0.77 (the
# K = 64 1 x 1 convs with two million outputs; 0.54 elsewhere). The device shares the emulation's split roundings (the
# same conversions), so the rest of the bound is for its summation order; it measured 0.61 / 0.61 / 0.39 / 0.77.
# rowrange: on its normal rows a power of two changes no rounding (rowscale's errors), on its tiny and zero rows the
# output is the unit-scale bias, whose rho D alone is 2^80 times the row's whole product; but rho is the maximum over
# the normal rows only, fewer elements than rowscale's, so the ratio is not rowscale's. The emulation is asked for half
# of the bound - the other half is the device's summation order, which rho's factor 4 is for (measured: 0.17 - 0.30).
EMUL_RATIO = {"uniform": 0.3, "rowscale": 0.3, "chanscale6": 0.5, "chanscale12": 0.8, "rowrange": 0.5}

ALL_CASES = ([("conv", c[0], c[1]) for c in C.CONV_CASES if c[0] != "x6-small-grid"]      # the same tensors as ragged
             + [("stem", f"stem-nhwc4-{s}", (s[0], 4, s[1], s[2])) for s in C.STEM_NHWC]
             + [("stem", f"stem-nchw-{s}", s) for s in C.STEM_NCHW]
             + [("mk", f"mk-{s}", s) for s in C.MK_CASES])


def _case(kind, shape, family):
    if kind == "conv":
        return C.conv_case(shape, family)
    if kind == "stem":
        return C.stem_case(*shape, family)
    return C.mk_case(*shape, family)


# --------------------------------------------------------------------------- (a), (c): the emulation and rho
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("kind,name,shape", ALL_CASES, ids=[c[1] for c in ALL_CASES])
def test_emulation_meets_the_bound(kind, name, shape, family):
    """(a) the emulation (fp32 accumulation in k16 steps) is within the family's share of the bound on every element,
    after the pooling for the stem; with float64 accumulation (the split error alone) too; (c) rho <= 1e-6."""
    case = _case(kind, shape, family)
    assert case.rho <= E.RHO_MAX, (name, family, case.rho)
    assert 4 * max(case.rho_emul, case.rho_fp32) == case.rho
    if family == "rowrange":
        # the flush allowance hides nothing on the normal rows: a millionth of their smallest bound at the most
        assert 0 < case.floor <= 1e-6 * case.normal_limit_min(), (name, case.floor, case.normal_limit_min())
        assert case.tiny.any() and case.normal.any()
    else:
        assert case.floor == 0.0 and case.tiny is None
    ratio = case.ratio(case.emul())
    split_only = case.ratio(case.emul(acc=torch.float64))
    print(f"{name} {family}: rho {case.rho:.3e} (emulation {case.rho_emul:.2e}, fp32 {case.rho_fp32:.2e}) "
          f"emulation / bound {ratio:.3f}, float64 accumulation {split_only:.3f}")
    assert ratio <= EMUL_RATIO[family], (name, family, ratio)
    assert split_only <= EMUL_RATIO[family], (name, family, split_only)
    if kind == "stem":
        assert case.pooled_ratio(case.emul_pooled()) <= ratio + 1e-12   # the max never widens a window's error


def test_row_exponents_isolate_the_tile_ends():
    """rowscale: exponents in -20 .. 10, the last channel and every 32-column tile's last channel at least 8 away from
    both neighbours, and the draw is spread (small channels exist next to large ones)."""
    for N in (24, 36, 40, 64, 128, 192, 200, 256):
        e = C.row_exponents(N, 215).numpy()
        assert e.min() >= -20 and e.max() <= 10
        for n in sorted({N - 1} | set(range(31, N, 32))):
            for m in (n - 1, n + 1):
                if 0 <= m < N:
                    assert abs(e[n] - e[m]) >= 8, (N, n, m)
        assert e.max() - e.min() >= 16, N


# --------------------------------------------------------------------------- (b): what the metric notices
def _mutant(case, mutant):
    out = case.emul(mutant=mutant)
    return case.ratio(out), E.old_bar_ok(out, case.truth())


MUTANT_CASES = [("conv", "x6-8x32-res", C.CONV_CASES[2][1]), ("conv", "x3-ksplit", C.CONV_CASES[5][1]),
                ("mk", "mk-1024", (1024, 256))]


@pytest.mark.parametrize("kind,name,shape", MUTANT_CASES, ids=[c[1] for c in MUTANT_CASES])
def test_bound_notices_a_lost_lo_product_in_the_last_k_chunk(kind, name, shape):
    """Mutant 1, ah x wl left out of the last k16 step only: over the new bound on rowscale and chanscale6 (measured
    4.5 - 37 times), and inside the old 3e-5 * (1 + max|ref|) bar on both - the old metric cannot see it."""
    for family in ("rowscale", "chanscale6"):
        ratio, old = _mutant(_case(kind, shape, family), "drop_ahwl_last")
        print(f"{name} {family}: drop_ahwl_last {ratio:.1f} x bound, old bar {'passes' if old else 'fails'}")
        assert ratio > 1.0, (name, family, ratio)
        assert old, (name, family)


@pytest.mark.parametrize("kind,name,shape", MUTANT_CASES, ids=[c[1] for c in MUTANT_CASES])
def test_bound_notices_flushed_subnormal_lo_parts(kind, name, shape):
    """Mutant 2, activation lo parts flushed to zero when subnormal: over the new bound on rowscale (5.9 - 16 times; unit
    randn activations, a fifth of them below 2^-2) and on chanscale6 (23 - 38 times). It passes the old bar on rowscale,
    the only one of the two families the old tests' inputs resemble; on chanscale6, inputs no test fed before, it fails
    the old bar as well (a flushed lo part of 2^-14 meets a weight scaled up by 2^6)."""
    ratio, old = _mutant(_case(kind, shape, "rowscale"), "flush_act_lo")
    print(f"{name} rowscale: flush_act_lo {ratio:.1f} x bound, old bar {'passes' if old else 'fails'}")
    assert ratio > 1.0 and old, (name, ratio, old)
    ratio, old = _mutant(_case(kind, shape, "chanscale6"), "flush_act_lo")
    print(f"{name} chanscale6: flush_act_lo {ratio:.1f} x bound, old bar {'passes' if old else 'fails'}")
    assert ratio >= 8.0, (name, ratio)
    assert ratio > 4.0 * _mutant(_case(kind, shape, "chanscale6"), None)[0]


SINV_CASES = [("conv", "x3-tapwalk-s2", C.CONV_CASES[3][1]), ("conv", "x3-1x1-s2", C.CONV_CASES[8][1]),
              ("mk", "mk-256", (256, 256)), ("mk", "mk-1024", (1024, 256))]


@pytest.mark.parametrize("kind,name,shape", SINV_CASES, ids=[c[1] for c in SINV_CASES])
def test_bound_notices_a_neighbours_row_scale_on_the_last_column(kind, name, shape):
    """Mutant 3, the last column scaled back with column N - 2's 1 / s: invisible to both metrics on uniform inputs (the
    rows share an exponent), far over the new bound on rowscale (the last channel is at least 8 binades from its
    neighbour), and inside the old bar on these cases, where the last channel and its neighbour are both small against
    the largest channel. (On the rowscale cases whose neighbour is a large channel the old bar sees it too.)"""
    ratio, old = _mutant(_case(kind, shape, "uniform"), "sinv_neighbour")
    assert ratio <= 1.0 and old, (name, ratio, old)
    ratio, old = _mutant(_case(kind, shape, "rowscale"), "sinv_neighbour")
    print(f"{name} rowscale: sinv_neighbour {ratio:.3g} x bound, old bar {'passes' if old else 'fails'}")
    assert ratio > 100.0, (name, ratio)
    assert old, name


@pytest.mark.parametrize("kind,name,shape", MUTANT_CASES + SINV_CASES[:1], ids=[c[1] for c in MUTANT_CASES + SINV_CASES[:1]])
def test_bound_notices_a_missing_row_scale(kind, name, shape):
    """Mutant 4, weights split without the per-row scale: the lo parts of the small rows fall into fp16's subnormals
    (rows below 2^-14 lose the hi part as well). Over the new bound on rowscale by four orders of magnitude; the old
    bar, which follows the largest channel, passes it."""
    ratio, old = _mutant(_case(kind, shape, "rowscale"), "no_row_scale")
    print(f"{name} rowscale: no_row_scale {ratio:.3g} x bound, old bar {'passes' if old else 'fails'}")
    assert ratio > 100.0, (name, ratio)
    assert old, name


# --------------------------------------------------------------------------- the rescaled dicts
@pytest.fixture(scope="module")
def inputs():
    from diffusiondrive_amd.weights import synthetic_inputs
    return synthetic_inputs(2, 7)


@pytest.fixture(scope="module")
def truth0(seeded_sd, inputs):
    return U.oracle_run(seeded_sd, inputs)


def _worst(got, ref):
    e = U.errors({k: got[k] for k in ref}, ref)
    name = max(e, key=lambda k: e[k] / U.bar_of(k, BARS))
    return e, name, e[name] / U.bar_of(name, BARS)


def test_rescaled_sites_are_found(seeded_sd):
    """16 + 16 BasicBlocks (two ResNet-34 trunks), the GPT blocks' MLPs, 3 tf-decoder layers, 2 trajectory-decoder
    layers; every parameter the rescaling touches stays finite and nonzero where it was."""
    assert len(R.basic_blocks(seeded_sd)) == 32
    mlps = R.relu_mlps(seeded_sd)
    assert sum(up.endswith(".linear1") for up, _ in mlps) == 3 and sum(up.endswith(".ffn.0") for up, _ in mlps) == 2
    assert sum(up.endswith(".mlp.0") for up, _ in mlps) >= 4
    sd = R.rescaled(seeded_sd, 12)
    for k, v in sd.items():
        assert np.isfinite(v).all(), k
        assert np.array_equal(v == 0, np.asarray(seeded_sd[k]) == 0), k
    var = R.rescaled_var(seeded_sd)
    small = min(float(var[p + ".bn1.running_var"].min()) for p in R.basic_blocks(var))
    assert 0 < small < 2e-5, small          # BN's eps is most of var + eps on some channel


def test_rescaling_keeps_the_function_in_float64(seeded_sd, inputs, truth0):
    """The float64 oracle on rescaled(s) against the float64 oracle on the seeded dict: powers of two commute with every
    rounding, so the measured difference is exactly 0 in every output and tap, at every spread tried (asserted at
    rounding level, 1e-12 of each bar). The fp32 oracle on rescaled(SPREAD) is within half of every bar of it."""
    for s in (R.SPREAD, max(R.SPREADS)):
        e, name, frac = _worst(U.oracle_run(R.rescaled(seeded_sd, s), inputs), truth0)
        print(f"rescaled({s}) float64 vs seeded float64: worst {name} {e[name]:.3e}")
        assert frac <= 1e-12, (s, name, e[name])
    e, name, frac = _worst(U.oracle_run(R.rescaled(seeded_sd), inputs, dtype=np.float32), truth0)
    print(f"rescaled({R.SPREAD}) fp32 oracle vs float64: worst {name} {e[name]:.3e} = {frac:.2f} of its bar")
    assert frac <= 0.5, (name, e[name])


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_emulated_f16x3_oracle_stays_inside_half_of_every_bar(seeded_sd, inputs, variant):
    """The oracle with conv / linear in the documented f16x3 arithmetic, on each dict of the GPU test at SPREAD, B = 2,
    against the float64 oracle on the same dict: within half of every bar (waypoint L2, heading, reg / cls per (step,
    layer), agents, taps at 2e-5). Measured for ``rescaled``: 0.12 / 0.15 / 0.26 / 0.54 / 3.8 of the tightest bar
    (query_out) at spreads 4 / 6 / 8 / 10 / 12 - so SPREAD = 8; the fp32 oracle reads 0.13 at every spread."""
    sd = R.VARIANTS[variant](seeded_sd)
    ref = U.oracle_run(sd, inputs)
    with E.emulated_f16x3_oracle():
        em = U.oracle_run(sd, inputs, dtype=np.float32)
    e, name, frac = _worst(em, ref)
    print(f"{variant}({R.SPREAD}) emulated f16x3 vs float64: worst {name} {e[name]:.3e} = {frac:.2f} of its bar; "
          + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert frac <= 0.5, (variant, name, e[name])
    e32, name32, frac32 = _worst(U.oracle_run(sd, inputs, dtype=np.float32), ref)
    assert frac32 <= 0.5, (variant, name32, e32[name32])


def test_spread_is_the_largest_that_qualifies(seeded_sd, inputs):
    """One step up (the next of SPREADS) the emulated-f16x3 oracle is outside half of a bar: SPREAD is the largest."""
    nxt = R.SPREADS[R.SPREADS.index(R.SPREAD) + 1]
    sd = R.rescaled(seeded_sd, nxt)
    ref = U.oracle_run(sd, inputs)
    with E.emulated_f16x3_oracle():
        em = U.oracle_run(sd, inputs, dtype=np.float32)
    e, name, frac = _worst(em, ref)
    print(f"rescaled({nxt}) emulated f16x3 vs float64: worst {name} {e[name]:.3e} = {frac:.2f} of its bar")
    assert frac > 0.5, (nxt, name, frac)


def test_emulation_patch_restores_the_oracle():
    import oracle.model as om
    before = om.conv, om.linear, om.bn
    with E.emulated_f16x3_oracle():
        assert (om.conv, om.linear, om.bn) != before
    assert (om.conv, om.linear, om.bn) == before


def test_decoded_query_rows_are_well_conditioned_on_the_sweep_scenes(seeded_sd):
    """Premise of what test_f16x3_bound_gpu.test_forward_on_rescaled_dict found in tfdec_mk: on the five scenes of B = 33
    and the rescaled_var dict, camera and LiDAR inputs perturbed by 1e-6 relative (float64 oracle) move keyval by 7e-6
    absolute and no decoded query row by more than 1.9e-6 (measured; asserted at 1e-5) - a query row that was 2.7e-4 off
    was not the function amplifying a rounding error."""
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = {k: np.asarray(v) for k, v in synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED).items()}
    sd = R.rescaled_var(seeded_sd)
    ref = U.oracle_run(sd, inp, heads=False)
    rng = np.random.default_rng(0)
    moved = dict(inp)
    for k in ("camera_feature", "lidar_feature"):
        moved[k] = inp[k].astype(np.float64) * (1 + 1e-6 * rng.standard_normal(inp[k].shape))
    got = U.oracle_run(sd, moved, heads=False)
    rows = np.abs(got["query_out"] - ref["query_out"]).max(-1)
    print(f"keyval moves {np.abs(got['keyval'] - ref['keyval']).max():.2e}, query rows at most {rows.max():.2e}")
    assert np.abs(got["keyval"] - ref["keyval"]).max() > 1e-7    # the perturbation reaches the decoder
    assert rows.max() <= 1e-5, rows.max()
