"""The numpy restatement of the PDM comfort metrics (tests/pdm_comfort_ref.py) against goldens written by the
reference's own pdm_comfort_metrics module (tests/golden/make_comfort_golden.py), on the CPU.

Sets: the simulated states of the three pdm_sim_s3_* goldens, 96 synthetic state arrays that drive every flag both
ways, three rows with a non-finite sample (flags only), the synthetic set under non-default bounds with one zero
bound, and three rows whose heading steps by exactly 3 pi (a rounding tie of the unwrap). No candidate is excluded.

Bars: the inputs are the same bits on both sides, so a rounded signal can differ only where a pre-round value lands
on the other side of a rounding tie: at most one quantum (1e-8) for signals 0, 1, 4, 5, and (1 + L) quanta for the
jerk signals, which differentiate a series that may itself differ by a quantum per sample (L = the largest absolute
row sum of the derivative operator, 2.81 for delta = 0.1). Measured here: every value of every set is bit-equal.

The four quirk tests show that a textbook reading - the yaw window the caller asked for, a jerk pre-window equal to
the final window, np.unwrap, a bound of 0 taken as the number 0 - fails against the same goldens.
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import pdm_comfort_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIM_SETS = ("moving", "standing", "global")
SIGNAL_SETS = SIM_SETS + ("synth", "tie")
ONE_QUANTUM = R.QUANTUM * (1 + 1e-6)


def load():
    """The comfort golden, with the states of the three simulator goldens under states_{name}."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "pdm_comfort_s*.npz")))
    assert len(files) == 1, files
    with np.load(files[0]) as g:
        rec = {k: g[k] for k in g.files}
    for name in SIM_SETS:
        with np.load(os.path.join(GOLDEN, f"pdm_sim_s3_{name}.npz")) as g:
            rec[f"states_{name}"] = g["states"]
    rec["alt"] = R.params(**dict(zip(rec["alt_names"].tolist(), rec["alt_bounds"].tolist())))
    rec["path"] = files[0]
    return rec


@pytest.fixture(scope="module")
def golden():
    return load()


def signal_bars(ops):
    jerk, _ = R.jerk_bar(ops)
    return np.array([ONE_QUANTUM, ONE_QUANTUM, jerk, jerk, ONE_QUANTUM, ONE_QUANTUM])


def compare_signals(tag, got, ref, ops):
    """Print and return (largest difference per signal, share of values that are not equal per signal, bars)."""
    diff = np.abs(got - ref).max(axis=(0, 2))
    share = (got != ref).mean(axis=(0, 2))
    bars = signal_bars(ops)
    fmt = lambda v: "[" + " ".join(f"{x:.3e}" for x in v) + "]"  # noqa: E731
    print(f"comfort {tag}: largest signal difference {fmt(diff)} (bars {fmt(bars)}), not bit-equal share {fmt(share)}")
    return diff, share, bars


def test_golden_covers_what_it_should(golden):
    g = golden
    assert os.path.getsize(g["path"]) < 1 << 20
    assert g["states_synth"].shape == (96, R.T, 11) and g["signals_synth"].shape == (96, 6, R.T)
    fb = g["flags_synth"]
    assert fb.shape == (96, 6) and fb.any(0).all() and (~fb).any(0).all()   # every flag passes and fails
    assert float(g["margin"]) >= 1e-6
    for name in SIGNAL_SETS:
        assert R.margin(g[f"signals_{name}"]) >= 1e-6, name
    assert R.margin(g["signals_synth"], g["alt"]) >= 1e-6
    assert g["alt"]["min_lon_accel"] == 0.0 and all(g["alt"][k] != R.DEFAULTS[k] for k in g["alt"] if k != "dt")
    assert int(g["wrapped_rows"]) > 20
    for name in SIM_SETS:   # the simulator never writes ay
        assert (g[f"states_{name}"][..., R.AY] == 0).all()
    # the non-finite rows: NaN in ax, NaN in the heading, inf in ay
    c = g["states_nonfinite"]
    assert np.isnan(c[0, :, R.AX]).sum() == 1 and np.isnan(c[1, :, R.HEADING]).sum() == 1
    assert np.isinf(c[2, :, R.AY]).sum() == 1
    # the window-8 pre-smoothing reads samples i - 3 .. i + 4 (the first / last window at the edges), as recorded
    # from impulses through the reference's own function
    want = np.array([[min(max(i - 3, 0), 33), min(max(i - 3, 0), 33) + 7] for i in range(R.T)])
    assert np.array_equal(g["pre_support"], want)
    M = R.savgol_matrix(8, 2)
    assert all(np.array_equal(np.nonzero(M[i])[0][[0, -1]], want[i]) for i in range(R.T))


@pytest.mark.parametrize("name", SIGNAL_SETS)
def test_restatement_matches_the_reference(golden, name):
    g = golden
    flags, signals, d = R.comfort(g[f"states_{name}"])
    assert np.array_equal(flags, g[f"flags_{name}"])
    diff, share, bars = compare_signals(f"restatement vs reference [{name}]", signals, g[f"signals_{name}"], d["ops"])
    assert (diff <= bars).all()
    assert (share <= 1e-3).all()
    a8_diff = np.abs(d["a8"] - g[f"a8_{name}"]).max()
    print(f"comfort restatement [{name}]: pre-smoothed series differ by {a8_diff:.3e}")
    assert a8_diff <= ONE_QUANTUM


def test_restatement_flags_on_non_finite_rows_and_other_bounds(golden):
    g = golden
    flags, signals, _ = R.comfort(g["states_nonfinite"])
    assert np.array_equal(flags, g["flags_nonfinite"])
    # a non-finite sample reaches every output of a window-41 fit, and every later output of the yaw signals
    assert np.isnan(signals[0, 0]).all() and np.isnan(signals[1, 4, 28:]).all()
    flags, _, _ = R.comfort(g["states_synth"], g["alt"])
    assert np.array_equal(flags, g["flags_alt"])
    assert (flags != g["flags_synth"]).any(0).all()   # every bound of the other set matters


def test_operators():
    """Window 41 is one fit of the whole series: a quadratic is reproduced, its derivative exact; the even window is
    fitted half a sample off the grid (symmetric weights over i - 3 .. i + 4)."""
    t = np.arange(R.T) * 0.1
    y = 1.5 - 2.0 * t + 0.7 * t * t
    ops = R.operators(R.time_delta(0.1))
    np.testing.assert_allclose(ops["acc"] @ y, y, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ops["jerk"] @ y, -2.0 + 1.4 * t, rtol=0, atol=1e-11)
    late = t + np.where((np.arange(R.T) >= 4) & (np.arange(R.T) < 37), 0.05, 0.0)   # interior: half a sample late
    np.testing.assert_allclose(ops["pre"] @ y, 1.5 - 2.0 * late + 0.7 * late * late, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ops["yaw_rate"] @ y, -2.0 + 1.4 * t, rtol=0, atol=1e-11)
    np.testing.assert_allclose(ops["yaw_accel"] @ y, np.full(R.T, 1.4), rtol=0, atol=1e-10)
    w = ops["pre"][20, 17:25]
    np.testing.assert_allclose(w, w[::-1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(w, np.array([-3, 3, 7, 9, 9, 7, 3, -3]) / 32.0, rtol=0, atol=1e-15)
    assert R.time_delta(0.1) == 0.1


# ---- the quirks: each textbook reading fails against the goldens

def test_quirk_yaw_window_is_5_not_41(golden):
    g = golden
    flags, signals, _ = R.comfort(g["states_synth"], yaw_window=41)
    assert (flags[:, 4:] != g["flags_synth"][:, 4:]).any(0).all()
    assert np.abs(signals[:, 4:] - g["signals_synth"][:, 4:]).max() > 1e-2
    assert np.array_equal(signals[:, :4], g["signals_synth"][:, :4])


def test_quirk_jerk_presmoothing_window_is_8(golden):
    g = golden
    flags, signals, d = R.comfort(g["states_synth"], jerk_pre_window=41)
    assert (flags[:, 2:4] != g["flags_synth"][:, 2:4]).any(0).all()
    assert np.abs(signals[:, 2:4] - g["signals_synth"][:, 2:4]).max() > 1e-2
    # and a one-sample shift of the even window is orders of magnitude over the bar
    shifted = R.operators(d["delta"])["pre"]
    shifted[4:37] = np.roll(shifted[4:37], -1, axis=1)   # i - 4 .. i + 3
    a8 = R.round8(g["states_synth"][..., R.AX] @ shifted.T)
    jerk = R.round8(a8 @ d["ops"]["jerk"].T)
    assert np.abs(jerk - g["signals_synth"][:, 3]).max() > 1e3 * R.jerk_bar(d["ops"])[0]


def test_quirk_unwrap_rounds_ties_to_even(golden):
    """On headings in [-pi, pi) _phase_unwrap and np.unwrap agree to rounding; a step of exactly 3 pi is a tie (1.5
    turns) that the reference rounds to even - two turns - and np.unwrap to one."""
    g = golden
    h = g["states_tie"][..., R.HEADING]
    steps = np.diff(h, axis=-1) / (2.0 * np.pi)
    assert ((steps == 1.5).sum(-1) == 1).all()
    _, signals, _ = R.comfort(g["states_tie"], unwrap="np")
    assert np.abs(signals[:, 4:] - g["signals_tie"][:, 4:]).max() > 1.0
    # the wraps of the ordinary sets are unwrapped by both: 43 of the global set's candidates wrap
    wraps = (np.abs(np.diff(g["states_global"][..., R.HEADING], axis=-1)) > np.pi).any(-1)
    assert wraps.sum() == 43
    assert np.abs(np.diff(R.phase_unwrap(g["states_global"][..., R.HEADING]), axis=-1)).max() < 0.5


def test_quirk_zero_bound_is_no_bound(golden):
    g = golden
    flags, _, _ = R.comfort(g["states_synth"], g["alt"], zero_is_unbounded=False)
    assert (flags[:, 0] != g["flags_alt"][:, 0]).sum() > 10
    assert np.array_equal(flags[:, 1:], g["flags_alt"][:, 1:])


# ---- the C entry on a machine without a GPU

def test_defaults_and_rejections_need_no_device():
    """The defaults are the reference's, and every bad argument is refused before any device call (the pointers here
    are host addresses that a launch could not use; the sentinel-filled outputs stay untouched)."""
    from diffusiondrive_amd import _lib
    lib = _lib.load()
    p = _lib.DDComfortParams()
    lib.dd_default_comfort_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k, _ in p._fields_} == R.DEFAULTS
    buf = (ctypes.c_double * 16)(*([-7.0] * 16))
    ptr = ctypes.addressof(buf)
    for kw, text in rejection_cases():
        rc, msg = call_comfort(lib, ptr, ptr, ptr, **kw)
        assert rc == -1 and msg.startswith("dd_comfort: ") and text in msg, (kw, rc, msg)
    assert list(buf) == [-7.0] * 16


def comfort_params_with(lib, **kw):
    from diffusiondrive_amd import _lib
    q = _lib.DDComfortParams()
    lib.dd_default_comfort_params(ctypes.byref(q))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def call_comfort(lib, states, flags, signals, n=96, params="default", null=(), stream=None, **over):
    q = None if "params" in null else comfort_params_with(lib, **over)
    rc = lib.dd_comfort(None if "states" in null else states, n, ctypes.byref(q) if q is not None else None,
                        None if "out_flags" in null else flags, signals, stream)
    return rc, lib.dd_last_error().decode()


def rejection_cases():
    """(keyword arguments of call_comfort, text dd_last_error() must carry): every rejection dd_comfort documents."""
    nan, inf = float("nan"), float("inf")
    return [
        (dict(n=0), "N = 0"), (dict(n=-5), "N = -5"),
        (dict(null=("states",)), "states is null"), (dict(null=("params",)), "params is null"),
        (dict(null=("out_flags",)), "out_flags is null"),
        (dict(dt=0.0), "dd_comfort_params.dt"), (dict(dt=-0.1), "dd_comfort_params.dt"),
        (dict(dt=nan), "dd_comfort_params.dt"), (dict(dt=inf), "dd_comfort_params.dt"),
        (dict(min_lon_accel=nan), "dd_comfort_params.min_lon_accel is NaN"),
        (dict(max_lon_accel=nan), "dd_comfort_params.max_lon_accel is NaN"),
        (dict(max_abs_lat_accel=nan), "dd_comfort_params.max_abs_lat_accel is NaN"),
        (dict(max_abs_mag_jerk=nan), "dd_comfort_params.max_abs_mag_jerk is NaN"),
        (dict(max_abs_lon_jerk=nan), "dd_comfort_params.max_abs_lon_jerk is NaN"),
        (dict(max_abs_yaw_accel=nan), "dd_comfort_params.max_abs_yaw_accel is NaN"),
        (dict(max_abs_yaw_rate=nan), "dd_comfort_params.max_abs_yaw_rate is NaN"),
        (dict(min_lon_accel=2.4), "dd_comfort_params.min_lon_accel"),
        (dict(min_lon_accel=3.0, max_lon_accel=-1.0), "dd_comfort_params.min_lon_accel"),
        (dict(max_abs_lat_accel=-4.89), "dd_comfort_params.max_abs_lat_accel"),
        (dict(max_abs_mag_jerk=-1.0), "dd_comfort_params.max_abs_mag_jerk"),
        (dict(max_abs_lon_jerk=-1.0), "dd_comfort_params.max_abs_lon_jerk"),
        (dict(max_abs_yaw_accel=-1.0), "dd_comfort_params.max_abs_yaw_accel"),
        (dict(max_abs_yaw_rate=-inf), "dd_comfort_params.max_abs_yaw_rate"),
    ]
