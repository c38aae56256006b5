"""float64 numpy restatement of NAVSIM's PDM comfort metrics (the truth of dd_comfort).

Restates ``ego_is_comfortable`` (pdm_planner/scoring/pdm_comfort_metrics.py:313-336) over N candidates of (41, 11)
states, as the reference really computes it (numpy only: no scipy):

* ``savgol_filter(..., mode="interp")`` as a 41 x 41 operator: interior outputs are a convolution with the
  least-squares coefficients, the first and last ``window // 2`` outputs come from the polynomial fitted to the first
  and last ``window`` samples. The coefficients are rows of ``np.linalg.pinv`` of the Vandermonde matrix. An even
  window is fitted half a sample off the grid: output i reads samples i - w/2 + 1 .. i + w/2.
* the lon / lat acceleration use window 41 (one fit of the whole series);
* the jerk signals pre-smooth with window 8 (``_extract_ego_jerk`` calls ``_extract_ego_acceleration`` with its
  default, :98), round to 1e-8, then differentiate with window 41;
* the yaw signals use window 5 (``_extract_ego_yaw_rate`` never passes ``window_length`` on, :110-136);
* ``_phase_unwrap`` (:139-157): ``h - 2 pi cumsum(rint(diff(h) / 2 pi))``, not ``np.unwrap``;
* ``_within_bound`` (:204-220): a bound of exactly 0 is no bound (``min_bound if min_bound else -inf``);
* every signal goes through ``np.round(., 8)``.

The keyword arguments of ``comfort`` switch each quirk to its textbook form; tests/test_comfort.py shows that each
textbook form fails against goldens written by the reference itself (tests/golden/make_comfort_golden.py).
"""
import math

import numpy as np

T = 41
HEADING, AX, AY = 2, 5, 6
FLAGS = ("lon_accel", "lat_accel", "mag_jerk", "lon_jerk", "yaw_accel", "yaw_rate")
DEFAULTS = dict(dt=0.1, min_lon_accel=-4.05, max_lon_accel=2.40, max_abs_lat_accel=4.89, max_abs_mag_jerk=8.37,
                max_abs_lon_jerk=4.13, max_abs_yaw_accel=1.93, max_abs_yaw_rate=0.95)
QUANTUM = 1e-8


def params(**over):
    p = dict(DEFAULTS)
    for k in over:
        if k not in p:
            raise KeyError(k)
    p.update(over)
    return p


def bounds_of(p):
    """The six (lo, hi) pairs in flag order, as the reference passes them to ``_within_bound``."""
    return [(p["min_lon_accel"], p["max_lon_accel"]), (-p["max_abs_lat_accel"], p["max_abs_lat_accel"]),
            (-p["max_abs_mag_jerk"], p["max_abs_mag_jerk"]), (-p["max_abs_lon_jerk"], p["max_abs_lon_jerk"]),
            (-p["max_abs_yaw_accel"], p["max_abs_yaw_accel"]), (-p["max_abs_yaw_rate"], p["max_abs_yaw_rate"])]


def time_delta(dt, n=T):
    """``np.diff(t).mean()`` of ``t = arange(n) * dt``, as ``_approximate_derivatives`` forms it (:188-192)."""
    return float(np.diff(np.arange(n) * dt).mean())


def _deriv_row(x, order, deriv):
    """d^deriv/dx^deriv of (1, x, ..., x^order) at x."""
    return np.array([math.perm(k, deriv) * x ** (k - deriv) if k >= deriv else 0.0 for k in range(order + 1)])


def savgol_matrix(window, order, deriv=0, delta=1.0, n=T):
    """The n x n operator of ``savgol_filter(y, window, order, deriv, delta, mode="interp")``: out = M @ y."""
    assert order < window <= n
    half = window // 2
    scale = 1.0 / delta ** deriv
    M = np.zeros((n, n))
    # interior: the fit over the window centred at pos, its deriv-th derivative there
    pos = half if window % 2 else half - 0.5
    P = np.linalg.pinv((np.arange(window) - pos)[:, None] ** np.arange(order + 1)[None, :])  # (order + 1, window)
    coeffs = math.factorial(deriv) * scale * P[deriv]
    first = half if window % 2 else half - 1   # samples i - first .. i - first + window - 1 feed output i
    for i in range(half, n - half):
        M[i, i - first:i - first + window] = coeffs
    # edges: one fit of the first (last) `window` samples, evaluated at the first (last) `half` positions
    P = np.linalg.pinv(np.arange(window)[:, None].astype(np.float64) ** np.arange(order + 1)[None, :])
    for s in range(half):
        M[s, :window] = scale * (_deriv_row(float(s), order, deriv) @ P)
        M[n - half + s, n - window:] = scale * (_deriv_row(float(window - half + s), order, deriv) @ P)
    return M


def round8(v):
    """``np.round(v, 8)``: rint(v * 1e8) / 1e8, ties to even."""
    return np.rint(v * 1e8) / 1e8


def phase_unwrap(h):
    two_pi = 2.0 * np.pi
    adj = np.zeros_like(h)
    adj[..., 1:] = np.cumsum(np.rint(np.diff(h, axis=-1) / two_pi), axis=-1)
    return h - two_pi * adj


def within(v, lo, hi, zero_is_unbounded=True):
    if zero_is_unbounded:
        lo = lo if lo else -np.inf
        hi = hi if hi else np.inf
    return ((v > lo) & (v < hi)).all(axis=-1)


def operators(delta, yaw_window=5, jerk_pre_window=8):
    """The five 41 x 41 operators: acc (window 41), pre (window 8), jerk (window 41, d/dt), yaw_accel, yaw_rate."""
    return dict(acc=savgol_matrix(T, 2), pre=savgol_matrix(jerk_pre_window, 2),
                jerk=savgol_matrix(T, 2, 1, delta), yaw_accel=savgol_matrix(yaw_window, 3, 2, delta),
                yaw_rate=savgol_matrix(yaw_window, 2, 1, delta))


def comfort(states, p=None, yaw_window=5, jerk_pre_window=8, unwrap="reference", zero_is_unbounded=True):
    """(N, 41, 11) float64 states -> flags (N, 6) bool, signals (N, 6, 41), details (a8 = the two pre-smoothed series
    (N, 2, 41), ops = the operator matrices, delta). The defaults restate the reference; the keywords are the textbook
    variants the quirk tests hold against the goldens."""
    p = p or DEFAULTS
    states = np.asarray(states, np.float64)
    assert states.ndim == 3 and states.shape[1:] == (T, 11)
    delta = time_delta(p["dt"])
    ops = operators(delta, yaw_window, jerk_pre_window)
    ax, ay, h = states[..., AX], states[..., AY], states[..., HEADING]
    apply = lambda M, y: y @ M.T  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        a8 = np.stack([round8(apply(ops["pre"], np.hypot(ax, ay))), round8(apply(ops["pre"], ax))], axis=1)
        uw = phase_unwrap(h) if unwrap == "reference" else np.unwrap(h, axis=-1)
        signals = np.stack([
            round8(apply(ops["acc"], ax)), round8(apply(ops["acc"], ay)),
            round8(apply(ops["jerk"], a8[:, 0])), round8(apply(ops["jerk"], a8[:, 1])),
            round8(apply(ops["yaw_accel"], uw)), round8(apply(ops["yaw_rate"], uw))], axis=1)
        flags = np.stack([within(signals[:, k], lo, hi, zero_is_unbounded)
                          for k, (lo, hi) in enumerate(bounds_of(p))], axis=1)
    return flags, signals, dict(a8=a8, ops=ops, delta=delta)


def margin(signals, p=None):
    """Smallest distance of a finite signal sample to either of its (non-zero) bounds."""
    p = p or DEFAULTS
    worst = np.inf
    for k, (lo, hi) in enumerate(bounds_of(p)):
        v = signals[:, k]
        v = v[np.isfinite(v)]
        for b in (lo, hi):
            if b and np.isfinite(b) and v.size:
                worst = min(worst, float(np.abs(v - b).min()))
    return worst


def jerk_bar(ops):
    """Bar of signals 2 and 3 against the reference on identical inputs: their own rounding tie (one quantum) plus a
    quantum per sample of the pre-smoothed series through the derivative operator, whose gain is its largest absolute
    row sum L."""
    L = float(np.abs(ops["jerk"]).sum(axis=1).max())
    return (1.0 + L) * QUANTUM, L


def synthetic_states(seed, n=96):
    """Set (b): states that exercise every flag both ways (the simulator never writes ay, and its headings and
    accelerations are tame). Only columns 2, 5 and 6 are filled."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * 0.1
    half = np.arange(n) % 2 == 0
    ax = rng.uniform(-5.0, 3.0, (n, 1)) + rng.uniform(-6.0, 6.0, (n, 1)) * t + rng.normal(0.0, 0.05, (n, T))
    ay = rng.uniform(-6.0, 6.0, (n, 1)) + np.where(half[:, None], rng.uniform(-8.0, 8.0, (n, 1)), 0.0) * t \
        + rng.normal(0.0, 0.05, (n, T))
    alpha = np.where(half[::-1, None], rng.uniform(-2.5, 2.5, (n, 1)), 0.0)
    h = rng.uniform(-np.pi, np.pi, (n, 1)) + rng.uniform(-1.3, 1.3, (n, 1)) * t + 0.5 * alpha * t * t \
        + rng.normal(0.0, 0.002, (n, T))
    h = (h + np.pi) % (2.0 * np.pi) - np.pi
    s = np.zeros((n, T, 11))
    s[..., AX], s[..., AY], s[..., HEADING] = ax, ay, h
    return s
