#!/usr/bin/env python3
"""Golden vectors of the PDM comfort metrics, from the REFERENCE's pdm_comfort_metrics module run unmodified (build
container only: it needs the reference tree and scipy).

``ego_is_comfortable`` and the ``_extract_*`` functions behind it (pdm_planner/scoring/pdm_comfort_metrics.py) are
imported from the reference tree through the ``refshim`` stub finder; the module itself needs only numpy, scipy and
``pdm_enums``.

Inputs:
  (a) the ``states`` of the three committed tests/golden/pdm_sim_s3_*.npz sets (not stored again: keyed by name);
  (b) 96 synthetic state arrays (tests/pdm_comfort_ref.py:synthetic_states) - the simulator never writes ay and its
      headings are tame, so only these exercise flags 1, 2, 3 and 5 both ways;
  (c) three rows of (b) with a non-finite sample: NaN in ax, NaN in the heading, inf in ay (flags only). Each is run
      through the reference ON ITS OWN: np.polyfit hands all candidates of a call to one LAPACK lstsq, which scales
      the right-hand sides together, so an inf in one candidate turns every other candidate's edge fit to NaN too -
      an artefact of batching that a per-candidate kernel neither can nor should reproduce;
  (d) set (b) again under a non-default bound set with one zero bound (``min_lon_accel = 0``: no lower bound), got by
      assigning the module's constants at run time - the reference is not edited;
  (e) three rows of (b) whose heading steps by exactly 3 pi at one sample (not a principal value any more):
      ``_phase_unwrap`` rounds the tie 1.5 to even and takes two turns off, np.unwrap takes one. On headings in
      [-pi, pi) the two agree to rounding, so only these rows pin that the unwrap is the reference's own.

Recorded per set: the flags, the six rounded signals, the two pre-smoothed window-8 series (``a8``: magnitude, x);
and once: which samples feed each output of the window-8 pre-smoothing (impulses through the reference's own
``_extract_ego_acceleration``), the scipy version and the smallest margin.

The generator asserts that every flag both passes and fails somewhere in (b), that every finite sample of every
signal is at least 1e-6 from both of its bounds (sets a, b, d and e), and that only numbers are stored. A seed that
fails is replaced by the next one. No candidate is excluded.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_comfort_golden.py [seed]
Writes tests/golden/pdm_comfort_s{seed}.npz. Only data is stored; nothing of the reference's source.
"""
import glob
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import pdm_comfort_ref as R  # noqa: E402

SEED = 7
MARGIN = 1e-6
# set (d): every bound moved, one of them to exactly 0
ALT = dict(min_lon_accel=0.0, max_lon_accel=1.1, max_abs_lat_accel=3.3, max_abs_mag_jerk=5.5, max_abs_lon_jerk=2.2,
           max_abs_yaw_accel=0.77, max_abs_yaw_rate=1.2)
MODULE_NAMES = dict(min_lon_accel="min_lon_accel", max_lon_accel="max_lon_accel",
                    max_abs_lat_accel="max_abs_lat_accel", max_abs_mag_jerk="max_abs_mag_jerk",
                    max_abs_lon_jerk="max_abs_lon_jerk", max_abs_yaw_accel="max_abs_yaw_accel",
                    max_abs_yaw_rate="max_abs_yaw_rate")


def run_reference(C, states, t):
    """The reference's flags and the series they are taken from."""
    n = states.shape[1]
    with np.errstate(all="ignore"):
        flags = C.ego_is_comfortable(states, t)
        signals = np.stack([
            C._extract_ego_acceleration(states, acceleration_coordinate="x", window_length=n),
            C._extract_ego_acceleration(states, acceleration_coordinate="y", window_length=n),
            C._extract_ego_jerk(states, acceleration_coordinate="magnitude", time_steps_s=t, window_length=n),
            C._extract_ego_jerk(states, acceleration_coordinate="x", time_steps_s=t, window_length=n),
            C._extract_ego_yaw_rate(states, t, deriv_order=2, poly_order=3, window_length=n),
            C._extract_ego_yaw_rate(states, t, window_length=n)], axis=1)
        a8 = np.stack([C._extract_ego_acceleration(states, acceleration_coordinate="magnitude"),
                       C._extract_ego_acceleration(states, acceleration_coordinate="x")], axis=1)
    return flags, signals, a8


def non_finite_rows(states_b):
    c = states_b[:3].copy()
    c[0, 17, R.AX] = np.nan
    c[1, 30, R.HEADING] = np.nan
    c[2, 5, R.AY] = np.inf
    return c


def tie_rows(states_b):
    e = states_b[3:6].copy()
    two_pi = 2.0 * np.pi
    for i, at in enumerate((1, 20, 40)):
        h = e[i, :, R.HEADING]
        for step in (1.5 * two_pi, np.nextafter(1.5 * two_pi, 0.0), np.nextafter(1.5 * two_pi, 10.0)):
            h[at] = h[at - 1] + step   # this sample alone: the next step is a tie or near one downwards
            if (h[at] - h[at - 1]) / two_pi == 1.5:
                break
        assert (h[at] - h[at - 1]) / two_pi == 1.5
    return e


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    import refshim
    refshim.install_stub_finder()
    sys.path.insert(0, REF)
    import scipy
    from navsim.planning.simulation.planner.pdm_planner.scoring import pdm_comfort_metrics as C

    t = np.arange(R.T) * 0.1
    sims = {}
    for f in sorted(glob.glob(os.path.join(HERE, "pdm_sim_s3_*.npz"))):
        with np.load(f) as g:
            sims[os.path.basename(f)[:-4].split("_")[-1]] = g["states"]
    assert sorted(sims) == ["global", "moving", "standing"]

    # which samples feed output i of the window-8 pre-smoothing: impulses through the reference's own function
    imp = np.zeros((R.T, R.T, 11))
    imp[np.arange(R.T), np.arange(R.T), R.AX] = 1.0
    resp = C._extract_ego_acceleration(imp, acceleration_coordinate="x")     # [impulse at j, output i]
    support = np.stack([[np.nonzero(resp[:, i])[0].min(), np.nonzero(resp[:, i])[0].max()] for i in range(R.T)])

    defaults = {k: getattr(C, v) for k, v in MODULE_NAMES.items()}
    assert defaults == {k: R.DEFAULTS[k] for k in defaults}
    while True:
        rec = dict(seed=np.array(seed), scipy_version=np.array(scipy.__version__), pre_support=support,
                   alt_bounds=np.array([ALT[k] for k in MODULE_NAMES]), alt_names=np.array(list(MODULE_NAMES)))
        worst = np.inf
        for name, states in sims.items():
            flags, signals, a8 = run_reference(C, states, t)
            worst = min(worst, R.margin(signals))
            rec.update({f"flags_{name}": flags, f"signals_{name}": signals, f"a8_{name}": a8})
        states_b = R.synthetic_states(seed)
        flags_b, signals_b, a8_b = run_reference(C, states_b, t)
        worst = min(worst, R.margin(signals_b))
        both = bool((flags_b.any(0) & (~flags_b).any(0)).all())
        states_c = non_finite_rows(states_b)
        flags_c = np.concatenate([run_reference(C, states_c[i:i + 1], t)[0] for i in range(len(states_c))])
        states_e = tie_rows(states_b)
        flags_e, signals_e, a8_e = run_reference(C, states_e, t)
        worst = min(worst, R.margin(signals_e))
        try:
            for k, v in MODULE_NAMES.items():
                setattr(C, v, ALT[k])
            flags_d, signals_d, _ = run_reference(C, states_b, t)
        finally:
            for k, v in MODULE_NAMES.items():
                setattr(C, v, defaults[k])
        assert np.array_equal(signals_d, signals_b)   # the bounds touch the flags only
        worst = min(worst, R.margin(signals_b, R.params(**ALT)))
        wraps = int((np.abs(np.diff(states_b[..., R.HEADING], axis=-1)) > np.pi).any(-1).sum())
        if both and worst >= MARGIN:
            break
        print(f"seed {seed}: every flag both ways = {both}, smallest margin {worst:.3e} (< {MARGIN}?); next seed")
        seed += 1
    rec.update(seed=np.array(seed), states_synth=states_b, flags_synth=flags_b, signals_synth=signals_b,
               a8_synth=a8_b, states_nonfinite=states_c, flags_nonfinite=flags_c, flags_alt=flags_d,
               states_tie=states_e, flags_tie=flags_e, signals_tie=signals_e, a8_tie=a8_e,
               margin=np.array(worst), wrapped_rows=np.array(wraps))
    for k, v in rec.items():   # numbers, booleans and two short strings: nothing of the reference's program text
        assert v.dtype.kind in "fib" or (v.dtype.kind == "U" and v.size <= 8 and max(map(len, v.ravel())) < 32), k
    path = os.path.join(HERE, f"pdm_comfort_s{seed}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path}: {size} bytes, scipy {scipy.__version__}, margin {worst:.3e}, rows with a wrap {wraps}, "
          f"pass counts (b) {flags_b.sum(0).tolist()} (d) {flags_d.sum(0).tolist()} "
          f"non-finite flags {flags_c.astype(int).tolist()}")


if __name__ == "__main__":
    main()
