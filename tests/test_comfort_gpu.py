"""dd_comfort on the GPU against the reference's ego_is_comfortable.

The yardstick is the golden written by the reference's own pdm_comfort_metrics module
(tests/golden/make_comfort_golden.py) and, where the input exists only on the device (the chained cases), the numpy
restatement (tests/pdm_comfort_ref.py) that test_comfort.py holds to the same goldens bit for bit. No candidate is
excluded.

Bars (derived, not tuned; the inputs are the same bits on both sides). A device value may land on the other side of a
rounding tie, so signals 0, 1, 4, 5 may differ by at most one quantum: 1e-8 (1 + 1e-6). Signals 2 and 3 differentiate
a series that may itself differ by a quantum per sample: (1 + L) 1e-8, L = the largest absolute row sum of the
restatement's 41 x 41 derivative operator (2.81 at delta = 0.1). So that the allowance cannot hide a systematic
rounding error (truncation differs on half the values), the share of values that are not equal to the reference's is
at most 1e-3 per signal in every case. The flags must be equal: every finite golden sample is at least 1e-6 from its
bounds. Every case prints its measured figures before asserting.

Measured on an MI355X: no flag differs anywhere. Every signal value is bit-equal to the
reference's except one lon-jerk value of the standing set, one value of each jerk signal of the global set (the same
through the chained cases) and one value of the 120 planner candidates (whose forward is not bit-stable from run to
run): each one quantum, a share of 2.5e-4 (1 of 3 936) and 2.0e-4 (1 of 4 920) of that signal's values. The three golden flips are sample 20 of a jerk
series, whose exact value lies 7e-9 of a quantum from a rounding tie.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import pdm_comfort_ref as R
from test_comfort import SIM_SETS, call_comfort, compare_signals, load, rejection_cases

pytestmark = pytest.mark.gpu

SHARE = 1e-3


@pytest.fixture(scope="module")
def golden():
    return load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_twice(states, params=None):
    """comfort_metrics with signals, twice: the two runs must be bit-equal (NaNs at the same places)."""
    from diffusiondrive_amd.simulate import comfort_metrics
    flags, signals = comfort_metrics(states, params, signals=True)
    flags2, signals2 = comfort_metrics(states, params, signals=True)
    only = comfort_metrics(states, params)
    torch.cuda.synchronize()
    assert flags.dtype == torch.bool and signals.dtype == torch.float64
    assert torch.equal(flags, flags2) and torch.equal(flags, only)
    assert torch.equal(signals.view(torch.int64), signals2.view(torch.int64))
    return flags.cpu().numpy(), signals.cpu().numpy()


def hold(tag, flags, signals, ref_flags, ref_signals, ops):
    wrong = int((flags != ref_flags).sum())
    print(f"comfort {tag}: {wrong} of {flags.size} flags differ; passing per flag {flags.sum(0).tolist()}")
    diff, share, bars = compare_signals(tag, signals, ref_signals, ops)
    assert wrong == 0
    assert (diff <= bars).all()
    assert (share <= SHARE).all()


@pytest.mark.parametrize("name", SIM_SETS + ("synth", "tie", "alt"))
def test_golden_sets_against_the_reference(gpu, golden, name):
    """Sets (a), (b), (d) at N = 96 and the three tie rows (e); each run twice."""
    g = golden
    key = "synth" if name == "alt" else name
    p = g["alt"] if name == "alt" else None
    ops = R.operators(R.time_delta(0.1))
    flags, signals = run_twice(dev(g[f"states_{key}"]), p)
    assert flags.shape == (len(g[f"states_{key}"]), 6) and signals.shape == flags.shape + (R.T,)
    hold(f"[{name}]", flags, signals, g[f"flags_{name}"], g[f"signals_{key}"], ops)


@pytest.mark.parametrize("n", [1, 5])
def test_spare_and_partial_workgroups(gpu, golden, n):
    """N = 1 (three spare wavefronts) and N = 5 (a full workgroup and a quarter): rows of (b), the outputs inside
    larger sentinel-filled buffers that must stay untouched past row N."""
    lib, g = gpu, golden
    rows = [7] if n == 1 else [0, 13, 40, 77, 95]
    states = dev(g["states_synth"][rows])
    flags = torch.full((n + 3, 6), 9, dtype=torch.uint8, device="cuda")
    signals = torch.full((n + 3, 6, R.T), -7.0, dtype=torch.float64, device="cuda")
    p = ctypes.byref(comfort_defaults(lib))
    rc = lib.dd_comfort(states.data_ptr(), n, p, flags.data_ptr(), signals.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.dd_last_error()
    assert bool((flags[n:] == 9).all()) and bool((signals[n:] == -7.0).all())
    hold(f"N={n}", flags[:n].cpu().numpy().astype(bool), signals[:n].cpu().numpy(), g["flags_synth"][rows],
         g["signals_synth"][rows], R.operators(R.time_delta(0.1)))


def comfort_defaults(lib):
    from diffusiondrive_amd import simulate as S
    return S.default_comfort_params(lib)


def test_non_finite_rows(gpu, golden):
    """Set (c): NaN in ax, NaN in the heading, inf in ay. The flags equal the reference's (each row run through the
    reference on its own); the signals are not compared, but a NaN must reach what the reference lets it reach."""
    g = golden
    flags, signals = run_twice(dev(g["states_nonfinite"]))
    print(f"comfort [non-finite]: flags {flags.astype(int).tolist()} reference "
          f"{g['flags_nonfinite'].astype(int).tolist()}; NaN samples per signal {np.isnan(signals).sum(-1).tolist()}")
    assert np.array_equal(flags, g["flags_nonfinite"])
    assert np.isnan(signals[0, [0, 2, 3]]).all()          # a window-41 fit spreads it over the series
    assert np.isnan(signals[1, 4:, 28:]).all() and np.isfinite(signals[1, 4:, :28]).all()   # the unwrap's cumsum
    assert not np.isfinite(signals[2, 1]).any()
    # among ordinary rows the non-finite ones change nothing: a candidate reads its own states only
    mixed = np.concatenate([g["states_synth"][:5], g["states_nonfinite"], g["states_synth"][5:9]])
    f2, s2 = run_twice(dev(mixed))
    assert np.array_equal(f2[5:8], flags)
    hold("[rows around the non-finite ones]", np.delete(f2, [5, 6, 7], 0), np.delete(s2, [5, 6, 7], 0),
         g["flags_synth"][:9], g["signals_synth"][:9], R.operators(R.time_delta(0.1)))


@pytest.mark.parametrize("name", SIM_SETS)
def test_chained_to_the_simulator_on_the_device(gpu, golden, name):
    """comfort_metrics(simulate_proposals(golden proposals)): the device's states are within 1e-11 of the golden's and
    the margins at least 1e-6, so the flags are the reference's on the golden states; the signals are held against the
    restatement on the device's own states."""
    from diffusiondrive_amd.simulate import simulate_proposals
    from test_simulate import load as load_sim
    g, sim = golden, load_sim(name)
    states = simulate_proposals(dev(sim["proposals"]), dev(sim["ego_states"]))
    flags, signals = run_twice(states)
    host = states.cpu().numpy()
    gap = np.abs(np.delete(host, R.HEADING, -1) - np.delete(sim["states"], R.HEADING, -1)).max()
    print(f"comfort chained [{name}]: device states within {gap:.3e} of the golden's")
    assert gap <= 1e-11
    ref_flags, ref_signals, d = R.comfort(host)
    hold(f"chained [{name}]", flags, signals, ref_flags, ref_signals, d["ops"])
    assert np.array_equal(flags, g[f"flags_{name}"])


def test_planner_samples_to_comfort(gpu, gpu_model):
    """forward_samples at B = 2, S = 3 -> simulate_trajectories -> comfort_metrics: (2, 3, 20, 6), read in place."""
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    from diffusiondrive_amd.simulate import comfort_metrics, simulate_trajectories
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(2, 31)
    feats = {k: dev(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}
    noise = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 20, 8, 2)).astype(np.float32)).cuda()
    poses = gpu_model.forward_samples(feats, 3, noise=noise, modes=True)["poses_reg"]
    ego = np.array([[0.0, 0.0, 0.0, 4.0, 0.0, 0.2, 0.0, 0.01, 0.0, 0.013, 0.0],
                    [664431.37, 3997675.12, np.pi - 0.05, 6.0, 0.0, -0.3, 0.0, -0.02, 0.01, -0.04, 0.0]])
    states = simulate_trajectories(poses, dev(ego))
    assert states.shape == (2, 3, 20, 41, 11)
    flags, signals = run_twice(states)
    assert flags.shape == (2, 3, 20, 6) and signals.shape == (2, 3, 20, 6, 41)
    ref_flags, ref_signals, d = R.comfort(states.cpu().numpy().reshape(120, 41, 11))
    print(f"comfort planner samples: smallest margin to a bound {R.margin(ref_signals):.3e}")
    hold("planner samples", flags.reshape(120, 6), signals.reshape(120, 6, 41), ref_flags, ref_signals, d["ops"])
    me = types.SimpleNamespace(_transfuser_model=gpu_model)
    via = DiffusionDriveAgent.comfort_metrics(me, states)
    assert torch.equal(via, comfort_metrics(states)) and torch.equal(via.cpu(), torch.from_numpy(flags))
    via_host = DiffusionDriveAgent.comfort_metrics(me, states.cpu())
    assert via_host.is_cuda and torch.equal(via_host, via)


def test_params_reach_the_kernel(gpu, golden):
    """A non-default dt and bound set (one bound 0, one infinite) against the restatement with the same set."""
    g = golden
    over = dict(dt=0.125, min_lon_accel=-2.0, max_lon_accel=0.0, max_abs_lat_accel=6.5, max_abs_mag_jerk=3.0,
                max_abs_lon_jerk=float("inf"), max_abs_yaw_accel=2.5, max_abs_yaw_rate=0.6)
    ref_flags, ref_signals, d = R.comfort(g["states_synth"], R.params(**over))
    worst = R.margin(ref_signals, R.params(**over))
    print(f"comfort non-default parameters: delta {d['delta']!r}, smallest margin {worst:.3e}")
    assert worst >= 1e-6
    flags, signals = run_twice(dev(g["states_synth"]), over)
    hold("non-default parameters", flags, signals, ref_flags, ref_signals, d["ops"])
    assert (flags != g["flags_synth"]).any(0).all()      # every flag moved against the default run
    assert ref_flags[:, 3].all()                         # the infinite bound


def test_rejections_launch_nothing(gpu, golden):
    """Every bad argument returns DD_ERR_INVALID with the argument or field named, and the outputs keep their
    sentinels; the Python surface raises ValueError."""
    from diffusiondrive_amd import simulate as S
    lib = gpu
    states = dev(golden["states_synth"])
    flags = torch.full((96, 6), 9, dtype=torch.uint8, device="cuda")
    signals = torch.full((96, 6, R.T), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for kw, text in rejection_cases():
        rc, msg = call_comfort(lib, states.data_ptr(), flags.data_ptr(), signals.data_ptr(), stream=st, **kw)
        assert rc == -1 and msg.startswith("dd_comfort: ") and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((flags == 9).all()) and bool((signals == -7.0).all())
    with pytest.raises(ValueError, match="dd_comfort_params.dt"):
        S.comfort_metrics(states, dict(dt=0.0))
    with pytest.raises(ValueError, match="max_abs_yaw_rate is NaN"):
        S.comfort_metrics(states, dict(max_abs_yaw_rate=float("nan")))
    with pytest.raises(ValueError, match="unknown comfort parameter"):
        S.comfort_metrics(states, dict(max_jerk=1.0))
    with pytest.raises(ValueError, match="float64"):
        S.comfort_metrics(states.float())
    with pytest.raises(ValueError, match="41, 11"):
        S.comfort_metrics(states[:, :40])
    with pytest.raises(ValueError, match="device tensor"):
        S.comfort_metrics(states.cpu())
    # what is documented as accepted is: a zero bound on either side, both zero, infinite bounds, signals = NULL
    for kw in (dict(min_lon_accel=0.0), dict(min_lon_accel=0.0, max_lon_accel=0.0), dict(max_abs_lat_accel=0.0),
               dict(min_lon_accel=-float("inf"), max_lon_accel=float("inf")),
               dict(min_lon_accel=1.0, max_lon_accel=0.0)):
        rc, msg = call_comfort(lib, states.data_ptr(), flags.data_ptr(), None, stream=st, **kw)
        assert rc == 0, (kw, msg)
    torch.cuda.synchronize()
    assert bool((signals == -7.0).all()) and bool((flags <= 1).all())
