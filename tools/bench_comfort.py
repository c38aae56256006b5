#!/usr/bin/env python3
"""Comfort metrics (dd_comfort): device time of one call, alone and chained to the simulation, beside the float64
numpy restatement on the CPU.

    python tools/bench_comfort.py [--out FILE.json] [--candidates 1280 40960] [--reps 20]

For every N (default 64 x 20, one plain forward's candidates at B = 64, and 64 x 32 x 20, a full forward_samples call):
the states come from ``simulate_trajectories`` on the seeded plans of tools/bench_simulate.py; then the median of
``--reps`` warm calls, timed with HIP events around the call (output allocation included, as a user pays it), of
``comfort_metrics(states)``, of ``comfort_metrics(states, signals=True)`` and of the chain
``comfort_metrics(simulate_trajectories(poses))``; and the wall time of ``tests/pdm_comfort_ref.py:comfort`` on the
same states on this host's CPU (run once). The number of flags that differ from the restatement's and the share of
signal values that are not bit-equal are printed with each row: a speed that computes something else is not a speed.

A measurement needs the GPU: without one this fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--candidates", type=int, nargs="+", default=[64 * 20, 64 * 32 * 20])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_comfort.py measures on the GPU: torch.cuda.is_available() is False")
    import pdm_comfort_ref as R
    from bench_simulate import plans
    from diffusiondrive_amd.simulate import comfort_metrics, simulate_trajectories

    rows = []
    for n in a.candidates:
        assert n % 20 == 0, "candidates come 20 per scene"
        b = n // 20
        ego = np.zeros((b, 11))
        ego[:, 3] = np.random.default_rng(3).uniform(0, 10, b)
        traj, ego_d = torch.from_numpy(plans(n)).cuda().view(b, 20, 8, 3), torch.from_numpy(ego).cuda()
        states, sim_ms = timed(lambda: simulate_trajectories(traj, ego_d), a.reps)
        flags, flags_ms = timed(lambda: comfort_metrics(states), a.reps)
        (flags2, signals), signals_ms = timed(lambda: comfort_metrics(states, signals=True), a.reps)
        chained, chain_ms = timed(lambda: comfort_metrics(simulate_trajectories(traj, ego_d)), a.reps)
        assert torch.equal(flags, flags2) and torch.equal(flags, chained)
        host = states.view(n, 41, 11).cpu().numpy()
        t0 = time.perf_counter()
        ref_flags, ref_signals, _ = R.comfort(host)
        cpu_s = time.perf_counter() - t0
        got = signals.view(n, 6, 41).cpu().numpy()
        row = dict(candidates=n, reps=a.reps, simulate_ms=sim_ms, comfort_ms=flags_ms,
                   comfort_with_signals_ms=signals_ms, simulate_plus_comfort_ms=chain_ms, cpu_restatement_s=cpu_s,
                   flags_that_differ=int((flags.view(n, 6).cpu().numpy() != ref_flags).sum()),
                   passing_per_flag=ref_flags.sum(0).tolist(),
                   not_bit_equal_share=(got != ref_signals).mean(axis=(0, 2)).tolist(),
                   largest_signal_difference=np.abs(got - ref_signals).max(axis=(0, 2)).tolist())
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
