#!/usr/bin/env python3
"""Candidate simulation (dd_simulate): device time of one call beside the float64 numpy restatement on the CPU.

    python tools/bench_simulate.py [--out FILE.json] [--candidates 1280 40960] [--reps 20] [--cpu-chunk 2560]

For every N (default 64 x 20, one plain forward's candidates at B = 64, and 64 x 32 x 20, a full forward_samples call):
the median of ``--reps`` warm calls of ``simulate_trajectories`` on a resident (N / 20, 20, 8, 3) float32 tensor, timed
with HIP events around the call's launch sequence (work and output allocation included, as a user pays them), and
the wall time of ``tests/pdm_sim_ref.py:simulate_trajectories`` on the same N poses on this host's CPU (run once, in
chunks of ``--cpu-chunk`` candidates so that its (N, 40, 40) temporaries stay small). The largest state difference
between the two over all N candidates is printed with each row: a speed that computes something else is not a speed.

Inputs are seeded kinematic plans (constant acceleration and yaw rate, 2 cm noise). A measurement needs the GPU:
without one this fails.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def plans(n, seed=11):
    """n seeded constant-acceleration, constant-yaw-rate plans at 0.5 s (ego frame), float32 (n, 8, 3)."""
    rng = np.random.default_rng(seed)
    t = (np.arange(1, 9) * 0.5)[None]
    v0, acc, yaw = rng.uniform(0, 12, (n, 1)), rng.uniform(-2, 1.5, (n, 1)), rng.uniform(-0.25, 0.25, (n, 1))
    tstop = np.where(acc < 0, v0 / np.maximum(-acc, 1e-9), np.inf)
    tt = np.minimum(t, tstop)
    s = v0 * tt + 0.5 * acc * tt * tt
    h = yaw * tt
    out = np.stack([s * np.cos(0.5 * h), s * np.sin(0.5 * h), h], -1)
    out[..., :2] += rng.normal(0, 0.02, out[..., :2].shape)
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--candidates", type=int, nargs="+", default=[64 * 20, 64 * 32 * 20])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-chunk", type=int, default=2560)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simulate.py measures on the GPU: torch.cuda.is_available() is False")
    import pdm_sim_ref as R
    from diffusiondrive_amd.simulate import simulate_trajectories

    rows = []
    for n in a.candidates:
        assert n % 20 == 0, "candidates come 20 per scene"
        b = n // 20
        poses = plans(n)
        ego = np.zeros((b, 11))
        ego[:, 3] = np.random.default_rng(3).uniform(0, 10, b)
        traj, ego_d = torch.from_numpy(poses).cuda().view(b, 20, 8, 3), torch.from_numpy(ego).cuda()
        for _ in range(3):
            out = simulate_trajectories(traj, ego_d)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = simulate_trajectories(traj, ego_d)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        chunk = max(a.cpu_chunk // 20, 1) * 20
        t0 = time.perf_counter()
        ref = np.concatenate([R.simulate_trajectories(poses[i:i + chunk], ego[i // 20:(i + chunk) // 20])
                              for i in range(0, n, chunk)])
        cpu_s = time.perf_counter() - t0
        err = R.state_error(out.view(n, 41, 11).cpu().numpy(), ref)
        row = dict(candidates=n, device_ms_median=statistics.median(ms), device_ms_min=min(ms), device_ms_max=max(ms),
                   reps=a.reps, cpu_restatement_s=cpu_s, cpu_chunk=chunk, largest_state_difference=err)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
