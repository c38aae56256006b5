#!/usr/bin/env python3
"""Map compliance (dd_ego_areas): device time of one call, with and without the bounding-box cull, alone and chained
to the simulation and the comfort metrics, beside the float64 numpy restatement on the CPU.

    python tools/bench_ego_areas.py [--out FILE.json] [--candidates 1280 40960] [--reps 20]

For every N (default 64 x 20, one plain forward's candidates at B = 64, and 64 x 32 x 20, a full forward_samples
call): the states come from ``simulate_trajectories`` on the seeded plans of tools/bench_simulate.py, 20 candidates
per scene; every scene gets the same seeded map of 200 polygons x 40 vertices (``grid_map``: 100 lane cells of 20 m x
5 m, the middle rows on route, over 100 roadblock cells shifted by half a cell, 100 m x 100 m around the start pose),
packed once. Then the median of ``--reps`` warm calls, timed with HIP events around the call (output and scratch
allocation included, as a user pays it), of ``ego_areas(states, maps)``, of the same with ``coords=True``, of the
same with DDMI_EGO_AREAS_CULL=0 (every wavefront tests every polygon), of ``simulate_trajectories`` alone and of the
chain simulate + comfort + ego_areas; and the wall time of ``tests/pdm_area_ref.py:ego_areas`` on this host's CPU over
the first ``--cpu-candidates`` candidates (the restatement tests every point against every edge). Printed with each
row: the flags and scores that differ from the restatement's on those candidates, and the edge tests per candidate
with and without the cull (an edge test = one edge against the five points of all 64 lanes of a wavefront), counted
on the host from the polygons' bounding boxes.

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


def cell(x0, y0, x1, y1, per_side=10):
    """A rectangle as a ring of 4 * per_side vertices."""
    s = np.arange(per_side) / per_side
    return np.concatenate([np.stack([x0 + (x1 - x0) * s, np.full(per_side, y0)], -1),
                           np.stack([np.full(per_side, x1), y0 + (y1 - y0) * s], -1),
                           np.stack([x1 - (x1 - x0) * s, np.full(per_side, y1)], -1),
                           np.stack([np.full(per_side, x0), y1 - (y1 - y0) * s], -1)])


def grid_map(seed=0):
    """200 polygons x 40 vertices: lane cells of 20 m x 5 m (rows within 7.5 m of the start pose on route) and
    roadblock cells shifted by half a cell, jittered by the seed so that no point sits on an edge."""
    j = np.random.default_rng(seed).uniform(0.01, 0.09, 2)
    items = []
    for r in range(20):
        for c in range(5):
            x0, y0 = -20.0 + 20.0 * c + j[0], -50.0 + 5.0 * r + j[1]
            items.append(([cell(x0, y0, x0 + 20.0, y0 + 5.0)], "LANE", abs(y0 + 2.5) < 7.5))
            items.append(([cell(x0 - 10.0, y0 - 2.5, x0 + 10.0, y0 + 2.5)], "ROADBLOCK", False))
    return items


def tiled(packed, scenes):
    """One packed scene repeated ``scenes`` times (the offsets shifted; the vertices are stored again per scene, as
    different scenes' maps would be)."""
    from diffusiondrive_amd.simulate import PackedDrivableMaps
    v, ro, pro, kind, spo = packed
    V, Rn, P = v.shape[0], ro.numel() - 1, kind.numel()
    k = torch.arange(scenes, device=v.device, dtype=torch.int32)
    ring_off = torch.cat([(ro[:-1][None] + k[:, None] * V).reshape(-1), ro[-1:] + (scenes - 1) * V])
    poly_ring_off = torch.cat([(pro[:-1][None] + k[:, None] * Rn).reshape(-1), pro[-1:] + (scenes - 1) * Rn])
    scene_poly_off = torch.arange(scenes + 1, device=v.device, dtype=torch.int32) * P
    return PackedDrivableMaps(v.repeat(scenes, 1).contiguous(), ring_off.to(torch.int32).contiguous(),
                              poly_ring_off.to(torch.int32).contiguous(), kind.repeat(scenes).contiguous(),
                              scene_poly_off.contiguous())


def edge_tests(items, coords):
    """Edges a wavefront tests per candidate: all of them without the cull; with it, those of the polygons whose
    closed bounding box holds at least one of the candidate's 205 points."""
    lo = np.stack([np.concatenate(it[0]).min(0) for it in items])
    hi = np.stack([np.concatenate(it[0]).max(0) for it in items])
    edges = np.array([sum(len(r) for r in it[0]) for it in items])
    pts = coords.reshape(coords.shape[0], -1, 1, 2)
    hit = ((pts >= lo) & (pts <= hi)).all(-1).any(1)      # (candidates, polygons)
    return float((hit * edges).sum(1).mean()), int(edges.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--candidates", type=int, nargs="+", default=[64 * 20, 64 * 32 * 20])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-candidates", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ego_areas.py measures on the GPU: torch.cuda.is_available() is False")
    import pdm_area_ref as R
    from bench_simulate import plans
    from diffusiondrive_amd.simulate import (comfort_metrics, ego_areas, pack_drivable_maps,
                                             simulate_trajectories)

    items = grid_map()
    one = pack_drivable_maps([items], "cuda")
    rows = []
    for n in a.candidates:
        assert n % 20 == 0, "candidates come 20 per scene"
        b = n // 20
        ego = np.zeros((b, 11))
        ego[:, 3] = np.random.default_rng(3).uniform(0, 10, b)
        traj, ego_d = torch.from_numpy(plans(n)).cuda().view(b, 20, 8, 3), torch.from_numpy(ego).cuda()
        maps = tiled(one, b)
        states, sim_ms = timed(lambda: simulate_trajectories(traj, ego_d), a.reps)
        res, areas_ms = timed(lambda: ego_areas(states, maps), a.reps)
        with_coords, coords_ms = timed(lambda: ego_areas(states, maps, coords=True), a.reps)
        os.environ["DDMI_EGO_AREAS_CULL"] = "0"
        try:
            uncut, nocull_ms = timed(lambda: ego_areas(states, maps), a.reps)
        finally:
            del os.environ["DDMI_EGO_AREAS_CULL"]

        def chain():
            s = simulate_trajectories(traj, ego_d)
            return comfort_metrics(s), ego_areas(s, maps)

        (_, chained), chain_ms = timed(chain, a.reps)
        for other in (with_coords, uncut, chained):
            assert torch.equal(res.areas, other.areas) and torch.equal(res.driving_direction, other.driving_direction)
        k = min(n, a.cpu_candidates)
        host = states.view(n, 41, 11)[:k].cpu().numpy()
        t0 = time.perf_counter()
        ref = R.ego_areas(host, items)
        cpu_s = time.perf_counter() - t0
        culled, total = edge_tests(items, ref["coords"])
        got_areas = res.areas.view(n, 41, 3)[:k].cpu().numpy()
        scores = np.stack([res.drivable_area.view(n)[:k].cpu().numpy(),
                           res.driving_direction.view(n)[:k].cpu().numpy()])
        row = dict(candidates=n, reps=a.reps, polygons_per_scene=len(items), edges_per_scene=total,
                   simulate_ms=sim_ms, ego_areas_ms=areas_ms, ego_areas_with_coords_ms=coords_ms,
                   ego_areas_without_cull_ms=nocull_ms, simulate_plus_comfort_plus_ego_areas_ms=chain_ms,
                   cpu_restatement_candidates=k, cpu_restatement_s=cpu_s,
                   cpu_restatement_s_scaled_to_all=cpu_s * n / k,
                   edge_tests_per_candidate_with_cull=culled, edge_tests_per_candidate_without_cull=total,
                   distance_to_an_edge_m=R.edge_distance(items, ref["coords"]),
                   flags_that_differ=int((got_areas != ref["areas"]).sum()),
                   scores_that_differ=int((scores != np.stack([ref["drivable_area"], ref["driving_direction"]])).sum()),
                   flags_set=res.areas.view(-1, 3).sum(0).tolist(),
                   drivable_area_mean=float(res.drivable_area.mean()),
                   driving_direction_mean=float(res.driving_direction.mean()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
