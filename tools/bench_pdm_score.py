#!/usr/bin/env python3
"""The rest of the PDM score (dd_collisions, dd_progress, dd_pdm_aggregate): device time of each call and of the whole
pdm_score chain, with and without the collision cull, beside the float64 numpy restatement on the CPU.

    python tools/bench_pdm_score.py [--out FILE.json] [--candidates 1280 40960] [--reps 20]

For every N (default 64 x 20 and 64 x 32 x 20): the states come from ``simulate_trajectories`` on the seeded plans of
tools/bench_simulate.py, 20 candidates per scene; every scene gets tools/bench_ego_areas.py's map of 200 polygons
plus one INTERSECTION polygon, a seeded 64 tracks (``seeded_traffic``: vehicles driving along and across the plans'
fan, parked ones, a few static objects; 51 occupancy maps) and a 40-vertex centerline, each packed once and stored
again per scene. Then the median of ``--reps`` warm calls, timed with HIP events around the Python call (output and
scratch allocation included), of ``collisions``, ``progress``, ``aggregate``, the chain ``pdm_score`` (comfort +
ego_areas + collisions + progress + aggregate), and the chain with DDMI_COLLISIONS_CULL=0; and the wall time of
``tests/pdm_collision_ref.py:pdm_score`` on this host's CPU over the first ``--cpu-candidates`` candidates of scene 0,
scaled. Printed with each row: the discrete results that differ from the restatement's on those candidates.

A measurement needs the GPU: without one this fails.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

TRACKS = 64


def seeded_traffic(seed=0, count=TRACKS):
    """``count`` tracks over 51 maps around the origin, where the plans fan out along +x: a third drive along x, a
    sixth across it, a third are parked, the rest are static objects that are no agents."""
    import pdm_collision_ref as R
    rng = np.random.default_rng(seed)
    t = np.arange(R.T_OBS) * 0.1
    tracks = []
    for i in range(count):
        kind = i % 6
        x0, y0 = rng.uniform(-10.0, 70.0), rng.uniform(-14.0, 14.0)
        if kind in (0, 1):
            v = rng.uniform(2.0, 12.0)
            tracks.append(R.track(f"along_{i}", x0 + v * t, y0, 0.0, 4.6, 1.9, "VEHICLE", v))
        elif kind == 2:
            v = rng.uniform(1.0, 6.0)
            tracks.append(R.track(f"across_{i}", x0, y0 + v * t, np.pi / 2, 4.6, 1.9, "VEHICLE", v))
        elif kind in (3, 4):
            tracks.append(R.track(f"parked_{i}", x0, y0, rng.uniform(-0.2, 0.2), 4.4, 1.9, "VEHICLE", 0.0))
        else:
            tracks.append(R.track(f"cone_{i}", x0, y0, rng.uniform(-3, 3), 0.5, 0.5, "TRAFFIC_CONE", 0.0))
    return tracks


def tiled_observations(packed, scenes):
    from diffusiondrive_amd.simulate import PackedObservations
    k = packed.heading.numel()
    off = torch.arange(scenes + 1, device=packed.heading.device, dtype=torch.int32) * k
    return PackedObservations(packed.boxes.repeat(scenes, 1, 1, 1).contiguous(), packed.valid.repeat(scenes, 1).contiguous(),
                              packed.heading.repeat(scenes).contiguous(), packed.flags.repeat(scenes).contiguous(),
                              off.contiguous(), packed.tokens * scenes)


def tiled_centerlines(packed, scenes):
    from diffusiondrive_amd.simulate import PackedCenterlines
    v = packed.verts.shape[0]
    off = torch.arange(scenes + 1, device=packed.verts.device, dtype=torch.int32) * v
    return PackedCenterlines(packed.verts.repeat(scenes, 1).contiguous(), off.contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--candidates", type=int, nargs="+", default=[64 * 20, 64 * 32 * 20])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-candidates", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pdm_score.py measures on the GPU: torch.cuda.is_available() is False")
    import pdm_area_ref as A
    import pdm_collision_ref as R
    from bench_ego_areas import grid_map, tiled, timed
    from bench_simulate import plans
    from diffusiondrive_amd import simulate as S

    items = grid_map() + [([A.rect(30.03, -20.07, 60.01, 20.02)], "INTERSECTION", False)]
    tracks = seeded_traffic()
    line = R.seeded_centerline(0, vertices=40)
    one_map = S.pack_drivable_maps([items], "cuda")
    one_ix = S.pack_drivable_maps([items], "cuda", layers=("INTERSECTION",))
    one_obs = S.pack_observations([R.track_items(tracks)], "cuda")
    one_line = S.pack_centerlines([line], "cuda")
    rows = []
    for n in a.candidates:
        assert n % 20 == 0, "candidates come 20 per scene"
        b = n // 20
        ego = np.zeros((b, 11))
        ego[:, 3] = np.random.default_rng(3).uniform(0, 10, b)
        traj, ego_d = torch.from_numpy(plans(n)).cuda().view(b, 20, 8, 3), torch.from_numpy(ego).cuda()
        maps, ix = tiled(one_map, b), tiled(one_ix, b)
        obs, lines = tiled_observations(one_obs, b), tiled_centerlines(one_line, b)
        states = S.simulate_trajectories(traj, ego_d)
        areas = S.ego_areas(states, maps)
        comfort = S.comfort_metrics(states)
        col, col_ms = timed(lambda: S.collisions(states, areas.areas, obs, ix), a.reps)
        raw, progress_ms = timed(lambda: S.progress(states, lines), a.reps)
        dac, ddc = areas.drivable_area.contiguous(), areas.driving_direction.contiguous()
        _, aggregate_ms = timed(lambda: S.aggregate(col.no_collision, dac, ddc, raw, col.ttc, comfort), a.reps)
        res, chain_ms = timed(lambda: S.pdm_score(states, (maps, ix), obs, lines), a.reps)
        os.environ["DDMI_COLLISIONS_CULL"] = "0"
        try:
            uncut, nocull_ms = timed(lambda: S.pdm_score(states, (maps, ix), obs, lines), a.reps)
            _, col_nocull_ms = timed(lambda: S.collisions(states, areas.areas, obs, ix), a.reps)
        finally:
            del os.environ["DDMI_COLLISIONS_CULL"]
        for k in ("no_collision", "ttc", "collision_time_idx", "ttc_time_idx", "score"):
            assert torch.equal(getattr(res, k).view(torch.int64), getattr(uncut, k).view(torch.int64)), k
        k = min(20, a.cpu_candidates)
        host = states[0, :k].cpu().numpy()
        t0 = time.perf_counter()
        ref = R.pdm_score(host, items, tracks, line)
        cpu_s = time.perf_counter() - t0
        differ = sum(int((getattr(res, key)[0, :k].cpu().numpy() != ref[key]).sum())
                     for key in ("no_collision", "ttc", "collision_time_idx", "ttc_time_idx", "drivable_area"))
        row = dict(candidates=n, reps=a.reps, tracks_per_scene=len(tracks), collisions_ms=col_ms,
                   collisions_without_cull_ms=col_nocull_ms, progress_ms=progress_ms, aggregate_ms=aggregate_ms,
                   pdm_score_chain_ms=chain_ms, pdm_score_chain_without_cull_ms=nocull_ms,
                   cpu_restatement_candidates=k, cpu_restatement_s=cpu_s, cpu_restatement_s_scaled_to_all=cpu_s * n / k,
                   discrete_results_that_differ=differ, restatement_margins=dict(
                       gap=ref["gap_margin"], speed=ref["speed_margin"], angle=ref["angle_margin"]),
                   raw_progress_largest_difference=float(np.nanmax(np.abs(raw[0, :k].cpu().numpy() - ref["raw_progress"]))),
                   no_collision_mean=float(res.no_collision.mean()), ttc_mean=float(res.ttc.mean()),
                   score_mean=float(res.score.nanmean()), score_max=float(res.score.nan_to_num(0.0).max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
