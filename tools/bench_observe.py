#!/usr/bin/env python3
"""PDM's forecasted observation (dd_observe): device time beside the host packers it replaces, and the whole chain.

    python tools/bench_observe.py [--out FILE.json] [--scenes 64 1024] [--reps 20]

For every G (default 64 and 1024 scenes x 135 detections: 55 vehicles, 28 pedestrians, 12 bicycles, 40 static objects
scattered 7 .. 95 m around the ego of tests/pdm_proposal_ref.py's seeded scenes, eight distinct ones repeated; all four
caps but the static one are passed, so 125 tracks are valid): the detections are packed once. Then
  observe_ms            the median of ``--reps`` warm ``observe`` calls, timed with HIP events around the Python call
                        (output and scratch allocation included)
  host_pack_ms          the wall time of ``pack_observations`` + ``pack_lead_objects`` over the same scenes' forecast
                        tracks in their list form (the restatement's boxes, built beforehand and not timed): the host
                        pass the device stage replaces, upload included
  collisions_ms         ``collisions`` alone over the chain's 15 proposals per scene against those tracks, for scale
  chain_device_ms       ``observe`` -> ``pdm_closed``, HIP events
  chain_host_ms         the host packers -> ``pdm_closed`` as before this stage existed: wall time, synchronised
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

DISTINCT = 8
COUNTS = dict(VEHICLE=55, PEDESTRIAN=28, BICYCLE=12, TRAFFIC_CONE=20, BARRIER=20)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--scenes", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import pdm_area_ref as A
    import pdm_observation_ref as O
    import pdm_proposal_ref as Q
    from diffusiondrive_amd import simulate as S
    base = []
    for i in range(DISTINCT):
        s = Q.seeded_scene(100 + i, speed_limit=8.0 + i)
        s["items"] = A.seeded_map(100 + i, tuple(s["ego"][:3]), lanes=3)[0]
        seen = O.seeded_scene(np.random.default_rng(500 + i), f"s{i}", tuple(s["ego"][:3]), COUNTS, far=0, ego_row=False)
        assert len(seen["dets"]) == 135
        s["dets"] = seen["dets"]
        ref = O.observe(seen["boxes"], seen["types"], s["ego"])
        tracks = []
        for k, d in enumerate(ref["order"]):   # every slot in the list form the host packers take
            mask = np.full(O.t_obs(), bool(ref["valid"][k]))
            agent, stopped = bool(ref["flags"][k] & O.FLAG_AGENT), bool(ref["flags"][k] & O.FLAG_STOPPED)
            tracks.append((seen["tokens"][d], (ref["boxes"][k], mask), float(ref["heading"][k]), agent, stopped,
                           float(ref["speed"][k])))
        s["lead_items"], s["obs_items"] = tracks, [t[:5] for t in tracks]
        base.append(s)
    rows = []
    for g in args.scenes:
        scenes = [base[i % DISTINCT] for i in range(g)]
        paths = S.pack_paths([[q["xyh"] for q in s["paths"]] for s in scenes], "cuda")
        ego = torch.from_numpy(np.stack([s["ego"] for s in scenes])).cuda()
        targets = torch.from_numpy(np.stack([s["targets"] for s in scenes])).cuda()
        maps = [s["items"] for s in scenes]
        packed = (S.pack_drivable_maps(maps, "cuda"), S.pack_drivable_maps(maps, "cuda", layers=("INTERSECTION",)))
        lines = S.pack_centerlines([s["paths"][0]["xyh"][:, :2] for s in scenes], "cuda")
        rings = [s["rings"] for s in scenes]
        det = S.pack_detections([s["dets"] for s in scenes], "cuda")
        obs_items, lead_items = [s["obs_items"] for s in scenes], [s["lead_items"] for s in scenes]

        def host_pack():
            return (S.pack_observations(obs_items, "cuda"),
                    S.pack_lead_objects(lead_items, "cuda", stop_polygons=rings))

        def chain_device():
            seen = S.observe(det, ego, stop_polygons=rings)
            return S.pdm_closed(paths, seen.lead_objects, ego, targets, packed, seen.observations, lines)

        def chain_host():
            obs, lead = host_pack()
            return S.pdm_closed(paths, lead, ego, targets, packed, obs, lines)

        reps = max(3, args.reps // 4) if g > 256 else args.reps   # the host pass takes seconds at 1024 scenes
        observe_ms = timed(lambda: S.observe(det, ego), args.reps)
        host_pack_ms = wall(host_pack, reps)
        obs, lead = host_pack()
        closed = S.pdm_closed(paths, lead, ego, targets, packed, obs, lines)
        areas = S.ego_areas(closed.states, packed[0]).areas
        collisions_ms = timed(lambda: S.collisions(closed.states, areas, obs, packed[1]), args.reps)
        row = dict(scenes=g, detections=g * 135, observe_ms=observe_ms, host_pack_ms=host_pack_ms,
                   collisions_ms=collisions_ms, chain_device_ms=timed(chain_device, args.reps),
                   chain_host_ms=wall(chain_host, reps))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
