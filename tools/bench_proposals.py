#!/usr/bin/env python3
"""PDM-Closed's proposal generation (dd_proposals) and the whole pdm_closed chain: device time beside the float64 numpy
restatement on the CPU.

    python tools/bench_proposals.py [--out FILE.json] [--scenes 64 1024] [--reps 20]

For every G (default 64 and 1024 scenes of 3 paths x 5 policies = 15 proposals): the scenes are
tests/pdm_proposal_ref.py's seeded scenes (a 24-vertex centerline with two lateral offsets, four tracks over 51 maps,
one red-light ring), eight distinct ones repeated, each on pdm_area_ref's seeded map. Packed once. Then the median of
``--reps`` warm calls, timed with HIP events around the Python call (output and scratch allocation included), of
``generate_proposals``, of the same with DDMI_PROPOSALS_CULL=0, and of the chain ``pdm_closed`` (generate + simulate +
pdm_score + select); and the wall time of the restatement's ``generate`` on this host's CPU over the eight distinct
scenes, scaled to G.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--scenes", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import pdm_area_ref as A
    import pdm_collision_ref as R
    import pdm_proposal_ref as Q
    from diffusiondrive_amd import simulate as S
    base = []
    for i in range(DISTINCT):
        s = Q.seeded_scene(100 + i, speed_limit=8.0 + i)
        s["tracks"] = [t for t in s["tracks"] if not t["token"].startswith("cut_")]
        s["items"] = A.seeded_map(100 + i, tuple(s["ego"][:3]), lanes=3)[0]
        base.append(s)
    t0 = time.perf_counter()
    for s in base:
        Q.generate(s["paths"], s["tracks"], s["rings"], s["ego"], s["targets"], collided=s["collided"])
    host_ms = (time.perf_counter() - t0) * 1e3 / DISTINCT
    rows = []
    for g in args.scenes:
        scenes = [base[i % DISTINCT] for i in range(g)]
        paths = S.pack_paths([[q["xyh"] for q in s["paths"]] for s in scenes], "cuda")
        items = [Q.lead_items(s) for s in scenes]
        objects = S.pack_lead_objects([i[0] for i in items], "cuda", stop_polygons=[i[1] for i in items],
                                      collided=[s["collided"] for s in scenes])
        ego = torch.from_numpy(np.stack([s["ego"] for s in scenes])).cuda()
        targets = torch.from_numpy(np.stack([s["targets"] for s in scenes])).cuda()
        maps = [s["items"] for s in scenes]
        packed = (S.pack_drivable_maps(maps, "cuda"), S.pack_drivable_maps(maps, "cuda", layers=("INTERSECTION",)))
        obs = S.pack_observations([R.track_items(s["tracks"]) for s in scenes], "cuda",
                                  collided=[s["collided"] for s in scenes])
        lines = S.pack_centerlines([s["paths"][0]["xyh"][:, :2] for s in scenes], "cuda")
        gen = timed(lambda: S.generate_proposals(paths, objects, ego, targets), args.reps)
        os.environ["DDMI_PROPOSALS_CULL"] = "0"
        try:
            uncut = timed(lambda: S.generate_proposals(paths, objects, ego, targets), args.reps)
        finally:
            del os.environ["DDMI_PROPOSALS_CULL"]
        chain = timed(lambda: S.pdm_closed(paths, objects, ego, targets, packed, obs, lines), args.reps)
        row = dict(scenes=g, proposals=g * 15, generate_ms=gen, generate_no_cull_ms=uncut, pdm_closed_ms=chain,
                   host_generate_ms=host_ms * g)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
