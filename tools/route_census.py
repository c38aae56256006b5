#!/usr/bin/env python3
"""Census of the routes the forward takes at every batch size (GPU only; a tool, not a test).

    timeout -k 10 900 python tools/route_census.py [--max-batch 129] [--out tests/golden/forward_routes.json]

On one handle in the default f16x3 mode, one profiled forward (heads and modes on) per B in 1 .. 129 with
$DDMI_LAUNCH_LOG set; each log is reduced to the sorted set of batch-independent route strings
(tests/batch_sweep_util.py route_string: kernel, N, K, k, s, HW and the configuration / groups / form the dispatcher
chose) and the sets are written as ranges of consecutive batches with an identical set. tests/test_batch_sweep.py
checks the file on the CPU; tests/test_batch_sweep_gpu.py holds every batch of its sweep to the file's entry.
Regenerate it after any change of a dispatcher ("Batch sweep").
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import batch_sweep_util as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-batch", type=int, default=U.MAX_BATCH)
    ap.add_argument("--out", default=U.ROUTES_PATH)
    a = ap.parse_args()
    log = tempfile.NamedTemporaryFile(prefix="ddmi_routes_", suffix=".tsv", delete=False).name
    os.environ["DDMI_LAUNCH_LOG"] = log
    import torch
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import seeded_state_dict, synthetic_inputs

    cfg = TransfuserConfig()
    model = DiffusionDriveModel(cfg, seeded_state_dict(cfg, 0), device=0, gemm="f16x3")
    scenes = synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED, cfg)
    dev = {k: torch.from_numpy(scenes[k]).cuda() for k in U.INPUT_KEYS}
    # a handle's first forward also computes the per-handle constants (the FiLM rows of the timesteps: one GEMM that
    # no later forward runs); that is no route of a batch, so one forward goes ahead of the census
    model.forward({k: dev[k][:1] for k in U.INPUT_KEYS[:3]}, noise=dev["noise"][:1], heads=True, modes=True)
    model.set_profiling(True)
    sets = {}
    try:
        for B in range(1, a.max_batch + 1):
            idx = torch.from_numpy(U.replica_index(B)).cuda()
            feats = {k: dev[k][idx].contiguous() for k in U.INPUT_KEYS[:3]}
            open(log, "w").close()
            model.forward(feats, noise=dev["noise"][idx].contiguous(), heads=True, modes=True)
            torch.cuda.synchronize()
            flags = model.numerics_flags()
            if flags:
                raise RuntimeError(f"numerics flag {flags:#x} at B={B}")
            sets[B] = U.route_set(U.read_launch_log(log))
            print(f"B={B}: {len(sets[B])} routes", flush=True)
    finally:
        model.set_profiling(False)
        os.unlink(log)
    ranges = U.ranges_of(sets)
    with open(a.out, "w") as f:
        json.dump(ranges, f, indent=0, ensure_ascii=True)
        f.write("\n")
    print(f"{len(ranges)} ranges -> {a.out}: " + ", ".join(
        f"{r['from']}" if r["from"] == r["to"] else f"{r['from']}..{r['to']}" for r in ranges))


if __name__ == "__main__":
    main()
