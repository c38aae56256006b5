#!/usr/bin/env python3
"""S trajectory samples per scene: forward_samples against S calls of forward, on one MI355X.

    python tools/bench_samples.py [--out FILE.json] [--batches 64 1] [--samples 1 2 4 8 16]
                                  [--baseline-root DIR]

For every batch B and S: the median device-synchronised time of ``forward_samples(B, S)`` (f16x3, 2 truncated DDIM
steps, explicit noise resident in HBM, hipGraph replay) beside S calls of ``forward`` on the same handle, measured in
alternating rounds; the spread is the largest difference between the round medians of one quantity. The S = 1 row is
the same program as ``forward`` and must agree with it within that spread.

From the ``value_cnt_s*l*`` / ``value_taps_s*l*`` taps of the last head pass: the mean live tap rows per decoder
scene (what value_proj computes today, per sample) and the mean size of the union of a scene's S samples' tap pixels
(what one tap table per perception scene would compute instead: the saving that design is judged by).

``--baseline-root DIR``: a built checkout of another commit (its own diffusiondrive_amd/libddmi.so). Its ``forward``
is timed at B = 64 in a child process of this job, before and after this tree's rows, and the S = 4 row is compared
with 4 of its forwards: the only way to draw 4 samples per scene on that commit.

All inputs synthetic and seeded, weights seeded random. A measurement needs the GPU: without one this fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

Q, P = 20, 8
STEPS = 2
SL = [(s, l) for s in range(STEPS) for l in range(2)]


def _model(root):
    sys.path.insert(0, root)
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import seeded_state_dict, synthetic_inputs
    if not torch.cuda.is_available():
        raise SystemExit("bench_samples.py measures on the GPU: torch.cuda.is_available() is False")
    cfg = TransfuserConfig()
    return DiffusionDriveModel(cfg, state_dict=seeded_state_dict(cfg, 0), device=0, gemm="f16x3"), synthetic_inputs


def _inputs(synthetic_inputs, B, distinct=8):
    """B scenes from `distinct` seeded scenes (resident in HBM)."""
    inp = synthetic_inputs(min(B, distinct), 7)
    idx = np.arange(B) % min(B, distinct)
    feats = {k: torch.from_numpy(np.ascontiguousarray(inp[k][idx])).cuda()
             for k in ("camera_feature", "lidar_feature", "status_feature")}
    return feats


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def forward_only(root, B, reps, rounds):
    """Round medians (ms) of forward() at batch B on the tree at `root` (the child process of --baseline-root)."""
    m, synthetic_inputs = _model(root)
    feats = _inputs(synthetic_inputs, B)
    nz = torch.randn((B, Q, P, 2), generator=torch.Generator().manual_seed(3)).cuda()
    for _ in range(5):
        m.forward(feats, noise=nz, steps=STEPS)
    return [_median_ms(lambda: m.forward(feats, noise=nz, steps=STEPS), reps) for _ in range(rounds)]


def tap_stats(m, D, S):
    """(mean live tap rows per decoder scene, mean union of a scene's S samples' tap pixels) over the (step, layer)
    tables of the last head pass (D decoder scenes, S per scene)."""
    live, union = [], []
    cap = Q * P * 4
    for s, l in SL:
        cnt = m.tap(f"value_cnt_s{s}l{l}", (D,)).view(torch.int32).cpu().numpy()
        rows = m.tap(f"value_taps_s{s}l{l}", (D, cap)).view(torch.int32).cpu().numpy()
        live.append(cnt.mean())
        for b in range(D // S):
            px = set()
            for d in range(b * S, (b + 1) * S):
                r = rows[d, :cnt[d]]
                assert (r // 4096 == b).all(), "a tap row names another scene's image"
                px.update(r.tolist())
            union.append(len(px))
    return float(np.mean(live)), float(np.mean(union))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--forward-only", type=int, default=0, metavar="B",
                    help="(child of --baseline-root) print the round medians of forward() at batch B as JSON")
    ap.add_argument("--root", default=ROOT, help="(with --forward-only) the tree whose package is imported")
    a = ap.parse_args()
    if a.forward_only:
        print(json.dumps({"forward_ms_rounds": forward_only(a.root, a.forward_only, a.reps, a.rounds)}))
        return

    def baseline():
        if not a.baseline_root:
            return None
        # the baseline tree may predate this tool: this file's forward-only mode, importing the package from there
        cmd = [sys.executable, os.path.abspath(__file__), "--forward-only", "64", "--reps", str(a.reps), "--rounds",
               str(a.rounds), "--root", os.path.abspath(a.baseline_root)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(f"baseline child failed ({a.baseline_root}):\n{r.stdout}\n{r.stderr}", file=sys.stderr)
            return []
        return json.loads(r.stdout.strip().splitlines()[-1])["forward_ms_rounds"]

    res = {"gemm": "f16x3", "steps": STEPS, "reps": a.reps, "rounds": a.rounds, "rows": []}
    base = [baseline()]
    m, synthetic_inputs = _model(ROOT)
    for B in a.batches:
        feats = _inputs(synthetic_inputs, B)
        nz1 = torch.randn((B, Q, P, 2), generator=torch.Generator().manual_seed(3)).cuda()
        for _ in range(5):
            m.forward(feats, noise=nz1, steps=STEPS)
        for S in a.samples:
            nz = torch.randn((B, S, Q, P, 2), generator=torch.Generator().manual_seed(5)).cuda()
            nz[:, 0] = nz1
            for _ in range(3):
                m.forward_samples(feats, S, noise=nz, steps=STEPS)
            fs, fw = [], []
            for _ in range(a.rounds):  # alternate the two so a drift of the box shows in both
                fs.append(_median_ms(lambda: m.forward_samples(feats, S, noise=nz, steps=STEPS), a.reps))
                fw.append(_median_ms(lambda: [m.forward(feats, noise=nz1, steps=STEPS) for _ in range(S)], a.reps))
            # the head passes of the chunk (default chunk limit 128; B <= 128 is one scene chunk)
            per_max = max(1, 128 // S)
            passes = (B + per_max - 1) // per_max
            per = (B + passes - 1) // passes
            last = B - per * (passes - 1)
            m.forward_samples(feats, S, noise=nz, steps=STEPS)  # the taps are the last forward's
            live, union = tap_stats(m, last * S, S)
            row = {"B": B, "S": S, "forward_samples_ms": statistics.median(fs), "forward_x_S_ms": statistics.median(fw),
                   "spread_ms": max(max(fs) - min(fs), max(fw) - min(fw)), "head_passes": passes,
                   "live_rows_per_decoder_scene": live, "union_rows_per_scene": union}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    base.append(baseline())
    if a.baseline_root and base[0] + base[1]:
        rounds = base[0] + base[1]
        res["baseline_forward_b64_ms"] = statistics.median(rounds)
        res["baseline_spread_ms"] = max(rounds) - min(rounds)
        s4 = [r for r in res["rows"] if r["B"] == 64 and r["S"] == 4]
        if s4:
            res["s4_vs_4_baseline_forwards"] = {"forward_samples_ms": s4[0]["forward_samples_ms"],
                                                "four_baseline_forwards_ms": 4 * res["baseline_forward_b64_ms"],
                                                "faster": s4[0]["forward_samples_ms"] < 4 * res["baseline_forward_b64_ms"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
