#!/usr/bin/env python3
"""uint8 camera / LiDAR features against the float features, resident and host-fed, on one MI355X.

    python tools/bench_u8_inputs.py [--out FILE.json] [--baseline-root DIR] [--batch 64] [--rounds 3] [--reps 15]

f16x3, 2 truncated DDIM steps, explicit noise. Three variants - ``base_f32`` (float features on the built checkout at
``--baseline-root``, its own diffusiondrive_amd/libddmi.so), ``f32`` (float features on this tree) and ``u8`` (uint8
features on this tree) - each measured in a child process of this job, the variants alternating round by round so a
drift of the box shows in all of them. Per variant and round, the median over ``--reps`` device-synchronised steps of

  (a) resident:   ``forward`` on features resident in HBM (hipGraph replay);
  (b) host_fed_1: pinned host memory -> device copy of the features and the noise, then ``forward``, one at a time;
      host_fed_3: the same with 3 lanes in flight (InFlightPlanner, one device buffer set per lane), as bench.py's
                  h2d_included leg stages it; ms per step = wall time of the run / steps.

The reported value of a quantity is the median of its round medians, its spread their largest difference. ``f32`` and
``base_f32`` must agree within the spread (the float path is unchanged). Bytes per step are the feature bytes copied.

(c) in this process, under dd_set_profiling: the stems' per-launch times and dd_kernel_bytes("stem_pool") for both
kinds, split by launch (the camera and the LiDAR stem have different byte counts).

All inputs synthetic and seeded (exactly byte-valued, so the uint8 form is lossless), weights seeded random. A
measurement needs the GPU: without one this fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

Q, P, STEPS = 20, 8, 2
KEYS = ("camera_feature", "lidar_feature", "status_feature")


def _setup(root, B, kind, distinct=8):
    """(model, host feature dict, host noise) of the tree at `root`; kind "u8" quantizes the features (this tree)."""
    sys.path.insert(0, root)
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import seeded_state_dict, synthetic_inputs
    if not torch.cuda.is_available():
        raise SystemExit("bench_u8_inputs.py measures on the GPU: torch.cuda.is_available() is False")
    cfg = TransfuserConfig()
    m = DiffusionDriveModel(cfg, state_dict=seeded_state_dict(cfg, 0), device=0, gemm="f16x3")
    inp = synthetic_inputs(min(B, distinct), 7)
    idx = np.arange(B) % min(B, distinct)
    host = {k: torch.from_numpy(np.ascontiguousarray(inp[k][idx])) for k in KEYS}
    if kind == "u8":
        from diffusiondrive_amd.features import quantize_features
        host = quantize_features(host, cfg)
    nz = torch.randn((B, Q, P, 2), generator=torch.Generator().manual_seed(3))
    return m, host, nz


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def child(root, B, kind, reps, lanes):
    """One variant's three legs, one median each (a child process: its own handle, streams and graphs)."""
    m, host, nz = _setup(root, B, kind)
    from diffusiondrive_amd.model import InFlightPlanner
    dev = {k: v.cuda() for k, v in host.items()}
    dnz = nz.cuda()
    for _ in range(5):
        m.forward(dev, noise=dnz, steps=STEPS)
    resident = _median_ms(lambda: m.forward(dev, noise=dnz, steps=STEPS), reps)

    pin = {k: v.pin_memory() for k, v in host.items()}
    pnz = nz.pin_memory()

    def fed(model, dbuf, dz, stream=None):
        for k in KEYS:
            dbuf[k].copy_(pin[k], non_blocking=True)
        dz.copy_(pnz, non_blocking=True)
        return model.forward(dbuf, noise=dz, steps=STEPS, stream=stream)["trajectory"]

    d1 = ({k: torch.empty_like(v, device="cuda") for k, v in host.items()}, torch.empty_like(nz, device="cuda"))
    for _ in range(3):
        fed(m, *d1)
    fed1 = _median_ms(lambda: fed(m, *d1), reps)

    models = [m] + [m.clone() for _ in range(lanes - 1)]
    pl = InFlightPlanner(models=models)
    dbufs = [({k: torch.empty_like(v, device="cuda") for k, v in host.items()}, torch.empty_like(nz, device="cuda"))
             for _ in range(lanes)]
    it = [0]

    def step():
        dbuf, dz = dbufs[it[0] % lanes]
        it[0] += 1
        with pl.next_lane() as lm:
            return fed(lm, dbuf, dz, torch.cuda.current_stream(0))

    for _ in range(2 * lanes):
        step()
    pl.synchronize()
    n = max(reps, 2 * lanes) * 2
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    pl.synchronize()
    torch.cuda.synchronize()
    fedn = (time.perf_counter() - t0) * 1e3 / n
    for c in models[1:]:
        c.close()
    nbytes = int(sum(v.numel() * v.element_size() for v in host.values()) + nz.numel() * 4)
    return {"resident_ms": resident, "host_fed_1_ms": fed1, f"host_fed_{lanes}_ms": fedn, "bytes_per_step": nbytes}


def stems(B):
    """(c): per-launch stem times and byte model of both kinds on this tree, under dd_set_profiling."""
    out = {}
    for kind in ("f32", "u8"):
        m, host, nz = _setup(ROOT, B, kind)
        dev = {k: v.cuda() for k, v in host.items()}
        dnz = nz.cuda()
        for _ in range(3):
            m.forward(dev, noise=dnz, steps=STEPS)
        with tempfile.TemporaryDirectory() as td:
            log = os.path.join(td, "launch.tsv")
            os.environ["DDMI_LAUNCH_LOG"] = log
            m.set_profiling(True)
            m.forward(dev, noise=dnz, steps=STEPS)  # warm the eager path
            torch.cuda.synchronize()
            open(log, "w").close()
            m.reset_stats()
            n = 10
            for _ in range(n):
                m.forward(dev, noise=dnz, steps=STEPS)
            torch.cuda.synchronize()
            st = m.kernel_stats("stem_pool")
            m.set_profiling(False)
            del os.environ["DDMI_LAUNCH_LOG"]
            per = {}
            for line in open(log):
                f = line.rstrip("\n").split("\t")
                if f[0] == "stem_pool":
                    per.setdefault(float(f[4]), []).append(float(f[3]))
        out[kind] = {"stem_pool_bytes_per_forward": st["bytes"] / n, "stem_pool_ms_per_forward": st["ms"] / n,
                     "launches_per_forward": st["launches"] / n,
                     "by_launch": [{"algorithmic_mb": round(b / 1e6, 3), "median_ms": statistics.median(v),
                                    "min_ms": min(v), "max_ms": max(v), "launches": len(v)}
                                   for b, v in sorted(per.items(), reverse=True)]}
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--child", default=None, choices=("f32", "u8"), help="(internal) run one variant and print JSON")
    ap.add_argument("--root", default=ROOT, help="(with --child) the tree whose package is imported")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.root, a.batch, a.child, a.reps, a.lanes)))
        return

    variants = [("f32", ROOT, "f32"), ("u8", ROOT, "u8")]
    if a.baseline_root:
        variants.insert(0, ("base_f32", os.path.abspath(a.baseline_root), "f32"))
    rounds = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, root, kind in variants:  # alternating: every round visits every variant
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--root", root, "--batch", str(a.batch),
                   "--reps", str(a.reps), "--lanes", str(a.lanes)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"child {name} failed (rc {p.returncode}):\n{p.stdout}\n{p.stderr}")
            row = json.loads(p.stdout.strip().splitlines()[-1])
            rounds[name].append(row)
            print(json.dumps({"round": r, "variant": name, **row}), flush=True)
    res = {"gemm": "f16x3", "steps": STEPS, "B": a.batch, "reps": a.reps, "rounds": a.rounds, "lanes": a.lanes,
           "variants": {}}
    for name, rows in rounds.items():
        v = {"bytes_per_step": rows[0]["bytes_per_step"]}
        for k in rows[0]:
            if k.endswith("_ms"):
                xs = [r[k] for r in rows]
                v[k] = {"median": statistics.median(xs), "spread": max(xs) - min(xs), "rounds": xs}
        res["variants"][name] = v
    res["stems"] = stems(a.batch)
    ref = res["variants"].get("base_f32", res["variants"]["f32"])
    legs = [k for k in ref if k.endswith("_ms")]
    res["float_spread_ms"] = {k: max(ref[k]["spread"], res["variants"]["f32"][k]["spread"]) for k in legs}
    res["u8_minus_reference_float_ms"] = {k: res["variants"]["u8"][k]["median"] - ref[k]["median"] for k in legs}
    res["conditions"] = {
        "resident_u8_not_slower_than_float_beyond_spread":
            res["u8_minus_reference_float_ms"]["resident_ms"] <= res["float_spread_ms"]["resident_ms"],
        "host_fed_u8_faster_than_float": all(res["u8_minus_reference_float_ms"][k] < 0 for k in legs if "host" in k)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
