"""The forward's launch sequence, launch by launch, against a recording.

tests/golden/forward_routes.json (test_batch_sweep_gpu.py) keeps the batch-independent *set* of routes of the default
mode. This module holds the ordered list of (kernel, detail) of one profiled B = 2 forward with the heads on - every
launch's M / N / K / k / s / z / HW, its route (cfg=, groups=, form=) and its place in the order - in five setups
that together reach every launch helper of the runtime: the default f16x3 mode, gemm fp32 (dense value maps, NHWC4
stems, the K-sliced bev_proj), gemm bf16, f16x3 with every fused form switched off, and the ResNet-50 config
(Bottleneck stages). Two scenes, so that a launch which mistakes a group for a row shows in its M or HW.

tests/golden/launch_shapes_b2.json was recorded from a library built at the commit before the launch helpers moved to
operand views (this file's __main__ with DDMI_LIB naming that library), so the lists pin that commit's launches; after
a change that is meant to alter a launch, record it again the same way.
"""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_shapes_b2.json")
UNFUSED = {"DDMI_DECODER_MK": "0", "DDMI_TFDEC_MK": "0", "DDMI_FUSE_POOL": "0", "DDMI_LN_FOLD": "0",
           "DDMI_BEVPROJ": "concat"}  # bev_proj mode 0
# name: (gemm mode, environment of the handle, image trunk)
CASES = {
    "f16x3": ("f16x3", {}, "resnet34"),
    "fp32": ("fp32", {}, "resnet34"),
    "bf16": ("bf16", {}, "resnet34"),
    "f16x3_unfused": ("f16x3", UNFUSED, "resnet34"),
    "f16x3_resnet50": ("f16x3", {}, "resnet50"),
}
B, SEED = 2, 77


def launch_sequence(case, mp, log):
    """[[kernel, detail], ...] of one profiled forward of ``case`` (after a profiled warm-up forward, so the launches
    of a handle's first call are not in it). mp: a pytest.MonkeyPatch; log: the path the library appends to."""
    from batch_sweep_util import read_launch_log
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import seeded_state_dict, synthetic_inputs
    mode, env, arch = CASES[case]
    for k, v in env.items():
        mp.setenv(k, v)
    cfg = TransfuserConfig(image_architecture=arch)
    m = DiffusionDriveModel(cfg, seeded_state_dict(cfg, 0), device=0)
    try:
        m.set_gemm_mode(mode)
        inp = synthetic_inputs(B, SEED, cfg)
        feats = {k: torch.from_numpy(inp[k]).cuda() for k in ("camera_feature", "lidar_feature", "status_feature")}
        noise = torch.from_numpy(inp["noise"]).cuda()
        m.set_profiling(True)
        m.forward(feats, noise=noise, heads=True)
        torch.cuda.synchronize()
        mp.setenv("DDMI_LAUNCH_LOG", str(log))
        m.forward(feats, noise=noise, heads=True)
        torch.cuda.synchronize()
        m.set_profiling(False)
    finally:
        m.close()
    return [list(e) for e in read_launch_log(log)]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence_matches_recording(gpu, golden, tmp_path, monkeypatch, case):
    got, want = launch_sequence(case, monkeypatch, tmp_path / "launches.tsv"), golden[case]
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, (case, len(got), len(want), first, got[first:first + 3], want[first:first + 3])


if __name__ == "__main__":  # record: DDMI_LIB=<library of the commit to pin> python tests/test_launch_shapes_gpu.py [out]
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out, rec = sys.argv[1] if len(sys.argv) > 1 else GOLDEN, {}
    for name in CASES:
        with pytest.MonkeyPatch.context() as mp, tempfile.TemporaryDirectory() as tmp:
            rec[name] = launch_sequence(name, mp, os.path.join(tmp, "launches.tsv"))
        print(name, len(rec[name]), "launches", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
