"""dd_forward_samples / DiffusionDriveModel.forward_samples on the host: argument checks that run before any GPU work,
and the draw-block rule of the device noise (include/ddmi.h) restated against the Philox reference."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import samples_util as S
from philox_ref import device_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handle_is_refused():
    """dd_forward_samples(NULL, ...) returns DD_ERR_INVALID with the reason, as every entry point does."""
    from diffusiondrive_amd import _lib
    lib = _lib.load()
    outs = _lib.DDSampleOutputs()
    assert lib.dd_forward_samples(None, None, None, None, None, 1, 2, 2, ctypes.byref(outs), None) == -1
    assert b"null" in lib.dd_last_error()
    assert lib.dd_forward_samples(None, None, None, None, None, 1, 2, 2, None, None) == -1
    assert b"null" in lib.dd_last_error()


def test_header_and_binding_agree():
    """DD_MAX_SAMPLES and the output struct's fields of include/ddmi.h are what the ctypes binding declares; the ABI
    version is unchanged (functions were added, nothing changed)."""
    from diffusiondrive_amd import _lib
    with open(os.path.join(ROOT, "include", "ddmi.h")) as f:
        h = f.read()
    assert int(re.search(r"#define DD_MAX_SAMPLES (\d+)", h).group(1)) == _lib.MAX_SAMPLES == S.MAX_SAMPLES
    assert int(re.search(r"#define DD_ABI_VERSION (\d+)", h).group(1)) == 1
    body = re.search(r"typedef struct dd_sample_outputs \{(.*?)\} dd_sample_outputs;", h, re.S).group(1)
    fields = re.findall(r"(?:float|int)\*\s+(\w+);", body)
    assert fields == [n for n, _ in _lib.DDSampleOutputs._fields_]


def _hostless_model():
    """A DiffusionDriveModel with no handle and no GPU: whatever it does before touching either can run here."""
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel.__new__(DiffusionDriveModel)
    m.config = TransfuserConfig()
    m.device = 0
    m._h = None
    return m


@pytest.mark.parametrize("n", [0, -1, S.MAX_SAMPLES + 1, 2.0, True, None])
def test_num_samples_is_validated_before_gpu_work(n):
    """num_samples outside 1..32 (or not an integer) is a ValueError raised before any device call: the model here
    has no handle and this machine may have no GPU."""
    feats = {"camera_feature": torch.zeros(2, 3, 256, 1024), "lidar_feature": torch.zeros(2, 1, 256, 256),
             "status_feature": torch.zeros(2, 8)}
    with pytest.raises(ValueError, match="num_samples"):
        _hostless_model().forward_samples(feats, n)


@pytest.mark.parametrize("shape", [(2, 20, 8, 2), (2, 3, 20, 8, 3), (3, 3, 20, 8, 2), (2, 4, 20, 8, 2), (2, 3, 8, 20, 2)])
def test_noise_shape_is_validated_before_gpu_work(shape):
    """A noise tensor that is not (B, S, Q, P, 2) is a ValueError before any device call; so is a noise string other
    than "device"."""
    feats = {"camera_feature": torch.zeros(2, 3, 256, 1024), "lidar_feature": torch.zeros(2, 1, 256, 256),
             "status_feature": torch.zeros(2, 8)}
    with pytest.raises(ValueError, match="noise must be"):
        _hostless_model().forward_samples(feats, 3, noise=torch.zeros(shape))
    with pytest.raises(ValueError, match="noise must be"):
        _hostless_model().forward_samples(feats, 3, noise="host")


def test_python_surface():
    """forward_samples on the model and the in-flight planner take the same arguments; the agent's forward_trajectory
    defaults to one sample and compute_trajectories exists."""
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    from diffusiondrive_amd.model import DiffusionDriveModel, InFlightPlanner
    pm = inspect.signature(DiffusionDriveModel.forward_samples).parameters
    assert list(pm) == ["self", "features", "num_samples", "noise", "steps", "heads", "modes", "best", "stream"]
    pl = inspect.signature(InFlightPlanner.forward_samples).parameters
    assert list(pl) == [k for k in pm if k != "stream"]
    assert inspect.signature(DiffusionDriveAgent.forward_trajectory).parameters["num_samples"].default == 1
    assert list(inspect.signature(DiffusionDriveAgent.compute_trajectories).parameters) == \
        ["self", "agent_input", "num_samples"]


def test_draw_block_rule():
    """Sample s of scene b takes block position + b * S + s of Q * P * 2 = 320 normals: every block is a slice of the
    one long draw, a samples call's noise is the contiguous window of its B * S blocks, and S = 1 reproduces the
    per-scene windows of dd_forward (scene s -> draws [320 s, 320 (s + 1)))."""
    seed, B, Sn, pos = 99, 3, 4, 5
    long = device_normals(seed, 0, (pos + B * Sn) * 320)
    for b in range(B):
        for s in range(Sn):
            first, n = S.block_window(pos, b, Sn, s)
            assert n == 320 and first == (pos + b * Sn + s) * 320
            assert np.array_equal(device_normals(seed, first, n), long[first:first + n])
    call = np.concatenate([device_normals(seed, *S.block_window(pos, b, Sn, s)) for b in range(B) for s in range(Sn)])
    assert np.array_equal(call, device_normals(seed, pos * 320, B * Sn * 320))
    for scene in range(4):
        assert S.block_window(0, scene, 1, 0) == (320 * scene, 320)
    # a shard of a samples run starts at first_scene * S blocks
    assert S.block_window(2 * Sn, 0, Sn, 0) == S.block_window(0, 2, Sn, 0)


def test_head_passes_keep_the_decoder_scenes_within_the_chunk_limit():
    """The head passes of a chunk: consecutive ranges that cover it, none with more than max_chunk decoder scenes."""
    for n, Sn, mc in [(64, 4, 128), (128, 32, 128), (3, 3, 4), (2, 3, 4), (5, 1, 128), (7, 3, 10), (128, 3, 128)]:
        ps = S.head_passes(n, Sn, mc)
        assert ps[0][0] == 0 and sum(c for _, c in ps) == n
        assert all(a + c == b for (a, c), (b, _) in zip(ps, ps[1:]))
        assert all(c * Sn <= mc for _, c in ps)
    assert S.head_passes(64, 4) == [(0, 32), (32, 32)] and S.head_passes(3, 3, 4) == [(0, 1), (1, 1), (2, 1)]
    assert S.head_passes(5, 1) == [(0, 5)]
    assert [S.decoder_groups(d) for d in (16, 17, 32, 33)] == [4, 2, 2, 1]
