"""uint8 camera / LiDAR features on the host: quantize_features (exact or not at all), the byte value maps, and the
dd_inputs descriptor / the *_in entry points of include/ddmi.h against the ctypes binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    from diffusiondrive_amd.config import TransfuserConfig
    return TransfuserConfig()


def _synthetic(B=2):
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(B, 7, _cfg())
    return {k: torch.from_numpy(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}


def test_quantize_round_trips_byte_valued_features():
    """synthetic_inputs is exactly byte-valued: quantize_features returns the uint8 dict (HWC camera, planar counts),
    and widening it gives the input back bit for bit."""
    from diffusiondrive_amd.features import quantize_features, widen_features
    cfg, f = _cfg(), _synthetic()
    q = quantize_features(f, cfg)
    assert q["camera_feature"].dtype == torch.uint8 and tuple(q["camera_feature"].shape) == (2, 256, 1024, 3)
    assert q["lidar_feature"].dtype == torch.uint8 and tuple(q["lidar_feature"].shape) == (2, 1, 256, 256)
    assert q["status_feature"] is f["status_feature"]
    assert int(q["lidar_feature"].max()) == cfg.hist_max_per_pixel and int(q["camera_feature"].max()) == 255
    # the value maps of the contract, written out
    assert torch.equal(q["camera_feature"].permute(0, 3, 1, 2).float().div(255), f["camera_feature"])
    hm = cfg.hist_max_per_pixel
    assert torch.equal((q["lidar_feature"].clamp(max=hm).double() / hm).float(), f["lidar_feature"])
    w = widen_features(q, cfg)
    for k in ("camera_feature", "lidar_feature"):
        assert w[k].dtype == torch.float32 and torch.equal(w[k].view(torch.int32), f[k].view(torch.int32)), k
    # uint8 features pass through
    q2 = quantize_features(q, cfg)
    assert torch.equal(q2["camera_feature"], q["camera_feature"]) and torch.equal(q2["lidar_feature"], q["lidar_feature"])


@pytest.mark.parametrize("key,idx,val", [("camera_feature", (1, 2, 200, 1000), 0.5),
                                         ("lidar_feature", (0, 0, 17, 3), 0.3),
                                         ("camera_feature", (0, 0, 0, 5), float("nan")),
                                         ("camera_feature", (0, 1, 3, 3), 1.5),
                                         ("lidar_feature", (1, 0, 255, 255), -0.2),
                                         ("camera_feature", (0, 0, 9, 9), float(np.float32(1 / 255) * np.float32(3)))])
def test_quantize_never_rounds(key, idx, val):
    """A value that is not exactly its byte's float (0.5 is no k / 255, 0.3f no c / 5; NaN, out of range, and
    3 * (1/255.f), which is not 3 / 255.f) raises ValueError naming the element."""
    from diffusiondrive_amd.features import quantize_features
    f = _synthetic()
    f[key] = f[key].clone()
    f[key][idx] = val
    with pytest.raises(ValueError, match=re.escape(f"{key}{list(idx)}")):
        quantize_features(f, _cfg())


def test_reciprocal_multiply_is_not_the_camera_map():
    """k / 255.f (the contract, torch's .float().div(255)) against k * (1 / 255.f): they differ for many bytes, which is
    why the table holds the division and why bit-identity tests can catch the shortcut."""
    k = np.arange(256, dtype=np.float32)
    div = k / np.float32(255)
    mul = k * (np.float32(1) / np.float32(255))
    assert np.array_equal(div, torch.arange(256, dtype=torch.uint8).float().div(255).numpy())
    assert int((div != mul).sum()) == 126
    # LiDAR: the double division rounded to float equals the float division for every hist_max
    for hm in range(1, 256):
        c = np.minimum(np.arange(256), hm)
        assert np.array_equal((c.astype(np.float64) / hm).astype(np.float32), c.astype(np.float32) / np.float32(hm))


def _header():
    with open(os.path.join(ROOT, "include", "ddmi.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _decl_args(h, name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", h, re.S)
    assert m, f"{name} is not declared in include/ddmi.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_binding_agree():
    """dd_inputs and the new entry points are declared in include/ddmi.h and bound in _lib.py with the same fields and
    argument counts; the additions leave the ABI version at 1."""
    from diffusiondrive_amd import _lib
    h = _header()
    assert int(re.search(r"#define DD_ABI_VERSION (\d+)", h).group(1)) == 1
    body = re.search(r"typedef struct dd_inputs \{(.*?)\} dd_inputs;", h, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == ["camera_f32", "camera_u8", "lidar_f32", "lidar_u8", "lidar_hist_max", "status", "noise"]
    assert fields == [n for n, _ in _lib.DDInputs._fields_]
    types = dict(_lib.DDInputs._fields_)
    assert types["lidar_hist_max"] is ctypes.c_int
    assert all(types[n] is ctypes.c_void_p for n in fields if n != "lidar_hist_max")
    assert ctypes.sizeof(_lib.DDInputs) == 7 * 8  # four pointers, an int padded to 8, two pointers
    for name in ("dd_forward_in", "dd_forward_samples_in", "dd_forward_train_in", "dd_build_camera_u8",
                 "dd_build_lidar_u8", "dd_op_stem_pool_u8"):
        args = _decl_args(h, name)
        res, argtypes = _lib._SIGS[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), (name, args, argtypes)
        assert name in _lib.EXPORTED
    # the descriptor entries are the float entries with the four input pointers replaced by the descriptor
    for new, old in (("dd_forward_in", "dd_forward_ex"), ("dd_forward_samples_in", "dd_forward_samples"),
                     ("dd_forward_train_in", "dd_forward_train")):
        assert len(_decl_args(h, new)) == len(_decl_args(h, old)) - 3
        assert _decl_args(h, new)[1].startswith("const dd_inputs*")
    # the uint8 builders take their float siblings' arguments
    for new, old in (("dd_build_camera_u8", "dd_build_camera"), ("dd_build_lidar_u8", "dd_build_lidar")):
        assert len(_decl_args(h, new)) == len(_decl_args(h, old))


def test_entry_points_are_exported_and_validate_before_gpu_work():
    """The built library exports the entries; a null handle or descriptor is refused with the reason (no device work:
    this machine may have no GPU)."""
    from diffusiondrive_amd import _lib
    lib = _lib.load()
    outs = _lib.DDOutputs()
    ins = _lib.DDInputs()
    assert lib.dd_forward_in(None, ctypes.byref(ins), 1, 2, ctypes.byref(outs), None) == -1
    assert b"null" in lib.dd_last_error()
    souts = _lib.DDSampleOutputs()
    assert lib.dd_forward_samples_in(None, ctypes.byref(ins), 1, 2, 2, ctypes.byref(souts), None) == -1
    assert b"null" in lib.dd_last_error()
    touts = _lib.DDTrainOutputs()
    assert lib.dd_forward_train_in(None, ctypes.byref(ins), None, None, 1, 10.0, 8.0, ctypes.byref(touts), None) == -1
    assert b"null" in lib.dd_last_error()
    assert lib.dd_op_stem_pool_u8(None, 0, 1, 3, 8, 8, None, None, None, None, 0, None, None) == -1
    assert b"stem_pool_u8" in lib.dd_op_last_error()


def test_uint8_shape_is_validated_before_gpu_work():
    """A uint8 camera that is not (B, H, W, 3) is a ValueError before any device call (no handle, no GPU here)."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel.__new__(DiffusionDriveModel)
    m.config, m.device, m._h = _cfg(), 0, None
    chw = torch.zeros(2, 3, 256, 1024, dtype=torch.uint8)
    lid = torch.zeros(2, 1, 256, 256, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 camera_feature must be HWC"):
        m._sensor_inputs({"camera_feature": chw, "lidar_feature": lid}, 2)
    with pytest.raises(ValueError, match="lidar_feature"):
        m._sensor_inputs({"camera_feature": chw.permute(0, 2, 3, 1), "lidar_feature": lid[:, :, :8]}, 2)


def test_feature_dtype_reaches_the_builder():
    """BatchedTrajectoryRunner(feature_dtype=...) and TransfuserFeatureBuilder(dtype=...) carry the dtype to the GPU
    builders (float32 by default); anything but float32 / uint8 is refused at construction."""
    from types import SimpleNamespace
    from diffusiondrive_amd.features import TransfuserFeatureBuilder
    from diffusiondrive_amd.runner import BatchedTrajectoryRunner
    agent = SimpleNamespace(_config=_cfg(), _transfuser_model=SimpleNamespace(device=0))
    assert BatchedTrajectoryRunner(agent).builder._dtype == torch.float32
    assert BatchedTrajectoryRunner(agent, feature_dtype=torch.uint8).builder._dtype == torch.uint8
    assert TransfuserFeatureBuilder(_cfg())._dtype == torch.float32
    with pytest.raises(ValueError, match="dtype"):
        TransfuserFeatureBuilder(_cfg(), dtype=torch.float16)
