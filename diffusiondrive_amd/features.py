"""Input feature builder on the GPU (the input side of the boundary).

Mirrors ``TransfuserFeatureBuilder`` (transfuser_features.py:25-138) so ``compute_trajectory``
works end to end on an ``AgentInput``, with the per-pixel / per-point work in HIP kernels
(``csrc/features.hip`` through the C ABI ``dd_build_camera`` / ``dd_build_lidar``):

* camera: the raw l0 / f0 / r0 uint8 images go to the device as-is (18.7 MB per scene instead of
  a CPU stitch + cv2 resize); one kernel crops, stitches, resizes (cv2 INTER_LINEAR at the exact
  4x NAVSIM factor) and converts to float CHW / 255.
* LiDAR: ``lidar_pc[:3]`` (contiguous planar x, y, z rows of NAVSIM's (6, N) array) goes to the
  device unchanged; one atomic histogram pass + an in-place finalize produce the (C, 256, 256)
  splat (``np.histogramdd`` semantics, bit-exact; tests/golden/lidar_feat_*.npz).
* status: [driving_command (4), ego_velocity (2), ego_acceleration (2)] (:46-53), 8 floats.

Both sensor features are byte-valued by construction (camera k / 255, LiDAR min(c, hist_max) / hist_max), and the
forward takes them as those bytes (include/ddmi.h, dd_inputs): ``dtype=torch.uint8`` makes the builders write the
(B, H, W, 3) HWC resized image and the (B, C, 256, 256) clipped counts instead of the floats (a quarter of the bytes,
bit-identical forward), and ``quantize_features`` turns a float feature dict into that form - or refuses, if a value is
not exactly byte-valued.

Features are returned as DEVICE tensors (the forward consumes them in place). There is no CPU
fallback: without libddmi.so or a GPU this raises. The CPU restatement used to check it lives in
``oracle/features.py`` (test infrastructure).
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import TransfuserConfig

# Host staging of the raw sensors: one reusable page-locked buffer per (device, kind), filled by a small pool of
# copy threads (np.copyto releases the GIL) straight from the caller's arrays, then one asynchronous H2D copy.
# The previous call's copy out of a buffer is waited for (its event) before the buffer is refilled. Replaces a
# np.stack + a fresh pin_memory() allocation + a pageable copy per call (C6 H2D-inclusive path).
_stage_lock = threading.Lock()
_stages: Dict[tuple, list] = {}
_pool: Optional[ThreadPoolExecutor] = None


def _cpu_share() -> int:
    """Host threads this process may use: min(sched affinity, the cgroup CPU quota) - a GPU box shows the whole
    machine's CPUs to os.cpu_count() but grants one job a share of them."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                n = min(n, max(1, -(-int(q) // int(per))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def _copy_pool() -> ThreadPoolExecutor:
    """$DDMI_COPY_THREADS copy threads (default: min(8, the CPU share))."""
    global _pool
    if _pool is None:
        n = int(os.environ.get("DDMI_COPY_THREADS", "0") or 0) or min(8, _cpu_share())
        _pool = ThreadPoolExecutor(max_workers=max(1, n))
    return _pool


def _stage(dev: torch.device, kind: str, numel: int, dtype: torch.dtype) -> torch.Tensor:
    """A pinned host tensor of >= numel elements for (dev, kind); the caller holds _stage_lock."""
    key = (dev.index, kind)
    ent = _stages.get(key)
    if ent is not None and ent[1] is not None:
        ent[1].synchronize()  # the H2D copy issued out of it last time has finished
    if ent is None or ent[0].numel() < numel:
        ent = [torch.empty(max(numel, 1), dtype=dtype, pin_memory=True), None]
        _stages[key] = ent
    ent[1] = None
    return ent[0]


_copy_streams: Dict[int, torch.cuda.Stream] = {}


def _upload(dev: torch.device, kind: str, host: torch.Tensor, shape) -> torch.Tensor:
    """Asynchronous H2D copy of the staged bytes on a copy stream of its own (so it overlaps a forward still
    running on the compute stream), which the current stream then waits for; the stage stays busy until it lands."""
    cs = _copy_streams.get(dev.index)
    if cs is None:
        cs = _copy_streams[dev.index] = torch.cuda.Stream(device=dev)
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.stream(cs):
        d = host.view(*shape).to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cs)
    cur.wait_event(ev)
    d.record_stream(cur)
    _stages[(dev.index, kind)][1] = ev
    return d


def _upload_chunked(dev: torch.device, kind: str, host: torch.Tensor, shape, items: int, copy_item,
                    groups: int = 4) -> torch.Tensor:
    """The staging copy and the H2D copy pipelined: the items (images) are copied into the pinned stage in `groups`
    runs by the copy threads, and each run's H2D copy is issued on the copy stream as soon as it is staged, so the
    transfer of one run overlaps the host copy of the next (the host copy of ~400 MB per 64 scenes and its H2D were
    serial before). The current stream waits for the last transfer; the stage stays busy until it lands."""
    cs = _copy_streams.get(dev.index)
    if cs is None:
        cs = _copy_streams[dev.index] = torch.cuda.Stream(device=dev)
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.stream(cs):  # allocated for the copy stream (no wait on the caller's queued work)
        d = torch.empty(tuple(shape), dtype=host.dtype, device=dev)
    flat_h, flat_d = host.view(items, -1), d.view(items, -1)
    per = -(-items // groups)
    pool = _copy_pool()
    for lo in range(0, items, per):
        hi = min(items, lo + per)
        list(pool.map(copy_item, range(lo, hi)))
        with torch.cuda.stream(cs):
            flat_d[lo:hi].copy_(flat_h[lo:hi], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(cs)
    cur.wait_event(ev)
    d.record_stream(cur)
    _stages[(dev.index, kind)][1] = ev
    return d


def _device(device: Optional[int]) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.DDMIUnavailable("the feature builder runs on the GPU (torch.cuda.is_available() is False)")
    return torch.device(f"cuda:{torch.cuda.current_device() if device is None else int(device)}")


def _check_dtype(dtype):
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"feature dtype must be torch.float32 or torch.uint8, got {dtype!r}")
    return dtype == torch.uint8


def widen_features(features: Dict[str, torch.Tensor], cfg: TransfuserConfig) -> Dict[str, torch.Tensor]:
    """The float features a uint8 feature dict stands for, in the reference's layouts: camera (B, H, W, 3) bytes ->
    (B, 3, H, W) ``k / 255``, LiDAR counts -> ``min(c, hist_max) / hist_max`` (float64 division rounded to float32,
    as the reference's numpy does). Float entries pass through. Pure torch: works without a GPU."""
    out = dict(features)
    cam, lid = torch.as_tensor(features["camera_feature"]), torch.as_tensor(features["lidar_feature"])
    if cam.dtype == torch.uint8:
        out["camera_feature"] = cam.permute(0, 3, 1, 2).float().div(255).contiguous()
    if lid.dtype == torch.uint8:
        hm = int(cfg.hist_max_per_pixel)
        out["lidar_feature"] = (lid.clamp(max=hm).double() / hm).float()
    return out


def quantize_features(features: Dict[str, torch.Tensor], cfg: TransfuserConfig) -> Dict[str, torch.Tensor]:
    """The uint8 form of a float feature dict: ``camera_feature`` (B, 3, H, W) -> (B, H, W, 3) bytes k with
    ``k / 255 == value``, ``lidar_feature`` -> the counts c with ``c / hist_max_per_pixel == value``; the other entries
    pass through, as do features that are uint8 already. Exact or not at all: a value that is not bit-equal to its
    byte's float raises ValueError naming the first offending element - nothing is ever rounded silently, so
    ``widen_features(quantize_features(x)) == x`` bitwise. Pure torch: works without a GPU."""
    hm = int(cfg.hist_max_per_pixel)
    if not 1 <= hm <= 255:
        raise ValueError(f"uint8 LiDAR features need hist_max_per_pixel in 1..255, got {hm}")
    out = dict(features)

    def exact(name, x, scale, back):
        x = torch.as_tensor(x)
        if x.dtype == torch.uint8:
            return x, None
        x = x.float()
        q = (x.double() * scale).round().clamp(0, scale)
        q = torch.where(torch.isfinite(q), q, torch.zeros_like(q)).to(torch.uint8)
        bad = (back(q) != x).reshape(-1)  # NaN, out of range and off-grid values all differ from their byte's float
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(x.shape)))
            raise ValueError(f"{name}{list(idx)} = {float(x.reshape(-1)[i])!r} is not k / {scale} for an integer k in "
                             f"0..{scale}: the feature is not byte-valued and cannot be passed as uint8")
        return q, x

    cam, was = exact("camera_feature", features["camera_feature"], 255, lambda q: q.float().div(255))
    out["camera_feature"] = cam.permute(0, 2, 3, 1).contiguous() if was is not None else cam
    lid, _ = exact("lidar_feature", features["lidar_feature"], hm, lambda q: (q.double() / hm).float())
    out["lidar_feature"] = lid
    return out


def camera_features(images: Sequence[Sequence[np.ndarray]], cfg: TransfuserConfig,
                    device: Optional[int] = None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """images: per scene (cam_l0, cam_f0, cam_r0) uint8 HWC arrays -> (B, 3, H, W) float on the GPU, or with
    ``dtype=torch.uint8`` the (B, H, W, 3) resized image itself (the float form is it / 255)."""
    u8 = _check_dtype(dtype)
    lib = _lib.load()
    dev = _device(device)
    B = len(images)
    if B == 0 or any(len(sc) != 3 for sc in images):
        raise ValueError("camera images: one (cam_l0, cam_f0, cam_r0) triple per scene, at least one scene")
    h, w = images[0][1].shape[:2]
    for sc in images:
        for im in sc:
            if im.dtype != np.uint8 or im.shape != (h, w, 3):
                raise ValueError(f"camera images must be uint8 ({h}, {w}, 3), got {im.dtype} {im.shape}")
    n = B * 3 * h * w * 3
    with _stage_lock:
        stage = _stage(dev, "camera", n, torch.uint8)[:n]
        arr = stage.numpy().reshape(B, 3, h, w, 3)
        cams = _upload_chunked(dev, "camera", stage, (B, 3, h, w, 3), 3 * B,
                               lambda bc: np.copyto(arr[bc // 3, bc % 3], images[bc // 3][bc % 3]))
    if u8:
        out = torch.empty((B, cfg.camera_height, cfg.camera_width, 3), device=dev, dtype=torch.uint8)
    else:
        out = torch.empty((B, 3, cfg.camera_height, cfg.camera_width), device=dev)
    s = torch.cuda.current_stream(dev)
    build = lib.dd_build_camera_u8 if u8 else lib.dd_build_camera
    _lib.check(build(cams.data_ptr(), B, h, w, out.data_ptr(), cfg.camera_height, cfg.camera_width,
                     s.cuda_stream), lib, op=True)
    out.record_stream(s)
    cams.record_stream(s)
    return out


def lidar_features(points: Sequence[np.ndarray], cfg: TransfuserConfig, device: Optional[int] = None,
                   dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """points: per scene a (3, N) float32 planar xyz array (NAVSIM ``lidar_pc[:3]``) ->
    (B, C, 256, 256) float on the GPU, or with ``dtype=torch.uint8`` the clipped counts min(c, hist_max_per_pixel)
    (the float form is them / hist_max_per_pixel)."""
    u8 = _check_dtype(dtype)
    lib = _lib.load()
    dev = _device(device)
    B = len(points)
    planes = [np.ascontiguousarray(p[:3], dtype=np.float32) for p in points]
    counts = np.array([p.shape[1] for p in planes], np.int64)
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum(counts)
    n = int(3 * offs[-1])
    with _stage_lock:
        stage = _stage(dev, "lidar", n, torch.float32)[:n]
        flat = stage.numpy()
        list(_copy_pool().map(lambda b: np.copyto(flat[3 * offs[b]:3 * offs[b + 1]], planes[b].reshape(-1)), range(B)))
        xyz_d = _upload(dev, "lidar", stage, (n,))
    offs_d = torch.from_numpy(offs).to(dev)
    C = cfg.lidar_in_channels
    res = cfg.lidar_resolution_height
    if cfg.lidar_resolution_width != res:
        raise ValueError("lidar feature: square BEV grid expected")
    out = torch.empty((B, C, res, res), device=dev, dtype=torch.uint8 if u8 else torch.float32)
    s = torch.cuda.current_stream(dev)
    build = lib.dd_build_lidar_u8 if u8 else lib.dd_build_lidar
    _lib.check(build(xyz_d.data_ptr() if xyz_d.numel() else None, offs_d.data_ptr(), B, C,
                     out.data_ptr(), res, float(cfg.lidar_min_x), float(cfg.lidar_max_x),
                     int(cfg.pixels_per_meter), float(cfg.max_height_lidar),
                     float(cfg.lidar_split_height), int(cfg.hist_max_per_pixel),
                     int(counts.max()) if B else 0, s.cuda_stream), lib, op=True)
    out.record_stream(s)
    xyz_d.record_stream(s)
    offs_d.record_stream(s)
    return out


def status_features(egos: Sequence, device: Optional[int] = None) -> torch.Tensor:
    """transfuser_features.py:46-53: [driving_command, ego_velocity, ego_acceleration] per scene."""
    dev = _device(device)
    rows = [np.concatenate([np.asarray(e.driving_command, np.float32), np.asarray(e.ego_velocity, np.float32),
                            np.asarray(e.ego_acceleration, np.float32)]) for e in egos]
    return torch.from_numpy(np.stack(rows)).to(dev)


class TransfuserFeatureBuilder:
    """transfuser_features.py:25-55 (inference features only), computed on the GPU."""

    def __init__(self, config: TransfuserConfig, device: Optional[int] = None, dtype: torch.dtype = torch.float32):
        """``dtype=torch.uint8``: the camera / LiDAR features as bytes ((B,H,W,3) image, (B,C,256,256) counts), which
        the forward reads in place."""
        _check_dtype(dtype)
        self._config = config
        self._device = device
        self._dtype = dtype

    def get_unique_name(self) -> str:
        return "transfuser_feature"

    def compute_features(self, agent_input) -> Dict[str, torch.Tensor]:
        """One scene, as the reference: (3,256,1024), (C,256,256), (8,) - device tensors."""
        f = self.compute_features_batch([agent_input])
        return {k: v[0] for k, v in f.items()}

    def compute_features_batch(self, agent_inputs: List) -> Dict[str, torch.Tensor]:
        """Many scenes at once (batched eval): (B,3,256,1024), (B,C,256,256), (B,8)."""
        cams = [(a.cameras[-1].cam_l0.image, a.cameras[-1].cam_f0.image, a.cameras[-1].cam_r0.image)
                for a in agent_inputs]
        pcs = [a.lidars[-1].lidar_pc[0:3] for a in agent_inputs]  # LidarIndex.POSITION (x, y, z)
        return {
            "camera_feature": camera_features(cams, self._config, self._device, dtype=self._dtype),
            "lidar_feature": lidar_features(pcs, self._config, self._device, dtype=self._dtype),
            "status_feature": status_features([a.ego_statuses[-1] for a in agent_inputs], self._device),
        }
