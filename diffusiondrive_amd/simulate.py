"""Simulate candidate trajectories on the GPU: NAVSIM's PDM LQR tracker + kinematic bicycle (``dd_simulate``).

The PDM score (navsim/evaluate/pdm_score.py:83-140) scores the states ``PDMSimulator.simulate_proposals`` produces
from a planner's trajectory, never the waypoints themselves. ``simulate_trajectories`` runs that simulation for every
candidate of a device tensor in one launch sequence - ``trajectory`` (B, 8, 3), ``poses_reg`` (B, 20, 8, 3) or the
samples outputs (B, S, 20, 8, 3), read in place - in float64 as the reference does; ``simulate_proposals`` takes
41-pose proposals that are already on the 0.1 s grid. ``comfort_metrics`` scores the comfort sub-score of those states
on the device (``dd_comfort``: the six flags of ``ego_is_comfortable``, pdm_comfort_metrics.py:313-336); the other
sub-scores need the map and the observations and are out of scope. There is no CPU fallback: a missing library or
device raises.
"""
import ctypes
from typing import Mapping, Optional, Tuple, Union

import torch

from . import _lib

NUM_POSES = 8    # planner poses per candidate (0.5 s apart)
NUM_STATES = 41  # simulated states per candidate (0.1 s apart, the start state first)
STATE_SIZE = 11  # StateIndex of pdm_enums.py: x, y, heading, vx, vy, ax, ay, steering angle / rate, yaw rate / accel
NUM_COMFORT = 6  # lon / lat acceleration, jerk magnitude, lon jerk, yaw acceleration, yaw rate (the reference's order)


def default_params(lib=None) -> _lib.DDSimParams:
    """``dd_default_sim_params``: the reference's tracker and bicycle constants."""
    p = _lib.DDSimParams()
    (lib or _lib.load()).dd_default_sim_params(ctypes.byref(p))
    return p


def _params(params: Union[None, _lib.DDSimParams, Mapping], lib) -> _lib.DDSimParams:
    if isinstance(params, _lib.DDSimParams):
        return params
    p = default_params(lib)
    for k, v in (params or {}).items():
        if k not in dict(p._fields_):
            raise ValueError(f"unknown simulation parameter {k!r}")
        setattr(p, k, tuple(v) if k == "q_lat" else v)
    return p


def _ego(ego_states: torch.Tensor, device) -> torch.Tensor:
    ego = torch.as_tensor(ego_states)
    if ego.dtype != torch.float64 or ego.dim() != 2 or ego.shape[1] != STATE_SIZE:
        raise ValueError(f"ego_states must be a (B, {STATE_SIZE}) float64 tensor, got {tuple(ego.shape)} {ego.dtype}")
    return ego.to(device).contiguous()


def _run(entry, lib, src, ego, n, per_group, params, stream):
    dev = src.device
    p = _params(params, lib)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):  # the output and the scratch belong to the stream that runs
        out = torch.empty((n, NUM_STATES, STATE_SIZE), dtype=torch.float64, device=dev)
        work = torch.empty((lib.dd_simulate_work(n),), dtype=torch.float64, device=dev)
        rc = entry(src, ego, n, per_group, ctypes.byref(p), work.data_ptr(), out.data_ptr(), s.cuda_stream)
    if rc == -1:  # DD_ERR_INVALID
        raise ValueError((lib.dd_last_error() or b"").decode(errors="replace"))
    _lib.check(rc, lib)
    return out


def simulate_trajectories(traj: torch.Tensor, ego_states: torch.Tensor, params=None,
                          stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Planner output -> simulated states. ``traj``: device float32 (B, ..., 8, 3) poses in the ego frame, exactly as
    the forwards write them; ``ego_states``: (B, 11) float64 start states in the StateIndex order of pdm_enums.py (the
    rear-axle pose in the frame the result should be in), scene b's for every candidate of ``traj[b]``. Returns
    (B, ..., 41, 11) float64 on ``traj``'s device: state 0 is the start state, state t the vehicle after t tracker +
    bicycle steps of 0.1 s. ``params``: a ``DDSimParams`` or a mapping of overrides of the reference defaults.
    A bad argument raises ``ValueError`` with ``dd_last_error()``'s text."""
    lib = _lib.load()
    if not isinstance(traj, torch.Tensor) or traj.device.type != "cuda":
        raise ValueError("traj must be a device tensor (the forwards' trajectory / poses_reg output)")
    if traj.dtype != torch.float32 or traj.dim() < 3 or traj.shape[-1] != 3:
        raise ValueError(f"traj must be float32 (B, ..., {NUM_POSES}, 3), got {tuple(traj.shape)} {traj.dtype}")
    traj = traj.contiguous()
    ego = _ego(ego_states, traj.device)
    lead = tuple(traj.shape[:-2])
    n = 1
    for d in lead:
        n *= d
    if ego.shape[0] != lead[0]:
        raise ValueError(f"ego_states has {ego.shape[0]} rows for {lead[0]} scenes")
    per_group = n // lead[0] if lead[0] else 0
    num_poses = int(traj.shape[-2])

    def entry(src, ego_t, n_, pg, p, work, out, s):
        return lib.dd_simulate(src.data_ptr(), num_poses, ego_t.data_ptr(), n_, pg, p, work, out, s)

    out = _run(entry, lib, traj, ego, n, per_group, params, stream)
    return out.view(*lead, NUM_STATES, STATE_SIZE)


def simulate_proposals(proposals: torch.Tensor, ego_states: torch.Tensor, params=None, per_group: Optional[int] = None,
                       stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """``PDMSimulator.simulate_proposals``: device float64 (N, 41, 3) proposals [x, y, heading] at 0.1 s and (G, 11)
    float64 start states -> (N, 41, 11); candidate n starts from ``ego_states[n // per_group]`` (per_group = N / G by
    default)."""
    lib = _lib.load()
    if not isinstance(proposals, torch.Tensor) or proposals.device.type != "cuda":
        raise ValueError("proposals must be a device tensor")
    if proposals.dtype != torch.float64 or proposals.dim() != 3 or tuple(proposals.shape[1:]) != (NUM_STATES, 3):
        raise ValueError(f"proposals must be float64 (N, {NUM_STATES}, 3), got {tuple(proposals.shape)} "
                         f"{proposals.dtype}")
    proposals = proposals.contiguous()
    ego = _ego(ego_states, proposals.device)
    n = int(proposals.shape[0])
    if per_group is None:
        per_group = n // ego.shape[0] if ego.shape[0] and n % ego.shape[0] == 0 else 0
    elif per_group > 0 and n % per_group == 0 and ego.shape[0] != n // per_group:
        raise ValueError(f"ego_states has {ego.shape[0]} rows for {n // per_group} groups")

    def entry(src, ego_t, n_, pg, p, work, out, s):
        return lib.dd_simulate_proposals(src.data_ptr(), ego_t.data_ptr(), n_, pg, p, work, out, s)

    return _run(entry, lib, proposals, ego, n, int(per_group), params, stream)


def default_comfort_params(lib=None) -> _lib.DDComfortParams:
    """``dd_default_comfort_params``: dt = 0.1 s and the reference's seven bounds (pdm_comfort_metrics.py:11-28)."""
    p = _lib.DDComfortParams()
    (lib or _lib.load()).dd_default_comfort_params(ctypes.byref(p))
    return p


def _comfort_params(params: Union[None, _lib.DDComfortParams, Mapping], lib) -> _lib.DDComfortParams:
    if isinstance(params, _lib.DDComfortParams):
        return params
    p = default_comfort_params(lib)
    for k, v in (params or {}).items():
        if k not in dict(p._fields_):
            raise ValueError(f"unknown comfort parameter {k!r}")
        setattr(p, k, v)
    return p


def comfort_metrics(states: torch.Tensor, params=None, signals: bool = False,
                    stream: Optional[torch.cuda.Stream] = None
                    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``ego_is_comfortable`` (pdm_comfort_metrics.py:313-336) on the device. ``states``: device float64
    (..., 41, 11), exactly what ``simulate_trajectories`` / ``simulate_proposals`` return, read in place. Returns
    ``flags`` (..., 6) torch.bool - lon acceleration, lat acceleration, jerk magnitude, lon jerk, yaw acceleration, yaw
    rate within their bounds at every sample - or ``(flags, signals)`` with the six rounded series (..., 6, 41) float64
    the flags are taken from. ``params``: a ``DDComfortParams`` or a mapping of overrides of the reference's values; a
    bound of exactly 0 means no bound on that side, as in the reference. A bad argument raises ``ValueError`` with
    ``dd_last_error()``'s text."""
    lib = _lib.load()
    if not isinstance(states, torch.Tensor) or states.device.type != "cuda":
        raise ValueError("states must be a device tensor (simulate_trajectories' / simulate_proposals' output)")
    if states.dtype != torch.float64 or states.dim() < 2 or tuple(states.shape[-2:]) != (NUM_STATES, STATE_SIZE):
        raise ValueError(f"states must be float64 (..., {NUM_STATES}, {STATE_SIZE}), got {tuple(states.shape)} "
                         f"{states.dtype}")
    states = states.contiguous()
    lead = tuple(states.shape[:-2])
    n = 1
    for d in lead:
        n *= d
    dev = states.device
    p = _comfort_params(params, lib)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):  # the outputs belong to the stream that runs
        flags = torch.empty((*lead, NUM_COMFORT), dtype=torch.uint8, device=dev)
        sig = torch.empty((*lead, NUM_COMFORT, NUM_STATES), dtype=torch.float64, device=dev) if signals else None
        rc = lib.dd_comfort(states.data_ptr(), n, ctypes.byref(p), flags.data_ptr(),
                            sig.data_ptr() if signals else None, s.cuda_stream)
    if rc == -1:  # DD_ERR_INVALID
        raise ValueError((lib.dd_last_error() or b"").decode(errors="replace"))
    _lib.check(rc, lib)
    flags = flags.view(torch.bool)
    return (flags, sig) if signals else flags
