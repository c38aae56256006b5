"""Simulate candidate trajectories on the GPU: NAVSIM's PDM LQR tracker + kinematic bicycle (``dd_simulate``).

The PDM score (navsim/evaluate/pdm_score.py:83-140) scores the states ``PDMSimulator.simulate_proposals`` produces
from a planner's trajectory, never the waypoints themselves. ``simulate_trajectories`` runs that simulation for every
candidate of a device tensor in one launch sequence - ``trajectory`` (B, 8, 3), ``poses_reg`` (B, 20, 8, 3) or the
samples outputs (B, S, 20, 8, 3), read in place - in float64 as the reference does; ``simulate_proposals`` takes
41-pose proposals that are already on the 0.1 s grid. ``comfort_metrics`` scores the comfort sub-score of those states
on the device (``dd_comfort``: the six flags of ``ego_is_comfortable``, pdm_comfort_metrics.py:313-336), and
``ego_areas`` the map flags of every state with the drivable-area and driving-direction compliance scores
(``dd_ego_areas``: ``PDMScorer._calculate_ego_area``, pdm_scorer.py:240-291, 351-396) against maps packed once by
``pack_drivable_maps``. Collision, progress and TTC need the observations and the centerline as well and are out of
scope. There is no CPU fallback: a missing library or device raises.
"""
import ctypes
from typing import Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
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


# ---- map compliance (dd_ego_areas): PDMScorer._calculate_ego_area and the two scores taken from it alone

NUM_AREAS = 3    # EgoAreaIndex: multiple lanes, non-drivable area, oncoming traffic
NUM_COORDS = 5   # BBCoordsIndex: front-left, rear-left, rear-right, front-right, center
KIND_LANE, KIND_DRIVABLE, KIND_ON_ROUTE = 1, 2, 4   # dd_drivable_maps.poly_kind
# SemanticMapLayer names _calculate_ego_area reads (pdm_scorer.py:251-262)
LAYER_KINDS = {"LANE": KIND_LANE, "LANE_CONNECTOR": KIND_LANE, "ROADBLOCK": KIND_DRIVABLE,
               "INTERSECTION": KIND_DRIVABLE, "DRIVABLE_AREA": KIND_DRIVABLE, "CARPARK_AREA": KIND_DRIVABLE}


class PackedDrivableMaps(NamedTuple):
    """``dd_drivable_maps``: the polygons of G scenes as flat device tensors (include/ddmi.h)."""
    verts: torch.Tensor           # float64 (V, 2)
    ring_off: torch.Tensor        # int32 (R + 1)
    poly_ring_off: torch.Tensor   # int32 (P + 1)
    poly_kind: torch.Tensor       # uint8 (P)
    scene_poly_off: torch.Tensor  # int32 (G + 1)


class EgoAreas(NamedTuple):
    areas: torch.Tensor                # bool (..., 41, 3): multiple lanes, non-drivable area, oncoming traffic
    drivable_area: torch.Tensor        # float64 (...): 0 if any state is non-drivable, else 1
    driving_direction: torch.Tensor    # float64 (...): 1, 0.5 or 0
    oncoming_progress: torch.Tensor    # float64 (...): the largest windowed oncoming progress in metres
    coords: Optional[torch.Tensor]     # float64 (..., 41, 5, 2) or None


def _scene_items(entry):
    """One scene's polygons as (rings, layer name, on_route) items: from a list of such items, or from a duck-typed
    PDMDrivableMap - alone when it carries ``route_lane_ids``, or as ``(drivable_map, route_lane_ids)``."""
    route = None
    if isinstance(entry, tuple) and len(entry) == 2 and hasattr(entry[0], "_geometries"):
        entry, route = entry
    if hasattr(entry, "_geometries"):
        if route is None:
            route = getattr(entry, "route_lane_ids", None)
        if route is None:
            raise ValueError("a drivable map needs route_lane_ids: pass (drivable_map, route_lane_ids) or set the "
                             "attribute")
        route = set(route)
        geoms, types, tokens = entry._geometries, entry.map_types, entry.tokens
        if not len(geoms) == len(types) == len(tokens):
            raise ValueError(f"drivable map with {len(geoms)} geometries, {len(types)} map types, {len(tokens)} tokens")
        return [([g.exterior.coords] + [r.coords for r in g.interiors], t, tok in route)
                for g, t, tok in zip(geoms, types, tokens)]
    return list(entry)


def pack_drivable_maps(maps: Sequence, device) -> PackedDrivableMaps:
    """The maps of G scenes -> the flat tensors ``dd_ego_areas`` reads, on ``device``. ``maps`` has one entry per
    scene: a list of ``(rings, layer, on_route)`` items - ``rings`` the polygon's rings, exterior first, each an (n, 2)
    sequence of x, y whose closing edge is implied (a repeated closing vertex is harmless); ``layer`` one of the
    SemanticMapLayer names in ``LAYER_KINDS`` or an enum member with such a ``name``; ``on_route`` whether the
    polygon's token is among the route's lane ids - or a duck-typed ``PDMDrivableMap``, read only through
    ``_geometries[i].exterior.coords`` / ``.interiors``, ``map_types[i].name`` and ``tokens``, given as
    ``(drivable_map, route_lane_ids)`` or carrying a ``route_lane_ids`` attribute. A scene may have no polygons.
    Raises ``ValueError`` on a ring with fewer than 3 vertices, a non-finite vertex or an unknown layer name: the
    device trusts these arrays."""
    verts, ring_off, poly_ring_off, kinds, scene_poly_off = [], [0], [0], [], [0]
    nv = 0
    for g, entry in enumerate(maps):
        for i, item in enumerate(_scene_items(entry)):
            try:
                rings, layer, on_route = item
            except (TypeError, ValueError):
                raise ValueError(f"scene {g} polygon {i}: expected (rings, layer, on_route)") from None
            name = getattr(layer, "name", layer)
            if name not in LAYER_KINDS:
                raise ValueError(f"scene {g} polygon {i}: unknown layer name {name!r} (known: {sorted(LAYER_KINDS)})")
            kind = LAYER_KINDS[name]
            if on_route and kind == KIND_LANE:
                kind |= KIND_ON_ROUTE
            if len(rings) == 0:
                raise ValueError(f"scene {g} polygon {i}: no rings")
            for r, ring in enumerate(rings):
                a = np.asarray(ring, dtype=np.float64)
                if a.ndim != 2 or a.shape[1] != 2:
                    raise ValueError(f"scene {g} polygon {i} ring {r}: expected (n, 2) vertices, got {a.shape}")
                if a.shape[0] < 3:
                    raise ValueError(f"scene {g} polygon {i} ring {r}: {a.shape[0]} vertices, fewer than 3")
                if not np.isfinite(a).all():
                    raise ValueError(f"scene {g} polygon {i} ring {r}: non-finite vertex")
                verts.append(a)
                nv += a.shape[0]
                ring_off.append(nv)
            poly_ring_off.append(len(ring_off) - 1)
            kinds.append(kind)
        scene_poly_off.append(len(kinds))
    if nv >= 2 ** 31:
        raise ValueError(f"{nv} vertices do not fit the int32 offsets")
    v = np.concatenate(verts) if verts else np.zeros((0, 2))
    dev = torch.device(device)
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    return PackedDrivableMaps(torch.from_numpy(np.ascontiguousarray(v)).to(dev), i32(ring_off), i32(poly_ring_off),
                              torch.from_numpy(np.asarray(kinds, dtype=np.uint8)).to(dev), i32(scene_poly_off))


def default_area_params(lib=None) -> _lib.DDAreaParams:
    """``dd_default_area_params``: the vehicle's half length, half width and rear-axle-to-center distance, dt = 0.1 s,
    the driving-direction horizon 1 s and thresholds 2 m / 6 m (pdm_scorer.py:45-47)."""
    p = _lib.DDAreaParams()
    (lib or _lib.load()).dd_default_area_params(ctypes.byref(p))
    return p


def _area_params(params: Union[None, _lib.DDAreaParams, Mapping], lib) -> _lib.DDAreaParams:
    if isinstance(params, _lib.DDAreaParams):
        return params
    p = default_area_params(lib)
    for k, v in (params or {}).items():
        if k not in dict(p._fields_):
            raise ValueError(f"unknown area parameter {k!r}")
        setattr(p, k, v)
    return p


def ego_areas(states: torch.Tensor, maps, params=None, coords: bool = False,
              stream: Optional[torch.cuda.Stream] = None) -> EgoAreas:
    """``PDMScorer._calculate_ego_area`` and the drivable-area and driving-direction compliance scores
    (pdm_scorer.py:240-291, 351-396) on the device. ``states``: device float64 (B, ..., 41, 11), exactly what
    ``simulate_trajectories`` / ``simulate_proposals`` return, read in place; ``maps``: ``pack_drivable_maps``' result
    for the B scenes (or what it takes: packed here, on every call); every candidate of ``states[b]`` is scored on
    scene b's map. Returns an ``EgoAreas``: ``areas`` (..., 41, 3) torch.bool - in multiple lanes, in non-drivable
    area, in oncoming traffic; ``drivable_area``, ``driving_direction`` and ``oncoming_progress`` (...) float64;
    ``coords`` (..., 41, 5, 2) float64 - the four corners and the center the flags are taken from - if asked for,
    else None. ``params``: a ``DDAreaParams`` or a mapping of overrides of ``default_area_params()``. A bad argument
    raises ``ValueError`` with ``dd_last_error()``'s text."""
    lib = _lib.load()
    if not isinstance(states, torch.Tensor) or states.device.type != "cuda":
        raise ValueError("states must be a device tensor (simulate_trajectories' / simulate_proposals' output)")
    if states.dtype != torch.float64 or states.dim() < 3 or tuple(states.shape[-2:]) != (NUM_STATES, STATE_SIZE):
        raise ValueError(f"states must be float64 (B, ..., {NUM_STATES}, {STATE_SIZE}), got {tuple(states.shape)} "
                         f"{states.dtype}")
    states = states.contiguous()
    dev = states.device
    if not isinstance(maps, PackedDrivableMaps):
        maps = pack_drivable_maps(maps, dev)
    want = (torch.float64, torch.int32, torch.int32, torch.uint8, torch.int32)
    for name, t, dt in zip(maps._fields, maps, want):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"maps.{name} must be a contiguous {dt} tensor on {dev}")
    lead = tuple(states.shape[:-2])
    n = 1
    for d in lead:
        n *= d
    scenes = int(maps.scene_poly_off.numel()) - 1
    if scenes != lead[0]:
        raise ValueError(f"maps holds {scenes} scenes for {lead[0]} (the first dimension of states)")
    per_group = n // lead[0] if lead[0] else 0
    num_polys = int(maps.poly_kind.numel())
    if int(maps.poly_ring_off.numel()) != num_polys + 1 or int(maps.verts.numel()) % 2:
        raise ValueError("maps is not what pack_drivable_maps returns: poly_ring_off / verts do not fit poly_kind")
    p = _area_params(params, lib)
    m = _lib.DDDrivableMaps(maps.verts.data_ptr() or None, maps.ring_off.data_ptr() or None,
                            maps.poly_ring_off.data_ptr() or None, maps.poly_kind.data_ptr() or None,
                            maps.scene_poly_off.data_ptr() or None, num_polys)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):  # the outputs and the scratch belong to the stream that runs
        areas = torch.empty((*lead, NUM_STATES, NUM_AREAS), dtype=torch.uint8, device=dev)
        scores = torch.empty((*lead, 2), dtype=torch.float64, device=dev)
        progress = torch.empty(lead, dtype=torch.float64, device=dev)
        pts = torch.empty((*lead, NUM_STATES, NUM_COORDS, 2), dtype=torch.float64, device=dev) if coords else None
        work = torch.empty((lib.dd_ego_areas_work(num_polys),), dtype=torch.float64, device=dev)
        rc = lib.dd_ego_areas(states.data_ptr(), n, per_group, ctypes.byref(m), scenes, ctypes.byref(p),
                              work.data_ptr(), areas.data_ptr(), scores.data_ptr(), progress.data_ptr(),
                              pts.data_ptr() if coords else None, s.cuda_stream)
    if rc == -1:  # DD_ERR_INVALID
        raise ValueError((lib.dd_last_error() or b"").decode(errors="replace"))
    _lib.check(rc, lib)
    return EgoAreas(areas.view(torch.bool), scores[..., 0], scores[..., 1], progress, pts)
