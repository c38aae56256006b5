"""Simulate candidate trajectories on the GPU: NAVSIM's PDM LQR tracker + kinematic bicycle (``dd_simulate``).

The PDM score (navsim/evaluate/pdm_score.py:83-140) scores the states ``PDMSimulator.simulate_proposals`` produces
from a planner's trajectory, never the waypoints themselves. ``simulate_trajectories`` runs that simulation for every
candidate of a device tensor in one launch sequence - ``trajectory`` (B, 8, 3), ``poses_reg`` (B, 20, 8, 3) or the
samples outputs (B, S, 20, 8, 3), read in place - in float64 as the reference does; ``simulate_proposals`` takes
41-pose proposals that are already on the 0.1 s grid. ``comfort_metrics`` scores the comfort sub-score of those states
on the device (``dd_comfort``: the six flags of ``ego_is_comfortable``, pdm_comfort_metrics.py:313-336), and
``ego_areas`` the map flags of every state with the drivable-area and driving-direction compliance scores
(``dd_ego_areas``: ``PDMScorer._calculate_ego_area``, pdm_scorer.py:240-291, 351-396) against maps packed once by
``pack_drivable_maps``. ``collisions`` scores no-at-fault collision and time-to-collision against the tracked objects
packed by ``pack_observations`` (``dd_collisions``: :293-349 and :414-498), ``progress`` the raw progress along the
centerlines packed by ``pack_centerlines`` (``dd_progress``: :398-412), ``aggregate`` combines the sub-scores
(``dd_pdm_aggregate``: ``_aggregate_scores``, :156-183), and ``pdm_score`` chains all of it on one stream, so that
candidates are ranked by PDM score without leaving the device. ``generate_proposals`` / ``pdm_closed`` run PDM-Closed's
candidate stage in front of it (``dd_proposals``), and ``observe`` builds the forecasted observation both read from the
current detections (``dd_observe``: ``PDMObservation.update``, pdm_observation.py:105-205), packed by
``pack_detections`` or taken from the agent head by ``detections_from_agent_head``. There is no CPU fallback: a missing
library or device raises.
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


def pack_drivable_maps(maps: Sequence, device, layers: Optional[Sequence[str]] = None) -> PackedDrivableMaps:
    """The maps of G scenes -> the flat tensors ``dd_ego_areas`` reads, on ``device``. ``maps`` has one entry per
    scene: a list of ``(rings, layer, on_route)`` items - ``rings`` the polygon's rings, exterior first, each an (n, 2)
    sequence of x, y whose closing edge is implied (a repeated closing vertex is harmless); ``layer`` one of the
    SemanticMapLayer names in ``LAYER_KINDS`` or an enum member with such a ``name``; ``on_route`` whether the
    polygon's token is among the route's lane ids - or a duck-typed ``PDMDrivableMap``, read only through
    ``_geometries[i].exterior.coords`` / ``.interiors``, ``map_types[i].name`` and ``tokens``, given as
    ``(drivable_map, route_lane_ids)`` or carrying a ``route_lane_ids`` attribute. A scene may have no polygons.
    ``layers``: keep only the polygons whose layer name is among these (``("INTERSECTION",)`` is what
    ``collisions`` reads); None keeps all. Raises ``ValueError`` on a ring with fewer than 3 vertices, a non-finite
    vertex or an unknown layer name: the device trusts these arrays."""
    verts, ring_off, poly_ring_off, kinds, scene_poly_off = [], [0], [0], [], [0]
    if layers is not None:
        layers = set(layers)
        unknown = layers - set(LAYER_KINDS)
        if unknown:
            raise ValueError(f"unknown layer names {sorted(unknown)} (known: {sorted(LAYER_KINDS)})")
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
            if layers is not None and name not in layers:
                continue
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


# ---- the rest of the score (dd_collisions, dd_progress, dd_pdm_aggregate): collisions, TTC, progress, aggregation

MIN_OBS_TIMES = 50            # TTC reads occupancy map t + 9 for t up to 40
RED_LIGHT_TOKEN = "red_light"  # PDMObservation.red_light_token: such tokens never count
AGENT_TYPE_NAMES = ("VEHICLE", "PEDESTRIAN", "BICYCLE")   # nuPlan's AGENT_TYPES, quoted from memory (include/ddmi.h)
TRACK_STOPPED_SPEED = 5e-2    # nuPlan's is_track_stopped, quoted from memory
FLAG_STOPPED, FLAG_AGENT = 1, 2   # dd_observations.flags


class PackedObservations(NamedTuple):
    """``dd_observations``: the tracked objects of G scenes as flat device tensors (include/ddmi.h)."""
    boxes: torch.Tensor            # float64 (K, T_obs, 4, 2): front-left, rear-left, rear-right, front-right
    valid: torch.Tensor            # uint8 (K, T_obs)
    heading: torch.Tensor          # float64 (K)
    flags: torch.Tensor            # uint8 (K): bit 0 stopped, bit 1 agent type
    scene_track_off: torch.Tensor  # int32 (G + 1)
    tokens: Tuple[Tuple[str, ...], ...]   # per scene, the packed tracks' tokens in order (host only)


class PackedCenterlines(NamedTuple):
    """``dd_centerlines``: the centerlines of G scenes as flat device tensors (include/ddmi.h)."""
    verts: torch.Tensor       # float64 (V, 2)
    scene_off: torch.Tensor   # int32 (G + 1)


class Collisions(NamedTuple):
    no_collision: torch.Tensor         # float64 (...): 1, 0.5 or 0
    collision_time_idx: torch.Tensor   # float64 (...): the first at-fault time index, inf if none
    ttc: torch.Tensor                  # float64 (...): 1 or 0
    ttc_time_idx: torch.Tensor         # float64 (...): the first TTC infraction's time index, inf if none


class PDMScores(NamedTuple):
    no_collision: torch.Tensor         # float64 (...): 1, 0.5 or 0
    drivable_area: torch.Tensor        # float64 (...): 1 or 0
    driving_direction: torch.Tensor    # float64 (...): 1, 0.5 or 0
    progress: torch.Tensor             # float64 (...): the normalised progress term
    ttc: torch.Tensor                  # float64 (...): 1 or 0
    comfort: torch.Tensor              # bool (..., 6)
    collision_time_idx: torch.Tensor   # float64 (...)
    ttc_time_idx: torch.Tensor         # float64 (...)
    raw_progress: torch.Tensor         # float64 (...): metres along the centerline
    score: torch.Tensor                # float64 (...)


def _quad(coords, what):
    a = np.asarray(coords, dtype=np.float64)
    if a.ndim == 2 and a.shape == (5, 2):
        a = a[:4]   # shapely's closed ring
    if a.shape != (4, 2):
        raise ValueError(f"{what}: a box is 4 (or 5, closed) x 2 coordinates, got {a.shape}")
    return a


def _scene_tracks(entry, g):
    """One scene's tracks as (token, boxes (T_obs, 4, 2), valid (T_obs), heading, is_agent, is_stopped), the red-light
    and previously collided tokens dropped."""
    out, seen = [], set()
    if hasattr(entry, "_occupancy_maps"):
        maps, skip = entry._occupancy_maps, set(entry.collided_track_ids)
        t_obs = len(maps)
        per = {}
        for t, m in enumerate(maps):
            if len(set(m.tokens)) != len(m.tokens):
                raise ValueError(f"scene {g} map {t}: duplicate token")
            for i, token in enumerate(m.tokens):
                if RED_LIGHT_TOKEN in token or token in skip:
                    continue
                if token not in per:
                    per[token] = (np.zeros((t_obs, 4, 2)), np.zeros(t_obs, dtype=bool))
                per[token][0][t] = _quad(m._geometries[i].exterior.coords, f"scene {g} map {t} token {token!r}")
                per[token][1][t] = True
        for token, (boxes, valid) in per.items():
            obj = entry.unique_objects[token]
            is_agent = obj.tracked_object_type.name in AGENT_TYPE_NAMES
            velocity = getattr(obj, "velocity", None)
            # is_track_stopped: not an Agent (no velocity), or an Agent at or below 5e-2 m/s
            stopped = velocity is None or float(velocity.magnitude()) <= TRACK_STOPPED_SPEED
            out.append((token, boxes, valid, float(obj.box.center.heading), is_agent, stopped))
        return out, t_obs
    t_obs = None
    for i, item in enumerate(entry):
        try:
            token, boxes, heading, is_agent, is_stopped = item
        except (TypeError, ValueError):
            raise ValueError(f"scene {g} track {i}: expected (token, boxes, heading, is_agent, is_stopped)") from None
        mask = None
        if isinstance(boxes, tuple):
            boxes, mask = boxes
        b = np.asarray(boxes, dtype=np.float64)
        if b.ndim == 3 and b.shape[1:] == (5, 2):
            b = b[:, :4]
        if b.ndim != 3 or b.shape[1:] != (4, 2):
            raise ValueError(f"scene {g} track {i}: boxes are (T_obs, 4 (or 5, closed), 2), got {b.shape}")
        valid = ~np.isnan(b).all(axis=(1, 2)) if mask is None else np.asarray(mask, dtype=bool)
        if valid.shape != (b.shape[0],):
            raise ValueError(f"scene {g} track {i}: the mask has shape {valid.shape} for {b.shape[0]} times")
        if t_obs is None:
            t_obs = b.shape[0]
        elif t_obs != b.shape[0]:
            raise ValueError(f"scene {g} track {i}: {b.shape[0]} times, the tracks before it {t_obs}")
        if token in seen:
            raise ValueError(f"scene {g} track {i}: duplicate token {token!r}")
        seen.add(token)
        if RED_LIGHT_TOKEN in token:
            continue
        out.append((token, np.where(valid[:, None, None], b, 0.0), valid, float(heading), bool(is_agent),
                    bool(is_stopped)))
    return out, t_obs


def pack_observations(observations: Sequence, device, collided: Optional[Sequence] = None) -> PackedObservations:
    """The tracked objects of G scenes -> the flat tensors ``dd_collisions`` reads, on ``device``. One entry per scene:
    a list of ``(token, boxes, heading, is_agent, is_stopped)`` - ``boxes`` (T_obs, 4, 2) float64, corners front-left,
    rear-left, rear-right, front-right, an all-NaN row where the object is absent, or ``(boxes, mask)`` with a
    (T_obs) bool mask of presence; ``heading`` the object's heading at its first appearance - or a duck-typed
    ``PDMObservation``, read only through ``_occupancy_maps[t].tokens`` / ``._geometries[i].exterior.coords``,
    ``collided_track_ids`` and ``unique_objects[token].box.center.heading`` / ``.tracked_object_type.name`` /
    ``.velocity.magnitude()`` where present (an object without a velocity is not an Agent and counts as stopped).
    ``collided[g]``: the list form's ``collided_track_ids``. Tokens containing "red_light" and tokens in the collided
    ids are DROPPED: both metrics skip them unconditionally. Raises ``ValueError`` on a box that is not 4 (or 5,
    closed) x 2, a non-finite box where the object is present, fewer than 50 times, scenes that disagree on T_obs, or
    a duplicate token: the device trusts these arrays."""
    boxes, valid, heading, flags, off, tokens = [], [], [], [], [0], []
    t_obs = None
    for g, entry in enumerate(observations):
        tracks, t_scene = _scene_tracks(entry, g)
        skip = set(collided[g]) if collided is not None and not hasattr(entry, "_occupancy_maps") else set()
        if t_scene is not None:
            if t_scene < MIN_OBS_TIMES:
                raise ValueError(f"scene {g}: T_obs = {t_scene} is below {MIN_OBS_TIMES} (TTC reads map t + 9)")
            if t_obs is not None and t_obs != t_scene:
                raise ValueError(f"scene {g}: T_obs = {t_scene}, the scenes before it {t_obs}")
            t_obs = t_scene
        names = []
        for token, b, v, h, is_agent, stopped in tracks:
            if token in skip:
                continue
            if not np.isfinite(b[v]).all():
                raise ValueError(f"scene {g} token {token!r}: non-finite box where the object is present")
            if not np.isfinite(h):
                raise ValueError(f"scene {g} token {token!r}: non-finite heading")
            boxes.append(b), valid.append(v), heading.append(h), names.append(token)
            flags.append((FLAG_STOPPED if stopped else 0) | (FLAG_AGENT if is_agent else 0))
        off.append(len(heading))
        tokens.append(tuple(names))
    t_obs = t_obs if t_obs is not None else MIN_OBS_TIMES
    dev = torch.device(device)
    k = len(heading)
    if k * t_obs * 8 >= 2 ** 31:
        raise ValueError(f"{k} tracks x {t_obs} times do not fit the int32 offsets")
    b = np.stack(boxes) if k else np.zeros((0, t_obs, 4, 2))
    v = np.stack(valid).astype(np.uint8) if k else np.zeros((0, t_obs), dtype=np.uint8)
    return PackedObservations(torch.from_numpy(np.ascontiguousarray(b)).to(dev), torch.from_numpy(v).to(dev),
                              torch.from_numpy(np.asarray(heading, dtype=np.float64)).to(dev),
                              torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(dev),
                              torch.from_numpy(np.asarray(off, dtype=np.int32)).to(dev), tuple(tokens))


def pack_centerlines(paths: Sequence, device) -> PackedCenterlines:
    """The centerlines of G scenes -> the flat tensors ``dd_progress`` reads. One entry per scene: an (L, 2) polyline
    or a duck-typed ``PDMPath``, read through ``_states_se2_array[:, :2]``. Raises ``ValueError`` on fewer than 2
    vertices or a non-finite vertex."""
    verts, off = [], [0]
    for g, path in enumerate(paths):
        a = np.asarray(path._states_se2_array if hasattr(path, "_states_se2_array") else path, dtype=np.float64)
        if a.ndim == 2 and a.shape[1] > 2 and hasattr(path, "_states_se2_array"):
            a = a[:, :2]
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"scene {g}: a centerline is (L, 2) vertices, got {a.shape}")
        if a.shape[0] < 2:
            raise ValueError(f"scene {g}: a centerline of {a.shape[0]} vertices, fewer than 2")
        if not np.isfinite(a).all():
            raise ValueError(f"scene {g}: non-finite centerline vertex")
        verts.append(a)
        off.append(off[-1] + a.shape[0])
    if off[-1] >= 2 ** 31:
        raise ValueError(f"{off[-1]} vertices do not fit the int32 offsets")
    dev = torch.device(device)
    v = np.concatenate(verts) if verts else np.zeros((0, 2))
    return PackedCenterlines(torch.from_numpy(np.ascontiguousarray(v)).to(dev),
                             torch.from_numpy(np.asarray(off, dtype=np.int32)).to(dev))


def default_score_params(lib=None) -> _lib.DDScoreParams:
    """``dd_default_score_params``: the weights 5 / 5 / 2 / 0, the progress threshold 5 m, the stopped speeds 5e-3
    (TTC) and 5e-2 (collision) and the ahead / behind bounds of 30 and 150 degrees."""
    p = _lib.DDScoreParams()
    (lib or _lib.load()).dd_default_score_params(ctypes.byref(p))
    return p


def _score_params(params: Union[None, _lib.DDScoreParams, Mapping], lib) -> _lib.DDScoreParams:
    if isinstance(params, _lib.DDScoreParams):
        return params
    p = default_score_params(lib)
    for k, v in (params or {}).items():
        if k not in dict(p._fields_):
            raise ValueError(f"unknown score parameter {k!r}")
        setattr(p, k, v)
    return p


def _states_arg(states, lead_dims):
    if not isinstance(states, torch.Tensor) or states.device.type != "cuda":
        raise ValueError("states must be a device tensor (simulate_trajectories' / simulate_proposals' output)")
    if (states.dtype != torch.float64 or states.dim() < 2 + lead_dims
            or tuple(states.shape[-2:]) != (NUM_STATES, STATE_SIZE)):
        raise ValueError(f"states must be float64 (B, ..., {NUM_STATES}, {STATE_SIZE}), got {tuple(states.shape)} "
                         f"{states.dtype}")
    states = states.contiguous()
    lead = tuple(states.shape[:-2])
    n = 1
    for d in lead:
        n *= d
    return states, lead, n


def _fields_on(packed, want, dev, name):
    for field, t, dt in zip(packed._fields, packed, want):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name}.{field} must be a contiguous {dt} tensor on {dev}")


def _raise(rc, lib):
    if rc == -1:  # DD_ERR_INVALID
        raise ValueError((lib.dd_last_error() or b"").decode(errors="replace"))
    _lib.check(rc, lib)


def collisions(states: torch.Tensor, areas: torch.Tensor, observations, intersections, area_params=None,
               score_params=None, stream: Optional[torch.cuda.Stream] = None) -> Collisions:
    """No-at-fault collision and time-to-collision (pdm_scorer.py:293-349, 414-498) on the device. ``states``: device
    float64 (B, ..., 41, 11); ``areas``: ``ego_areas(states, maps).areas`` (bool or uint8 (B, ..., 41, 3));
    ``observations``: ``pack_observations``' result for the B scenes (or what it takes: packed here);
    ``intersections``: ``pack_drivable_maps(maps, device, layers=("INTERSECTION",))``' result (or maps: filtered and
    packed here). Returns a ``Collisions`` of four float64 (B, ...) tensors. A bad argument raises ``ValueError`` with
    ``dd_last_error()``'s text."""
    lib = _lib.load()
    states, lead, n = _states_arg(states, 1)
    dev = states.device
    if not isinstance(areas, torch.Tensor) or areas.device != dev or areas.dtype not in (torch.bool, torch.uint8) \
            or tuple(areas.shape) != (*lead, NUM_STATES, NUM_AREAS):
        raise ValueError(f"areas must be ego_areas' bool or uint8 {(*lead, NUM_STATES, NUM_AREAS)} tensor on {dev}")
    areas = areas.contiguous().view(torch.uint8)
    if not isinstance(observations, PackedObservations):
        observations = pack_observations(observations, dev)
    if not isinstance(intersections, PackedDrivableMaps):
        intersections = pack_drivable_maps(intersections, dev, layers=("INTERSECTION",))
    _fields_on(observations, (torch.float64, torch.uint8, torch.float64, torch.uint8, torch.int32), dev, "observations")
    _fields_on(intersections, (torch.float64, torch.int32, torch.int32, torch.uint8, torch.int32), dev, "intersections")
    scenes = int(observations.scene_track_off.numel()) - 1
    if scenes != lead[0] or int(intersections.scene_poly_off.numel()) - 1 != lead[0]:
        raise ValueError(f"observations hold {scenes} scenes and intersections "
                         f"{int(intersections.scene_poly_off.numel()) - 1} for {lead[0]} (the first dimension of states)")
    per_group = n // lead[0] if lead[0] else 0
    k = int(observations.heading.numel())
    b = observations.boxes
    if b.dim() != 4 or tuple(b.shape[2:]) != (4, 2) or b.shape[0] != k or tuple(observations.valid.shape) != \
            (k, b.shape[1]) or int(observations.flags.numel()) != k:
        raise ValueError("observations is not what pack_observations returns: boxes / valid / flags do not fit heading")
    num_polys = int(intersections.poly_kind.numel())
    if int(intersections.poly_ring_off.numel()) != num_polys + 1:
        raise ValueError("intersections is not what pack_drivable_maps returns")
    ap, sp = _area_params(area_params, lib), _score_params(score_params, lib)
    o = _lib.DDObservations(b.data_ptr() or None, observations.valid.data_ptr() or None,
                            observations.heading.data_ptr() or None, observations.flags.data_ptr() or None,
                            observations.scene_track_off.data_ptr() or None, k, int(b.shape[1]))
    m = _lib.DDDrivableMaps(intersections.verts.data_ptr() or None, intersections.ring_off.data_ptr() or None,
                            intersections.poly_ring_off.data_ptr() or None, intersections.poly_kind.data_ptr() or None,
                            intersections.scene_poly_off.data_ptr() or None, num_polys)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):  # the outputs and the scratch belong to the stream that runs
        out = torch.empty((4, *lead), dtype=torch.float64, device=dev)
        work = torch.empty((lib.dd_collisions_work(k),), dtype=torch.float64, device=dev)
        rc = lib.dd_collisions(states.data_ptr(), areas.data_ptr(), n, per_group, ctypes.byref(o), ctypes.byref(m),
                               scenes, ctypes.byref(ap), ctypes.byref(sp), work.data_ptr(), out[0].data_ptr(),
                               out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), s.cuda_stream)
    _raise(rc, lib)
    return Collisions(out[0], out[1], out[2], out[3])


def progress(states: torch.Tensor, centerlines, area_params=None,
             stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Raw progress along the centerline (pdm_scorer.py:398-412) on the device: ``states`` device float64
    (B, ..., 41, 11), ``centerlines`` ``pack_centerlines``' result for the B scenes (or what it takes) -> float64
    (B, ...) metres, clipped at 0. A bad argument raises ``ValueError`` with ``dd_last_error()``'s text."""
    lib = _lib.load()
    states, lead, n = _states_arg(states, 1)
    dev = states.device
    if not isinstance(centerlines, PackedCenterlines):
        centerlines = pack_centerlines(centerlines, dev)
    _fields_on(centerlines, (torch.float64, torch.int32), dev, "centerlines")
    scenes = int(centerlines.scene_off.numel()) - 1
    if scenes != lead[0]:
        raise ValueError(f"centerlines holds {scenes} scenes for {lead[0]} (the first dimension of states)")
    per_group = n // lead[0] if lead[0] else 0
    ap = _area_params(area_params, lib)
    c = _lib.DDCenterlines(centerlines.verts.data_ptr() or None, centerlines.scene_off.data_ptr() or None,
                           int(centerlines.verts.numel()) // 2)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        out = torch.empty(lead, dtype=torch.float64, device=dev)
        rc = lib.dd_progress(states.data_ptr(), n, per_group, ctypes.byref(c), scenes, ctypes.byref(ap),
                             out.data_ptr(), s.cuda_stream)
    _raise(rc, lib)
    return out


def aggregate(no_collision: torch.Tensor, drivable_area: torch.Tensor, driving_direction: torch.Tensor,
              raw_progress: torch.Tensor, ttc: torch.Tensor, comfort: torch.Tensor, score_params=None,
              progress_reference: Optional[torch.Tensor] = None,
              stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``PDMScorer._aggregate_scores`` (pdm_scorer.py:156-183) on the device. The five float64 (B, ...) sub-scores and
    ``comfort`` (B, ..., 6) bool or uint8 -> ``(score, progress)``, both float64 (B, ...). The progress term is
    normalised by the largest ``raw_progress * no_collision * drivable_area`` of scene b's candidates
    (``score_proposals``' rule), or, with ``progress_reference`` (B) float64, per candidate by the larger of its own
    and the scene's reference value - the rule of navsim/evaluate/pdm_score.py:99-130, which scores each prediction as
    a pair with the PDM-closed trajectory, whose ``raw * multi`` is the reference."""
    lib = _lib.load()
    dev = no_collision.device if isinstance(no_collision, torch.Tensor) else None
    lead = tuple(no_collision.shape) if dev is not None else ()
    if dev is None or dev.type != "cuda" or len(lead) < 1:
        raise ValueError("no_collision must be a device tensor (B, ...)")
    ins = []
    for name, t in (("no_collision", no_collision), ("drivable_area", drivable_area),
                    ("driving_direction", driving_direction), ("raw_progress", raw_progress), ("ttc", ttc)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float64 or tuple(t.shape) != lead:
            raise ValueError(f"{name} must be a float64 {lead} tensor on {dev}")
        ins.append(t.contiguous())
    if not isinstance(comfort, torch.Tensor) or comfort.device != dev or comfort.dtype not in (torch.bool, torch.uint8) \
            or tuple(comfort.shape) != (*lead, NUM_COMFORT):
        raise ValueError(f"comfort must be a bool or uint8 {(*lead, NUM_COMFORT)} tensor on {dev}")
    comfort = comfort.contiguous().view(torch.uint8)
    n = 1
    for d in lead:
        n *= d
    per_group = n // lead[0] if lead[0] else 0
    if progress_reference is not None:
        if not isinstance(progress_reference, torch.Tensor) or progress_reference.dtype != torch.float64 \
                or tuple(progress_reference.shape) != (lead[0],):
            raise ValueError(f"progress_reference must be a float64 ({lead[0]},) tensor")
        progress_reference = progress_reference.to(dev).contiguous()
    sp = _score_params(score_params, lib)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        out = torch.empty((2, *lead), dtype=torch.float64, device=dev)
        rc = lib.dd_pdm_aggregate(*(t.data_ptr() for t in ins), comfort.data_ptr(), n, per_group, ctypes.byref(sp),
                                  progress_reference.data_ptr() if progress_reference is not None else None,
                                  out[0].data_ptr(), out[1].data_ptr(), s.cuda_stream)
    _raise(rc, lib)
    return out[0], out[1]


def pdm_score(states: torch.Tensor, maps, observations, centerlines, *, progress_reference=None, comfort_params=None,
              area_params=None, score_params=None, stream: Optional[torch.cuda.Stream] = None) -> PDMScores:
    """The PDM score of simulated candidates, all on the device and on one stream: ``comfort_metrics``, ``ego_areas``,
    ``collisions``, ``progress`` and ``aggregate``. ``states``: device float64 (B, ..., 41, 11); ``maps``: the B
    scenes' maps as ``pack_drivable_maps`` takes them (a ``PackedDrivableMaps`` serves the flags, but the TTC rule
    needs the INTERSECTION polygons alone: then pass ``(packed_all, packed_intersections)``); ``observations`` and
    ``centerlines``: packed or as the packers take them. Returns a ``PDMScores`` with the leading shape of
    ``states``."""
    states, lead, _ = _states_arg(states, 1)
    dev = states.device
    if isinstance(maps, tuple) and len(maps) == 2 and all(isinstance(m, PackedDrivableMaps) for m in maps):
        packed, inter = maps
    elif isinstance(maps, PackedDrivableMaps):
        raise ValueError("pdm_score needs the INTERSECTION polygons on their own: pass the maps themselves, or "
                         "(pack_drivable_maps(maps, device), pack_drivable_maps(maps, device, layers=('INTERSECTION',)))")
    else:
        packed, inter = pack_drivable_maps(maps, dev), pack_drivable_maps(maps, dev, layers=("INTERSECTION",))
    if not isinstance(observations, PackedObservations):
        observations = pack_observations(observations, dev)
    if not isinstance(centerlines, PackedCenterlines):
        centerlines = pack_centerlines(centerlines, dev)
    s = stream or torch.cuda.current_stream(dev)
    comfort = comfort_metrics(states, comfort_params, stream=s)
    ego = ego_areas(states, packed, area_params, stream=s)
    col = collisions(states, ego.areas, observations, inter, area_params, score_params, stream=s)
    raw = progress(states, centerlines, area_params, stream=s)
    score, term = aggregate(col.no_collision, ego.drivable_area.contiguous(), ego.driving_direction.contiguous(), raw,
                            col.ttc, comfort, score_params, progress_reference, stream=s)
    return PDMScores(col.no_collision, ego.drivable_area, ego.driving_direction, term, col.ttc, comfort,
                     col.collision_time_idx, col.ttc_time_idx, raw, score)


# ---- PDM-Closed's proposal generation (dd_proposals) and the planner's pick (dd_pdm_select)

MIN_LEAD_TIMES = 41           # the leader update at time index 40 reads occupancy map 40
MAX_POLICIES = 64             # one lane per policy of a path


class PackedPaths(NamedTuple):
    """``dd_paths``: the lateral paths of G scenes as flat device tensors (include/ddmi.h)."""
    verts: torch.Tensor        # float64 (V, 3): x, y, unwrapped heading
    progress: torch.Tensor     # float64 (V)
    path_off: torch.Tensor     # int32 (G P + 1)
    paths_per_scene: int


class PackedLeadObjects(NamedTuple):
    """``dd_lead_objects``: the tracks and stop polygons ``dd_proposals`` reads (include/ddmi.h)."""
    boxes: torch.Tensor            # float64 (K, T_obs, 4, 2)
    valid: torch.Tensor            # uint8 (K, T_obs)
    heading: torch.Tensor          # float64 (K)
    speed: torch.Tensor            # float64 (K)
    scene_track_off: torch.Tensor  # int32 (G + 1)
    stop_verts: torch.Tensor       # float64 (Vs, 2)
    ring_off: torch.Tensor         # int32 (R + 1)
    scene_ring_off: torch.Tensor   # int32 (G + 1)
    tokens: Tuple[Tuple[str, ...], ...]   # per scene, the packed tracks' tokens, then the rings' (host only)


class Proposals(NamedTuple):
    proposals: torch.Tensor              # float64 (G, P L, 41, 3): x, y, heading
    idm: Optional[torch.Tensor]          # float64 (G, P L, 41, 2): progress, velocity
    lead: Optional[torch.Tensor]         # float64 (G, P L, 41, 3): the leader's progress, velocity, rear length
    lead_index: Optional[torch.Tensor]   # int32 (G, P L, 41): object index in the scene (tracks, then rings), -1 free


class PDMClosed(NamedTuple):
    scores: PDMScores                    # of all (G, P L) proposals
    best_index: torch.Tensor             # int32 (G)
    best_states: torch.Tensor            # float64 (G, 41, 11)
    progress_reference: torch.Tensor     # float64 (G): what pdm_score(progress_reference=) takes
    proposals: torch.Tensor              # float64 (G, P L, 41, 3)
    states: torch.Tensor                 # float64 (G, P L, 41, 11)


def pack_paths(paths: Sequence, device) -> PackedPaths:
    """The lateral paths of G scenes -> the flat tensors ``dd_proposals`` reads. One entry per scene: a sequence of P
    paths (the same P in every scene), each a (V, 3) array of x, y, heading - the heading is unwrapped and the
    cumulative progress formed here as ``PDMPath.__init__`` forms them (np.unwrap; calculate_progress: diff, norm,
    cumsum) - or a duck-typed ``PDMPath``, read through ``_states_se2_array`` and ``_progress``. Raises ``ValueError``
    on fewer than 2 vertices, a non-finite value, a progress that decreases, or a length <= 1e-5."""
    verts, progress, off = [], [], [0]
    per_scene = None
    for g, scene in enumerate(paths):
        scene = list(scene)
        if per_scene is None:
            per_scene = len(scene)
        if len(scene) != per_scene or per_scene == 0:
            raise ValueError(f"scene {g}: {len(scene)} paths, the scenes before it {per_scene} (at least 1, the same "
                             "in every scene)")
        for i, path in enumerate(scene):
            if hasattr(path, "_states_se2_array"):
                a = np.array(path._states_se2_array, dtype=np.float64)
                s = np.array(path._progress, dtype=np.float64)
            else:
                a = np.array(path, dtype=np.float64)
                s = None
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"scene {g} path {i}: a path is (V, 3) x, y, heading, got {a.shape}")
            if a.shape[0] < 2:
                raise ValueError(f"scene {g} path {i}: {a.shape[0]} vertices, fewer than 2")
            if not np.isfinite(a).all():
                raise ValueError(f"scene {g} path {i}: non-finite value")
            if s is None:
                a[:, 2] = np.unwrap(a[:, 2], axis=0)
                diff = np.concatenate(([np.diff(a[:, 0])], [np.diff(a[:, 1])]), axis=0, dtype=np.float64)
                s = np.cumsum(np.append(0.0, np.linalg.norm(diff, axis=0)), dtype=np.float64)
            if s.shape != (a.shape[0],) or not np.isfinite(s).all() or (np.diff(s) < 0.0).any():
                raise ValueError(f"scene {g} path {i}: the progress must be {a.shape[0]} finite values that never "
                                 "decrease")
            if not s[-1] - s[0] > 1e-5 or s[0] != 0.0:
                raise ValueError(f"scene {g} path {i}: the progress must start at 0 and the length {s[-1] - s[0]} be "
                                 "above 1e-5")
            verts.append(a), progress.append(s)
            off.append(off[-1] + a.shape[0])
    if per_scene is None:
        raise ValueError("no scenes")
    if off[-1] >= 2 ** 31 // 3:
        raise ValueError(f"{off[-1]} vertices do not fit the int32 offsets")
    dev = torch.device(device)
    return PackedPaths(torch.from_numpy(np.ascontiguousarray(np.concatenate(verts))).to(dev),
                       torch.from_numpy(np.ascontiguousarray(np.concatenate(progress))).to(dev),
                       torch.from_numpy(np.asarray(off, dtype=np.int32)).to(dev), per_scene)


def _ring(coords, what):
    a = np.asarray(coords, dtype=np.float64)
    if a.ndim == 2 and a.shape[0] > 1 and a.shape[1] >= 2 and (a[0, :2] == a[-1, :2]).all():
        a = a[:-1]   # shapely's closed ring
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: a ring is (n, 2) vertices, got {a.shape}")
    if a.shape[0] < 3:
        raise ValueError(f"{what}: {a.shape[0]} vertices, fewer than 3")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: non-finite vertex")
    return a


def _scene_lead_objects(entry, g, rings, collided):
    """One scene's (tracks: (token, boxes, valid, heading, speed)), (rings: (token, (n, 2))), T_obs."""
    tracks, stops = [], []
    if hasattr(entry, "_occupancy_maps"):
        maps, skip = entry._occupancy_maps, set(entry.collided_track_ids)
        t_obs = len(maps)
        per = {}
        for t, m in enumerate(maps):
            if len(set(m.tokens)) != len(m.tokens):
                raise ValueError(f"scene {g} map {t}: duplicate token")
            for i, token in enumerate(m.tokens):
                if token in skip:
                    continue
                if RED_LIGHT_TOKEN in token:   # static over time: the first map that holds it
                    if token not in per:
                        per[token] = None
                        stops.append((token, _ring(m._geometries[i].exterior.coords, f"scene {g} token {token!r}")))
                    continue
                if token not in per:
                    per[token] = (np.zeros((t_obs, 4, 2)), np.zeros(t_obs, dtype=bool))
                per[token][0][t] = _quad(m._geometries[i].exterior.coords, f"scene {g} map {t} token {token!r}")
                per[token][1][t] = True
        for token, pair in per.items():
            if pair is None:
                continue
            obj = entry.unique_objects[token]
            velocity = getattr(obj, "velocity", None)   # an object without a velocity is no nuPlan Agent
            tracks.append((token, pair[0], pair[1], float(obj.box.center.heading),
                           0.0 if velocity is None else float(velocity.magnitude())))
        return tracks, stops, t_obs
    t_obs, seen = None, set()
    for i, item in enumerate(entry):
        try:
            token, boxes, heading, _, _, speed = item
        except (TypeError, ValueError):
            raise ValueError(f"scene {g} track {i}: expected (token, boxes, heading, is_agent, is_stopped, speed)") \
                from None
        mask = None
        if isinstance(boxes, tuple):
            boxes, mask = boxes
        b = np.asarray(boxes, dtype=np.float64)
        if b.ndim == 3 and b.shape[1:] == (5, 2):
            b = b[:, :4]
        if b.ndim != 3 or b.shape[1:] != (4, 2):
            raise ValueError(f"scene {g} track {i}: boxes are (T_obs, 4 (or 5, closed), 2), got {b.shape}")
        valid = ~np.isnan(b).all(axis=(1, 2)) if mask is None else np.asarray(mask, dtype=bool)
        if valid.shape != (b.shape[0],):
            raise ValueError(f"scene {g} track {i}: the mask has shape {valid.shape} for {b.shape[0]} times")
        if t_obs is None:
            t_obs = b.shape[0]
        elif t_obs != b.shape[0]:
            raise ValueError(f"scene {g} track {i}: {b.shape[0]} times, the tracks before it {t_obs}")
        if token in seen:
            raise ValueError(f"scene {g} track {i}: duplicate token {token!r}")
        seen.add(token)
        if token in collided:
            continue
        if RED_LIGHT_TOKEN in token:
            if valid.any():
                stops.append((token, _ring(b[int(np.argmax(valid))], f"scene {g} token {token!r}")))
            continue
        tracks.append((token, np.where(valid[:, None, None], b, 0.0), valid, float(heading), float(speed)))
    for i, ring in enumerate(rings):
        stops.append((f"{RED_LIGHT_TOKEN}_{i}", _ring(ring, f"scene {g} stop polygon {i}")))
    return tracks, stops, t_obs


def pack_lead_objects(observations: Sequence, device, stop_polygons: Optional[Sequence] = None,
                      collided: Optional[Sequence] = None) -> PackedLeadObjects:
    """What the proposal generator reads of G scenes' observations -> the flat tensors ``dd_proposals`` reads. One
    entry per scene: the list form ``pack_observations`` takes with a speed per track, ``(token, boxes, heading,
    is_agent, is_stopped, speed)`` - ``speed`` is ``velocity.magnitude()``, 0 for an object that is no nuPlan Agent -
    with ``stop_polygons[g]`` the scene's red-light polygons as (n, 2) rings (closing edge implied) and
    ``collided[g]`` its ``collided_track_ids``; or a duck-typed ``PDMObservation``, read as ``pack_observations`` reads
    it (map t for time t). Tokens in the collided ids are DROPPED: the generator skips them. Tokens containing
    "red_light" are KEPT, as stop polygons (their shape at the first time they appear: they are static). Raises
    ``ValueError`` on what ``pack_observations`` rejects, with 41 in place of 50 times, and on a ring of fewer than 3
    vertices or with a non-finite vertex."""
    boxes, valid, heading, speed, off, tokens = [], [], [], [], [0], []
    verts, ring_off, scene_ring_off = [], [0], [0]
    t_obs = None
    for g, entry in enumerate(observations):
        duck = hasattr(entry, "_occupancy_maps")
        rings = [] if duck or stop_polygons is None else stop_polygons[g]
        skip = set() if duck or collided is None else set(collided[g])
        tracks, stops, t_scene = _scene_lead_objects(entry, g, rings, skip)
        if t_scene is not None:
            if t_scene < MIN_LEAD_TIMES:
                raise ValueError(f"scene {g}: T_obs = {t_scene} is below {MIN_LEAD_TIMES} (the update at 40 reads map 40)")
            if t_obs is not None and t_obs != t_scene:
                raise ValueError(f"scene {g}: T_obs = {t_scene}, the scenes before it {t_obs}")
            t_obs = t_scene
        names = []
        for token, b, v, h, sp in tracks:
            if not np.isfinite(b[v]).all():
                raise ValueError(f"scene {g} token {token!r}: non-finite box where the object is present")
            if not np.isfinite(h) or not np.isfinite(sp):
                raise ValueError(f"scene {g} token {token!r}: non-finite heading or speed")
            boxes.append(b), valid.append(v), heading.append(h), speed.append(sp), names.append(token)
        off.append(len(heading))
        for token, ring in stops:
            verts.append(ring), names.append(token)
            ring_off.append(ring_off[-1] + ring.shape[0])
        scene_ring_off.append(len(ring_off) - 1)
        tokens.append(tuple(names))
    t_obs = t_obs if t_obs is not None else MIN_LEAD_TIMES
    k = len(heading)
    if k * t_obs * 8 >= 2 ** 31 or ring_off[-1] * 2 >= 2 ** 31:
        raise ValueError(f"{k} tracks x {t_obs} times or {ring_off[-1]} ring vertices do not fit the int32 offsets")
    dev = torch.device(device)
    b = np.stack(boxes) if k else np.zeros((0, t_obs, 4, 2))
    v = np.stack(valid).astype(np.uint8) if k else np.zeros((0, t_obs), dtype=np.uint8)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    return PackedLeadObjects(f64(b), torch.from_numpy(v).to(dev), f64(heading), f64(speed), i32(off),
                             f64(np.concatenate(verts) if verts else np.zeros((0, 2))), i32(ring_off),
                             i32(scene_ring_off), tuple(tokens))


def default_idm_params(lib=None) -> _lib.DDIdmParams:
    """``dd_default_idm_params``: min gap 1 m, headway 1.5 s, acceleration 1.5 and deceleration 3 m/s^2, dt 0.1 s, the
    exponent 10, the leader update every 2 steps, a corridor of 50 poses (metric_cache_processor.py:44-59)."""
    p = _lib.DDIdmParams()
    (lib or _lib.load()).dd_default_idm_params(ctypes.byref(p))
    return p


def _idm_params(params: Union[None, _lib.DDIdmParams, Mapping], lib) -> _lib.DDIdmParams:
    if isinstance(params, _lib.DDIdmParams):
        return params
    p = default_idm_params(lib)
    for k, v in (params or {}).items():
        if k not in dict(p._fields_):
            raise ValueError(f"unknown IDM parameter {k!r}")
        setattr(p, k, v)
    return p


def generate_proposals(paths, lead_objects, ego_states: torch.Tensor, target_velocities, params=None,
                       details: bool = False, stream: Optional[torch.cuda.Stream] = None, area_params=None,
                       device=None) -> Proposals:
    """``PDMGenerator.generate_proposals`` (pdm_generator.py:68-95) on the device. ``paths``: ``pack_paths``' result for
    the G scenes (or what it takes: packed here); ``lead_objects``: ``pack_lead_objects``' result (or a sequence of
    duck-typed ``PDMObservation``: packed here); ``ego_states`` (G, 11) float64 start states; ``target_velocities``
    (G, L): the target velocity of each of the L <= 64 IDM policies per scene (``speed_limit_fraction * speed_limit``,
    or the fallback) - a host array is checked (positive, finite) and moved; a device tensor is trusted. Returns a
    ``Proposals``: ``proposals`` (G, P L, 41, 3) float64 in ``PDMProposalManager``'s order (lateral-major), which is
    what ``simulate_proposals`` takes flattened; with ``details`` also the IDM states, the leader rows and the leader's
    object index. ``params``: a ``DDIdmParams`` or a mapping of overrides; ``area_params`` gives the vehicle's width
    and length. The device is ``paths``' if packed, else ``lead_objects``', else ``ego_states``', else ``device``. A
    bad argument raises ``ValueError`` with ``dd_last_error()``'s text."""
    lib = _lib.load()
    dev = None
    for t in (paths.verts if isinstance(paths, PackedPaths) else None,
              lead_objects.boxes if isinstance(lead_objects, PackedLeadObjects) else None,
              ego_states if isinstance(ego_states, torch.Tensor) else None,
              target_velocities if isinstance(target_velocities, torch.Tensor) else None):
        if t is not None and t.device.type == "cuda":
            dev = t.device
            break
    if dev is None:
        dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(paths, PackedPaths):
        paths = pack_paths(paths, dev)
    if not isinstance(lead_objects, PackedLeadObjects):
        lead_objects = pack_lead_objects(lead_objects, dev)
    for name, t, dt in (("paths.verts", paths.verts, torch.float64), ("paths.progress", paths.progress, torch.float64),
                        ("paths.path_off", paths.path_off, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor on {dev}")
    _fields_on(PackedLeadObjects(*lead_objects[:8], ()),
               (torch.float64, torch.uint8, torch.float64, torch.float64, torch.int32, torch.float64, torch.int32,
                torch.int32), dev, "lead_objects")
    ego = _ego(ego_states, dev)
    scenes = int(ego.shape[0])
    per_scene = int(paths.paths_per_scene)
    if per_scene < 1 or int(paths.path_off.numel()) != scenes * per_scene + 1:
        raise ValueError(f"paths holds {int(paths.path_off.numel()) - 1} paths, {per_scene} per scene, for {scenes} "
                         "scenes (the rows of ego_states)")
    if int(lead_objects.scene_track_off.numel()) != scenes + 1 or int(lead_objects.scene_ring_off.numel()) != scenes + 1:
        raise ValueError(f"lead_objects holds {int(lead_objects.scene_track_off.numel()) - 1} scenes for {scenes} (the "
                         "rows of ego_states)")
    k = int(lead_objects.heading.numel())
    b = lead_objects.boxes
    if b.dim() != 4 or tuple(b.shape[2:]) != (4, 2) or b.shape[0] != k or tuple(lead_objects.valid.shape) != \
            (k, b.shape[1]) or int(lead_objects.speed.numel()) != k or int(lead_objects.stop_verts.numel()) % 2:
        raise ValueError("lead_objects is not what pack_lead_objects returns: boxes / valid / speed do not fit heading")
    rings = int(lead_objects.ring_off.numel()) - 1
    host = None
    if isinstance(target_velocities, torch.Tensor) and target_velocities.device.type == "cuda":
        targets = target_velocities
    else:
        host = np.ascontiguousarray(np.asarray(target_velocities, dtype=np.float64))
        targets = torch.from_numpy(host)
    if targets.dtype != torch.float64 or targets.dim() != 2 or targets.shape[0] != scenes:
        raise ValueError(f"target_velocities must be float64 ({scenes}, L), got {tuple(targets.shape)} {targets.dtype}")
    policies = int(targets.shape[1])
    targets = targets.to(dev).contiguous()
    p, ap = _idm_params(params, lib), _area_params(area_params, lib)
    pp = _lib.DDPaths(paths.verts.data_ptr() or None, paths.progress.data_ptr() or None,
                      paths.path_off.data_ptr() or None, per_scene, int(paths.progress.numel()))
    lo = _lib.DDLeadObjects(b.data_ptr() or None, lead_objects.valid.data_ptr() or None,
                            lead_objects.heading.data_ptr() or None, lead_objects.speed.data_ptr() or None,
                            lead_objects.scene_track_off.data_ptr() or None, k, int(b.shape[1]),
                            lead_objects.stop_verts.data_ptr() or None, lead_objects.ring_off.data_ptr() or None,
                            lead_objects.scene_ring_off.data_ptr() or None, rings)
    n = scenes * per_scene * policies
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):  # the outputs and the scratch belong to the stream that runs
        out = torch.empty((scenes, per_scene * policies, NUM_STATES, 3), dtype=torch.float64, device=dev)
        idm = torch.empty((scenes, per_scene * policies, NUM_STATES, 2), dtype=torch.float64, device=dev) if details else None
        lead = torch.empty((scenes, per_scene * policies, NUM_STATES, 3), dtype=torch.float64, device=dev) if details else None
        index = torch.empty((scenes, per_scene * policies, NUM_STATES), dtype=torch.int32, device=dev) if details else None
        size = lib.dd_proposals_work(scenes, per_scene, k, rings)
        work = torch.empty((size,), dtype=torch.float64, device=dev)
        rc = lib.dd_proposals(ctypes.byref(pp), ctypes.byref(lo), ego.data_ptr(), targets.data_ptr() or None,
                              host.ctypes.data if host is not None and host.size else None, scenes, policies,
                              ctypes.byref(p), ctypes.byref(ap), work.data_ptr(), size, out.data_ptr() if n else None,
                              idm.data_ptr() if details and n else None, lead.data_ptr() if details and n else None,
                              index.data_ptr() if details and n else None, s.cuda_stream)
    _raise(rc, lib)
    return Proposals(out, idm, lead, index)


def select_best(scores: PDMScores, states: torch.Tensor, stream: Optional[torch.cuda.Stream] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``dd_pdm_select``: per scene np.argmax of ``scores.score`` (G, n) - the first maximum - as int32 (G), that
    candidate's states (G, 41, 11) and its ``raw_progress * no_collision * drivable_area`` (G)."""
    lib = _lib.load()
    states, lead, n = _states_arg(states, 1)
    dev = states.device
    if len(lead) != 2:
        raise ValueError(f"states must be (G, n, {NUM_STATES}, {STATE_SIZE}), got {tuple(states.shape)}")
    ins = []
    for name in ("score", "raw_progress", "no_collision", "drivable_area"):
        t = getattr(scores, name)
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float64 or tuple(t.shape) != lead:
            raise ValueError(f"scores.{name} must be a float64 {lead} tensor on {dev}")
        ins.append(t.contiguous())
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        index = torch.empty((lead[0],), dtype=torch.int32, device=dev)
        best = torch.empty((lead[0], NUM_STATES, STATE_SIZE), dtype=torch.float64, device=dev)
        reference = torch.empty((lead[0],), dtype=torch.float64, device=dev)
        rc = lib.dd_pdm_select(*(t.data_ptr() for t in ins), states.data_ptr(), n, lead[1] if lead[0] else 0,
                               index.data_ptr(), best.data_ptr(), reference.data_ptr(), s.cuda_stream)
    _raise(rc, lib)
    return index, best, reference


def pdm_closed(paths, lead_objects, ego_states: torch.Tensor, target_velocities, maps, observations, centerlines, *,
               idm_params=None, sim_params=None, comfort_params=None, area_params=None, score_params=None,
               stream: Optional[torch.cuda.Stream] = None, device=None) -> PDMClosed:
    """The PDM-Closed planner's candidate stage on one stream, nothing leaving the device: ``generate_proposals`` ->
    ``simulate_proposals`` -> ``pdm_score`` (the scene's P L proposals normalised as a group, ``score_proposals``'
    rule) -> per scene the first maximum (``dd_pdm_select``). ``maps``, ``observations`` and ``centerlines`` are what
    ``pdm_score`` takes. Returns a ``PDMClosed``: the scores of all proposals, the best index, the best proposal's
    simulated states, and ``progress_reference`` (G) - the best proposal's ``raw_progress * no_collision *
    drivable_area``, the value ``pdm_score(progress_reference=)`` needs to score a planner's candidates as pairs with
    the PDM-Closed trajectory (navsim/evaluate/pdm_score.py)."""
    made = generate_proposals(paths, lead_objects, ego_states, target_velocities, idm_params, stream=stream,
                              area_params=area_params, device=device)
    dev = made.proposals.device
    s = stream or torch.cuda.current_stream(dev)
    scenes, per = int(made.proposals.shape[0]), int(made.proposals.shape[1])
    with torch.cuda.device(dev), torch.cuda.stream(s):
        states = simulate_proposals(made.proposals.view(scenes * per, NUM_STATES, 3), _ego(ego_states, dev), sim_params,
                                    per_group=per, stream=s).view(scenes, per, NUM_STATES, STATE_SIZE)
        scores = pdm_score(states, maps, observations, centerlines, comfort_params=comfort_params,
                           area_params=area_params, score_params=score_params, stream=s)
        index, best, reference = select_best(scores, states, stream=s)
    return PDMClosed(scores, index, best, reference, made.proposals, states)


# ---- PDM's forecasted observation from raw detections (dd_observe) and the agent head's detections

DET_VEHICLE, DET_PEDESTRIAN, DET_BICYCLE, DET_STATIC, DET_SKIP = 0, 1, 2, 3, 255   # dd_detections.type
# nuPlan's TrackedObjectType names, quoted from memory (include/ddmi.h): the three AGENT_TYPES, the static types, EGO
DETECTION_TYPE_NAMES = {"VEHICLE": DET_VEHICLE, "PEDESTRIAN": DET_PEDESTRIAN, "BICYCLE": DET_BICYCLE,
                        "TRAFFIC_CONE": DET_STATIC, "BARRIER": DET_STATIC, "CZONE_SIGN": DET_STATIC,
                        "GENERIC_OBJECT": DET_STATIC, "EGO": DET_SKIP}
NUM_AGENT_BOXES = 30   # the agent head's boxes per scene (transfuser_config.py: num_bounding_boxes)


class PackedDetections(NamedTuple):
    """``dd_detections``: the raw detections of G scenes as flat device tensors (include/ddmi.h)."""
    boxes: torch.Tensor           # float64 (D, 7): center x, y, heading, length, width, velocity x, y
    type: torch.Tensor            # uint8 (D): 0 VEHICLE, 1 PEDESTRIAN, 2 BICYCLE, 3 static, 255 EGO / skip
    scene_det_off: torch.Tensor   # int32 (G + 1)
    tokens: Tuple[Tuple[str, ...], ...]   # per scene, the detections' tokens in order (host only)


class Observed(NamedTuple):
    """``observe``'s result: the same device tensors seen as what the scorer and the generator take."""
    observations: PackedObservations    # for pdm_score / collisions / pdm_closed; its ``tokens`` is ()
    lead_objects: PackedLeadObjects     # for generate_proposals / pdm_closed; its ``tokens`` is ()
    order: torch.Tensor                 # int32 (K = D): the detection index each slot holds
    collided: torch.Tensor              # uint8 (D), detection order: what the next call's ``collided`` takes
    detection_tokens: Tuple[Tuple[str, ...], ...]   # the detections' tokens (host only)
    ring_tokens: Tuple[Tuple[str, ...], ...]        # per scene, the names of the stop polygons that were packed
    ignored_rings: Tuple[Tuple[str, ...], ...]      # per scene, the names of the stop polygons that hold the ego quad

    def tokens(self) -> Tuple[Tuple[str, ...], ...]:
        """Per scene, the token of every slot in order, then the packed stop polygons' names: the object order
        ``Proposals.lead_index`` counts in. Reads ``order`` back: the one device read of the stage."""
        order = self.order.cpu().numpy()
        flat = [t for scene in self.detection_tokens for t in scene]
        out, k = [], 0
        for scene, rings in zip(self.detection_tokens, self.ring_tokens):
            out.append(tuple(flat[int(d)] for d in order[k:k + len(scene)]) + tuple(rings))
            k += len(scene)
        return tuple(out)


def _detection_rows(entry, g):
    """One scene's detections as (token, x, y, heading, length, width, vx, vy, type_name) tuples."""
    for _ in range(2):   # DetectionsTracks.tracked_objects is a TrackedObjects, whose .tracked_objects is the list
        entry = getattr(entry, "tracked_objects", entry)
    rows = []
    for i, item in enumerate(entry):
        if hasattr(item, "track_token"):
            velocity = getattr(item, "velocity", None)   # a static object has none
            rows.append((item.track_token, item.center.x, item.center.y, item.center.heading, item.box.length,
                         item.box.width, 0.0 if velocity is None else velocity.x,
                         0.0 if velocity is None else velocity.y, item.tracked_object_type.name))
            continue
        try:
            token, x, y, heading, length, width, vx, vy, type_name = item
        except (TypeError, ValueError):
            raise ValueError(f"scene {g} detection {i}: expected (token, x, y, heading, length, width, vx, vy, "
                             "type_name) or a TrackedObject") from None
        rows.append((token, x, y, heading, length, width, vx, vy, type_name))
    return rows


def pack_detections(scenes: Sequence, device) -> PackedDetections:
    """The raw detections of G scenes -> the flat tensors ``dd_observe`` reads, on ``device``. One entry per scene: a
    list of ``(token, x, y, heading, length, width, vx, vy, type_name)`` - the box's center pose and size, the
    velocity (0, 0 for a static object) and nuPlan's ``TrackedObjectType`` name - or a duck-typed ``DetectionsTracks``
    / list of ``TrackedObject``, read only through ``track_token``, ``center.x`` / ``.y`` / ``.heading``,
    ``box.length`` / ``.width``, ``velocity.x`` / ``.y`` where present and ``tracked_object_type.name``. Raises
    ``ValueError`` on a non-finite value, a non-positive length or width, a duplicate token within a scene or an
    unknown type name: the device trusts these arrays."""
    boxes, types, off, tokens = [], [], [0], []
    for g, entry in enumerate(scenes):
        names = []
        seen = set()
        for i, (token, *figures, type_name) in enumerate(_detection_rows(entry, g)):
            if type_name not in DETECTION_TYPE_NAMES:
                raise ValueError(f"scene {g} detection {i} ({token!r}): unknown type name {type_name!r}")
            row = np.asarray(figures, dtype=np.float64)
            if not np.isfinite(row).all():
                raise ValueError(f"scene {g} detection {i} ({token!r}): non-finite value")
            if not (row[3] > 0.0 and row[4] > 0.0):
                raise ValueError(f"scene {g} detection {i} ({token!r}): non-positive length or width")
            if token in seen:
                raise ValueError(f"scene {g} detection {i}: duplicate token {token!r}")
            seen.add(token)
            boxes.append(row), types.append(DETECTION_TYPE_NAMES[type_name]), names.append(token)
        off.append(len(types))
        tokens.append(tuple(names))
    dev = torch.device(device)
    b = np.stack(boxes) if boxes else np.zeros((0, 7))
    return PackedDetections(torch.from_numpy(np.ascontiguousarray(b)).to(dev),
                            torch.from_numpy(np.asarray(types, dtype=np.uint8)).to(dev),
                            torch.from_numpy(np.asarray(off, dtype=np.int32)).to(dev), tuple(tokens))


def default_observe_params(lib=None) -> _lib.DDObserveParams:
    """``dd_default_observe_params``: the radius 100 m, dt 0.1 s, 50 samples at resolution 2 (T_obs = 52), the caps 50
    vehicles / 25 pedestrians / 10 bicycles / 50 static objects, the stopped speed 5e-2 m/s."""
    p = _lib.DDObserveParams()
    (lib or _lib.load()).dd_default_observe_params(ctypes.byref(p))
    return p


def _observe_params(params: Union[None, _lib.DDObserveParams, Mapping], lib) -> _lib.DDObserveParams:
    if isinstance(params, _lib.DDObserveParams):
        return params
    p = default_observe_params(lib)
    for k, v in (params or {}).items():
        if k not in dict(p._fields_):
            raise ValueError(f"unknown observe parameter {k!r}")
        setattr(p, k, v)
    return p


def ego_quad(pose, half_length: float, half_width: float, rear_axle_to_center: float) -> np.ndarray:
    """The ego quad (4, 2) of a rear-axle pose (x, y, heading) by ``dd_ego_areas``' corner formulas, on the host."""
    x, y, h = (float(v) for v in pose)
    cos, sin = np.cos(h), np.sin(h)
    cx, cy = x + rear_axle_to_center * cos, y + rear_axle_to_center * sin
    cq, sq = np.cos(h + np.pi / 2.0), np.sin(h + np.pi / 2.0)
    return np.array([[cx + ((lat * cq) + (lon * cos)), cy + ((lat * sq) + (lon * sin))]
                     for lon, lat in ((half_length, half_width), (-half_length, half_width),
                                      (-half_length, -half_width), (half_length, -half_width))])


def ring_holds_quad(ring, quad) -> bool:
    """The rule by which ``observe`` ignores a red light (pdm_observation.py:196-201, ``ego_polygon.within(light)``):
    all four corners of the quad lie strictly inside the ring (the even-odd crossing count of ``dd_ego_areas``, on
    differences against the corner: a corner on the ring is outside) and no edge of the ring meets an edge of the quad
    (closed: touching counts as meeting). A ring that only touches or cuts the quad, or lies apart from it, is kept."""
    v = _ring(ring, "stop polygon")
    q = np.asarray(quad, dtype=np.float64)
    w = np.roll(v, -1, axis=0)
    for px, py in q:
        a, b, c, d = v[:, 0] - px, v[:, 1] - py, w[:, 0] - px, w[:, 1] - py
        cross = (c - a) * (0.0 - b) - (0.0 - a) * (d - b)
        on_edge = (cross == 0.0) & (np.minimum(a, c) <= 0.0) & (np.maximum(a, c) >= 0.0) \
            & (np.minimum(b, d) <= 0.0) & (np.maximum(b, d) >= 0.0)
        flips = ((b > 0.0) != (d > 0.0)) & np.where(d > b, cross > 0.0, cross < 0.0)
        if on_edge.any() or not (int(flips.sum()) & 1):
            return False

    def side(ox, oy, ax, ay, bx, by):   # the orientation of (b - o) against (a - o), on differences
        return np.sign((ax - ox) * (by - oy) - (ay - oy) * (bx - ox))

    for i in range(4):
        p0, p1 = q[i], q[(i + 1) % 4]
        for e0, e1 in zip(v, w):
            d1, d2 = side(*p0, *p1, *e0), side(*p0, *p1, *e1)
            d3, d4 = side(*e0, *e1, *p0), side(*e0, *e1, *p1)
            if d1 * d2 < 0 and d3 * d4 < 0:
                return False
            if 0 in (d1, d2, d3, d4):   # collinear somewhere: met if the bounding boxes of the two edges overlap
                if (max(min(p0[0], p1[0]), min(e0[0], e1[0])) <= min(max(p0[0], p1[0]), max(e0[0], e1[0]))
                        and max(min(p0[1], p1[1]), min(e0[1], e1[1])) <= min(max(p0[1], p1[1]), max(e0[1], e1[1]))
                        and d1 * d2 <= 0 and d3 * d4 <= 0):
                    return False
    return True


def split_stop_polygons(stop_polygons: Sequence, ego_states, half_length: float, half_width: float,
                        rear_axle_to_center: float):
    """Per scene the stop polygons ``observe`` packs and the names of those it ignores (``ring_holds_quad``). The ring
    ``i`` of a scene is named ``red_light_<i>``, as ``pack_lead_objects`` names it; a kept ring keeps its name.
    ``ego_states``: host (G, >= 3) rear-axle poses."""
    ego = np.asarray(ego_states, dtype=np.float64)
    kept, names, ignored = [], [], []
    for g, rings in enumerate(stop_polygons):
        quad = ego_quad(ego[g, :3], half_length, half_width, rear_axle_to_center)
        kept.append([]), names.append([]), ignored.append([])
        for i, ring in enumerate(rings):
            name = f"{RED_LIGHT_TOKEN}_{i}"
            if ring_holds_quad(ring, quad):
                ignored[-1].append(name)
            else:
                kept[-1].append(_ring(ring, f"scene {g} stop polygon {i}")), names[-1].append(name)
    return kept, tuple(tuple(n) for n in names), tuple(tuple(n) for n in ignored)


def observe(detections, ego_states: torch.Tensor, *, collided: Optional[torch.Tensor] = None,
            stop_polygons: Optional[Sequence] = None, params=None, area_params=None,
            stream: Optional[torch.cuda.Stream] = None, device=None) -> Observed:
    """``PDMObservation.update`` with ``PDMObjectManager`` (pdm_observation.py:105-205) on the device: from the current
    detections and the ego states (G, 11) to the forecasted observation the scorer and the generator read. The ego, far
    (``map_radius``) and previously collided objects are dropped; the nearest 50 static objects, 50 vehicles, 25
    pedestrians and 10 bicycles are kept; every kept agent is forecast at constant velocity along its own axis on a
    0.2 s grid for 5.2 s; what already overlaps the ego quad is recorded in ``collided`` and is valid at no time
    (include/ddmi.h has the rules at length). ``detections``: ``pack_detections``' or
    ``detections_from_agent_head``'s result (or what ``pack_detections`` takes: packed here). ``collided``: the
    ``Observed.collided`` of the call before on the same detections, or None. ``stop_polygons[g]``: the scene's
    red-light rings, host data as ``pack_lead_objects`` takes them; a ring that holds the whole ego quad
    (``ring_holds_quad``) is ignored, as the reference ignores such a light from then on, and named in
    ``ignored_rings`` - with stop polygons the ego poses are read back to the host for that test. ``params``: a
    ``DDObserveParams`` or a mapping of overrides of ``default_observe_params()``. Scene g's tracks are its
    detections' slots: K = D, a dropped detection is a track valid at no time, and no count returns to the host.
    Returns an ``Observed``; both packed results share their tensors and go into ``pdm_score``, ``collisions``,
    ``generate_proposals`` and ``pdm_closed`` as they are. A bad argument raises ``ValueError`` with
    ``dd_last_error()``'s text."""
    lib = _lib.load()
    dev = None
    for t in (detections.boxes if isinstance(detections, PackedDetections) else None,
              ego_states if isinstance(ego_states, torch.Tensor) else None):
        if t is not None and t.device.type == "cuda":
            dev = t.device
            break
    if dev is None:
        dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(detections, PackedDetections):
        detections = pack_detections(detections, dev)
    _fields_on(detections, (torch.float64, torch.uint8, torch.int32), dev, "detections")
    ego = _ego(ego_states, dev)
    scenes = int(ego.shape[0])
    d = int(detections.type.numel())
    if int(detections.scene_det_off.numel()) != scenes + 1:
        raise ValueError(f"detections hold {int(detections.scene_det_off.numel()) - 1} scenes for {scenes} (the rows of "
                         "ego_states)")
    if tuple(detections.boxes.shape) != (d, 7):
        raise ValueError(f"detections.boxes must be ({d}, 7), got {tuple(detections.boxes.shape)}")
    if collided is not None and (not isinstance(collided, torch.Tensor) or collided.device != dev
                                 or collided.dtype != torch.uint8 or tuple(collided.shape) != (d,)
                                 or not collided.is_contiguous()):
        raise ValueError(f"collided must be a contiguous uint8 ({d},) tensor on {dev} (an Observed.collided)")
    p, ap = _observe_params(params, lib), _area_params(area_params, lib)
    t_obs = int(p.num_samples) + int(p.sample_res)
    kept_rings = [[] for _ in range(scenes)]
    ring_names = ignored = tuple(() for _ in range(scenes))
    if stop_polygons is not None:
        if len(stop_polygons) != scenes:
            raise ValueError(f"stop_polygons holds {len(stop_polygons)} scenes for {scenes}")
        kept_rings, ring_names, ignored = split_stop_polygons(stop_polygons, ego[:, :3].cpu().numpy(), ap.half_length,
                                                              ap.half_width, ap.rear_axle_to_center)
    verts, ring_off, scene_ring_off = [], [0], [0]
    for rings in kept_rings:
        for ring in rings:
            verts.append(ring)
            ring_off.append(ring_off[-1] + ring.shape[0])
        scene_ring_off.append(len(ring_off) - 1)
    det = _lib.DDDetections(detections.boxes.data_ptr() or None, detections.type.data_ptr() or None,
                            detections.scene_det_off.data_ptr() or None,
                            collided.data_ptr() or None if collided is not None else None, d)
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):  # the outputs and the scratch belong to the stream that runs
        boxes = torch.empty((d, max(t_obs, 0), 4, 2), dtype=torch.float64, device=dev)
        valid = torch.empty((d, max(t_obs, 0)), dtype=torch.uint8, device=dev)
        heading = torch.empty((d,), dtype=torch.float64, device=dev)
        speed = torch.empty((d,), dtype=torch.float64, device=dev)
        flags = torch.empty((d,), dtype=torch.uint8, device=dev)
        order = torch.empty((d,), dtype=torch.int32, device=dev)
        out_collided = torch.empty((d,), dtype=torch.uint8, device=dev)
        work = torch.empty((lib.dd_observe_work(d),), dtype=torch.float64, device=dev)
        rc = lib.dd_observe(ctypes.byref(det), ego.data_ptr(), scenes, ctypes.byref(p), ctypes.byref(ap),
                            work.data_ptr(), boxes.data_ptr() or None, valid.data_ptr() or None,
                            heading.data_ptr() or None, speed.data_ptr() or None, flags.data_ptr() or None,
                            order.data_ptr() or None, out_collided.data_ptr() or None, s.cuda_stream)
        _raise(rc, lib)
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
        i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)  # noqa: E731
        stop_verts = f64(np.concatenate(verts) if verts else np.zeros((0, 2)))
        rings_dev, scene_rings_dev = i32(ring_off), i32(scene_ring_off)
    off = detections.scene_det_off
    return Observed(PackedObservations(boxes, valid, heading, flags, off, ()),
                    PackedLeadObjects(boxes, valid, heading, speed, off, stop_verts, rings_dev, scene_rings_dev, ()),
                    order, out_collided, detections.tokens, ring_names, ignored)


def detections_from_agent_head(agent_states: torch.Tensor, agent_labels: torch.Tensor, ego_states: torch.Tensor,
                               threshold: float = 0.0, stream: Optional[torch.cuda.Stream] = None) -> PackedDetections:
    """``dd_detections_from_agents``: the planner's own agent head as detections. ``agent_states`` device float32
    (B, A, 5) - ego-frame x, y, heading, length, width (transfuser_features.py:192-204) - and ``agent_labels`` float32
    (B, A) logits, exactly what a forward writes, read in place; ``ego_states`` (B, 11) float64. A box is a VEHICLE
    where its logit exceeds ``threshold`` (0 = the callback's ``sigmoid() > 0.5``), its length and width are positive
    and every value is finite; any other row is zeroed and skipped. The center is the rear-axle pose composed with
    (x, y), the heading the ego's plus the box's, the velocity 0: such a track is flagged stopped and forecast in
    place. The tokens are ``agent_<a>``."""
    lib = _lib.load()
    if not isinstance(agent_states, torch.Tensor) or agent_states.device.type != "cuda":
        raise ValueError("agent_states must be a device tensor (a forward's agent_states)")
    dev = agent_states.device
    if agent_states.dtype != torch.float32 or agent_states.dim() != 3 or agent_states.shape[2] != 5:
        raise ValueError(f"agent_states must be float32 (B, A, 5), got {tuple(agent_states.shape)} {agent_states.dtype}")
    b, a = int(agent_states.shape[0]), int(agent_states.shape[1])
    if not isinstance(agent_labels, torch.Tensor) or agent_labels.device != dev or agent_labels.dtype != torch.float32 \
            or tuple(agent_labels.shape) != (b, a):
        raise ValueError(f"agent_labels must be a float32 ({b}, {a}) tensor on {dev}")
    agent_states, agent_labels = agent_states.contiguous(), agent_labels.contiguous()
    ego = _ego(ego_states, dev)
    if int(ego.shape[0]) != b:
        raise ValueError(f"ego_states holds {int(ego.shape[0])} scenes for {b} (the first dimension of agent_states)")
    s = stream or torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        boxes = torch.empty((b * a, 7), dtype=torch.float64, device=dev)
        types = torch.empty((b * a,), dtype=torch.uint8, device=dev)
        off = torch.empty((b + 1,), dtype=torch.int32, device=dev)
        rc = lib.dd_detections_from_agents(agent_states.data_ptr() or None, agent_labels.data_ptr() or None,
                                           ego.data_ptr() or None, b, a, float(threshold), boxes.data_ptr() or None,
                                           types.data_ptr() or None, off.data_ptr(), s.cuda_stream)
    _raise(rc, lib)
    return PackedDetections(boxes, types, off, tuple(tuple(f"agent_{i}" for i in range(a)) for _ in range(b)))
