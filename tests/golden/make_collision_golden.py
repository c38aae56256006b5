#!/usr/bin/env python3
"""Golden vectors of the whole PDM score - no-at-fault collision, TTC, progress, aggregation - from the REFERENCE's
PDMScorer run unmodified (build container only: it needs the reference tree and scipy).

shapely and nuPlan are not available and ``refshim`` stubs them. Before the reference is imported, real stand-ins are
registered where the stub finder would hand out stubs: ``StateSE2``, ``CollisionType`` and a tracked-object-type Enum
with ``AGENT_TYPES``, ``SemanticMapLayer``, the three idm.utils predicates (quoted from memory of nuPlan: include/ddmi.h)
and small duck classes for ``shapely.Point`` / ``LineString`` / ``Polygon`` / ``creation.polygons``. Then ``_reset``,
``_calculate_ego_area``, ``_calculate_no_at_fault_collision`` (with ``get_collision_type`` as imported),
``_calculate_drivable_area_compliance``, ``_calculate_driving_direction_compliance``, ``_calculate_progress``,
``_calculate_ttc``, ``_calculate_is_comfortable`` and ``_aggregate_scores`` run as they are on duck-typed inputs: an
observation of occupancy maps with ``query``, a centerline with ``project``, make_area_golden's map with
``is_in_layer``. After ``_reset`` the ego polygons are set from ``_ego_coords`` explicitly.

Only the geometric primitives stand in for shapely (tests/pdm_collision_ref.py): closed quad - quad and segment - quad
intersection, the quad centroid, strict point-in-polygon, the polyline projection. Each is checked here on EVERY use
against an independent predicate that shares no code with it (vertex containment by half-plane signs and proper edge
crossings, behind a bounding-circle test; the corner mean; half-plane containment; dense sampling of the polyline).
The reference does not keep the collision type of a hit: the ``get_collision_type`` the scorer module imported is
wrapped to count what it returns (every classified hit), and the deciding first hits are counted by the restatement
over the reference's own flags.

Inputs: the ``states`` of the three committed pdm_sim_s3_*.npz sets (keyed by name, not stored again) on the seeded
maps of pdm_area_ref.seeded_map (the ``global`` set at 6.6e5 / 4.0e6 m), with seeded tracks laid around each set's
paths (pdm_collision_ref.seeded_tracks: moving and stopped vehicles, a pedestrian, a static non-agent object, a track
absent for part of the horizon, a red-light token, a previously collided token) and a seeded centerline; the synthetic
states of pdm_area_ref (their velocities set along their headings); one row with a NaN pose; the first 24 rows of
the ``moving`` set under non-default parameters (pdm_area_ref.ALT and pdm_collision_ref.SCORE_ALT; get_collision_type's stopped-speed
default is replaced through ``__defaults__``, the only way to pass it); the ``moving`` set again as pairs [candidate 0,
candidate i] (the rule of navsim/evaluate/pdm_score.py). Tracks, maps and centerlines are rebuilt by the tests from
the recorded seed.

Asserted, a failing seed being replaced by the next and no candidate excluded: every separating-axis gap or
penetration of every tested quad pair and bumper segment >= 1e-6 m; every finite speed >= 1e-6 from both stopped
thresholds; every used relative angle >= 1e-9 rad from both bounds and its cosine at least 1e-12 inside [-1, 1]; every
tested rear-axle point >= 1e-6 m from every INTERSECTION edge; for every projected point the two nearest segments
differ by >= 1e-6 m or are adjacent at the nearest vertex; every group's pmax >= 1e-6 from the threshold; every comfort
signal >= 1e-5 from its bounds; no_collision takes all of {1, 0.5, 0} and ttc both of {1, 0}; all five collision types
decide a first hit; both progress branches occur; a score differs between group and pair normalisation.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_collision_golden.py [seed]
Writes tests/golden/pdm_score_s{seed}.npz. Only data is stored; nothing of the reference's source.
"""
import enum
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_area_golden as MA  # noqa: E402
import pdm_area_ref as A  # noqa: E402
import pdm_collision_ref as R  # noqa: E402
import pdm_comfort_ref as C  # noqa: E402

SEED = 5
MARGIN = 1e-6
ANGLE_MARGIN = 1e-9
COMFORT_MARGIN = 1e-5
SIM_SETS = MA.SIM_SETS
ALT_ROWS = MA.ALT_ROWS
NAN_ROW, NAN_AT = 5, 17
LOG = dict(gap=np.inf, angle=np.inf, cosine=np.inf, axle=np.inf, tie=np.inf, types=[])
ANGLES = dict(ahead=R.SCORE_DEFAULTS["ahead_angle"], behind=R.SCORE_DEFAULTS["behind_angle"])


# ---- the stand-ins registered before the reference is imported

class Point:
    def __init__(self, x, y):
        self.x, self.y = float(x), float(y)


class Polygon:
    """A quad: ``exterior.coords`` is the closed ring of five points, ``centroid`` the area centroid."""

    def __init__(self, coords):
        c = np.asarray(coords, dtype=np.float64)
        self.quad = c[:4]
        self.exterior = types.SimpleNamespace(coords=np.concatenate([c[:4], c[:1]]))

    @property
    def centroid(self):
        c = R.centroid(self.quad)
        mean = self.quad.mean(0)     # independent: a parallelogram's centroid is its corner mean
        assert np.abs(c - mean).max() <= 1e-9 * max(1.0, np.abs(mean).max()), (c, mean)
        return Point(*c)


def touch_checked(a, b, got, log_gap=True):
    """The independent predicate for one pair (behind a bounding-circle test), and the margin of the pair."""
    if np.isfinite(a).all():
        ca, cb = a.mean(0), b.mean(0)
        apart = np.hypot(*(ca - cb)) > np.hypot(*(a - ca).T).max() + np.hypot(*(b - cb).T).max()
        want = False if apart else R.independent_touch(a, b)
    else:
        want = False
    assert bool(got) == want, ("the separating-axis test and the independent predicate differ", a, b)
    if log_gap:
        LOG["gap"] = min(LOG["gap"], abs(float(R.gap(a, b))))


class LineString:
    def __init__(self, coords):
        self.seg = np.asarray(coords, dtype=np.float64)[:, :2]

    def intersects(self, polygon):
        got = bool(R.segment_touches(self.seg, polygon.quad))
        touch_checked(self.seg, polygon.quad, got)
        return got


def polygons(coords):
    coords = np.asarray(coords)
    out = np.empty(coords.shape[:-2], dtype=object)
    for idx in np.ndindex(*out.shape):
        out[idx] = Polygon(coords[idx])
    return out


class StateSE2:
    def __init__(self, x, y, heading):
        self.x, self.y, self.heading = float(x), float(y), float(heading)

    @property
    def point(self):
        return Point(self.x, self.y)


TrackedObjectType = enum.Enum("TrackedObjectType", ["VEHICLE", "PEDESTRIAN", "BICYCLE", "TRAFFIC_CONE", "BARRIER",
                                                    "CZONE_SIGN", "GENERIC_OBJECT", "EGO"])
AGENT_TYPES = {TrackedObjectType.VEHICLE, TrackedObjectType.PEDESTRIAN, TrackedObjectType.BICYCLE}
CollisionType = enum.IntEnum("CollisionType", list(R.TYPE_NAMES), start=0)


class Agent:
    """What the scorer reads of a nuPlan Agent; a StaticObject is the same without a velocity."""

    def __init__(self, heading, kind, speed):
        self.box = types.SimpleNamespace(center=types.SimpleNamespace(heading=heading))
        self.tracked_object_type = TrackedObjectType[kind]
        self.velocity = types.SimpleNamespace(magnitude=lambda: speed)


class StaticObject:
    def __init__(self, heading, kind):
        self.box = types.SimpleNamespace(center=types.SimpleNamespace(heading=heading))
        self.tracked_object_type = TrackedObjectType[kind]


def relative_angle(ego, agent):
    """nuPlan's get_agent_relative_angle, as quoted in include/ddmi.h."""
    vector = np.array([agent.x - ego.x, agent.y - ego.y])
    with np.errstate(invalid="ignore", divide="ignore"):
        cosine = np.dot(np.array([np.cos(ego.heading), np.sin(ego.heading)]), vector / np.linalg.norm(vector))
        angle = float(np.arccos(cosine))
    LOG["angle"] = min(LOG["angle"], abs(angle - ANGLES["ahead"]), abs(angle - ANGLES["behind"]))
    LOG["cosine"] = min(LOG["cosine"], 1.0 - abs(float(cosine)))
    return angle


def is_agent_ahead(ego, agent):
    return bool(relative_angle(ego, agent) < ANGLES["ahead"])


def is_agent_behind(ego, agent):
    return bool(relative_angle(ego, agent) > ANGLES["behind"])


def is_track_stopped(tracked_object, stopped_speed_threshold=R.TRACK_STOPPED_SPEED):
    if not isinstance(tracked_object, Agent):
        return True
    return bool(tracked_object.velocity.magnitude() <= stopped_speed_threshold)


def install_reference():
    import refshim
    from refshim import stubs
    refshim.install_stub_finder()

    def register(name, **real):
        mod = stubs._StubModule(name)   # every other name of the module stays a stub
        for k, v in real.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        return mod

    layers = enum.IntEnum("SemanticMapLayer", A.LAYER_IDS)
    register("nuplan.common.maps.maps_datatypes", SemanticMapLayer=layers)
    register("nuplan.common.actor_state.state_representation", StateSE2=StateSE2)
    register("nuplan.common.actor_state.tracked_objects_types", TrackedObjectType=TrackedObjectType,
             AGENT_TYPES=AGENT_TYPES)
    register("nuplan.planning.metrics.utils.collision_utils", CollisionType=CollisionType)
    register("nuplan.planning.simulation.observation.idm.utils", is_agent_ahead=is_agent_ahead,
             is_agent_behind=is_agent_behind, is_track_stopped=is_track_stopped)
    creation = register("shapely.creation", polygons=polygons)
    register("shapely", Point=Point, LineString=LineString, Polygon=Polygon, creation=creation)
    sys.path.insert(0, REF)
    from navsim.planning.simulation.planner.pdm_planner.scoring import pdm_scorer, pdm_scorer_utils
    from navsim.planning.simulation.planner.pdm_planner.utils.pdm_enums import MultiMetricIndex, WeightedMetricIndex
    assert pdm_scorer.SemanticMapLayer is layers and pdm_scorer.Point is Point and pdm_scorer.creation is creation
    assert pdm_scorer_utils.LineString is LineString and pdm_scorer.AGENT_TYPES is AGENT_TYPES
    inner = pdm_scorer.get_collision_type

    def recording(*args, **kwargs):   # the reference keeps no record of the type it acts on
        kind = inner(*args, **kwargs)
        LOG["types"].append(int(kind))
        return kind

    pdm_scorer.get_collision_type = recording
    return pdm_scorer, layers, MultiMetricIndex, WeightedMetricIndex, inner


# ---- the duck-typed inputs

class OccupancyMap:
    def __init__(self, tracks, t):
        here = [tr for tr in tracks if tr["valid"][t]]
        self.tokens = [tr["token"] for tr in here]
        self.boxes = np.stack([tr["boxes"][t] for tr in here]) if here else np.zeros((0, 4, 2))
        self._polygons = {tr["token"]: Polygon(tr["boxes"][t]) for tr in here}

    def __getitem__(self, token):
        return self._polygons[token]

    def query(self, geometries, predicate=None):
        assert predicate == "intersects"
        quads = np.stack([g.quad for g in geometries])
        if not len(self.tokens):
            return np.zeros((2, 0), dtype=np.int64)
        hits = R.quads_touch(quads[:, None], self.boxes[None])
        LOG["gap"] = min(LOG["gap"], float(np.abs(R.gap(quads[:, None], self.boxes[None])).min()))
        for i in range(quads.shape[0]):
            for j in range(self.boxes.shape[0]):
                touch_checked(quads[i], self.boxes[j], hits[i, j], log_gap=False)
        return np.stack(np.nonzero(hits))


class Observation:
    red_light_token = R.RED_LIGHT

    def __init__(self, tracks, collided):
        self._maps = [OccupancyMap(tracks, t) for t in range(len(tracks[0]["valid"]))]
        self.collided_track_ids = list(collided)
        self.unique_objects = {tr["token"]: Agent(tr["heading"], tr["kind"], tr["speed"]) if tr["is_agent"]
                               else StaticObject(tr["heading"], tr["kind"]) for tr in tracks}

    def __getitem__(self, t):
        return self._maps[t]


class Centerline:
    def __init__(self, line):
        self.line = line

    def project(self, points):
        out = []
        for p in points:
            got = float(R.project(self.line, p.x, p.y))
            if np.isfinite(got):
                want, bound = R.independent_project(self.line, p.x, p.y)
                assert abs(got - want) <= bound, ("the projection and the dense sampling differ", got, want)
                LOG["tie"] = min(LOG["tie"], tie_margin(self.line, p.x, p.y))
            out.append(got)
        return np.array(out)


def tie_margin(line, x, y):
    """The distance between the two nearest segments' distances, inf where they are adjacent at the nearest vertex."""
    a, b = line[:-1], line[1:]
    d = b - a
    s = np.clip(((x - a[:, 0]) * d[:, 0] + (y - a[:, 1]) * d[:, 1]) / (d * d).sum(-1), 0.0, 1.0)
    dist = np.hypot(x - (a[:, 0] + s * d[:, 0]), y - (a[:, 1] + s * d[:, 1]))
    i, j = np.argsort(dist)[:2]
    lo, hi = min(i, j), max(i, j)
    if hi == lo + 1 and s[lo] == 1.0 and s[hi] == 0.0:
        return np.inf
    return float(dist[j] - dist[i])


class Map(MA.DuckMap):
    def __init__(self, items, tokens, layer_enum, checks):
        super().__init__(items, tokens, layer_enum)
        self.checks = checks

    def is_in_layer(self, point, layer):
        inside = False
        for item, kind, check in zip(self.items, self.map_types, self.checks):
            if kind != layer:
                continue
            got = bool(A.contains(item[0], point.x, point.y))
            assert got == bool(MA.independent_inside(check, np.float64(point.x), np.float64(point.y)))
            LOG["axle"] = min(LOG["axle"], A.edge_distance([item], np.array([[point.x, point.y]])))
            inside |= got
        return inside


def run_reference(ref, states, scene, ap, sp, pairs_with=None):
    """One call of the reference's stages over ``states``; ``scene`` = (items, tokens, route ids, checks, tracks,
    collided, line)."""
    pdm_scorer, layer_enum, multi, weighted, collision_type = ref
    from refshim.stubs import TrajectorySampling
    items, tokens, ids, checks, tracks, collided, line = scene
    config = pdm_scorer.PDMScorerConfig(
        progress_weight=sp["progress_weight"], ttc_weight=sp["ttc_weight"],
        comfortable_weight=sp["comfortable_weight"], driving_direction_weight=sp["driving_direction_weight"],
        driving_direction_horizon=ap["driving_direction_horizon"],
        driving_direction_compliance_threshold=ap["driving_direction_compliance_threshold"],
        driving_direction_violation_threshold=ap["driving_direction_violation_threshold"],
        stopped_speed_threshold=sp["ttc_stopped_speed_threshold"],
        progress_distance_threshold=sp["progress_distance_threshold"])
    vehicle = types.SimpleNamespace(half_length=ap["half_length"], half_width=ap["half_width"],
                                    rear_axle_to_center=ap["rear_axle_to_center"])
    ANGLES.update(ahead=sp["ahead_angle"], behind=sp["behind_angle"])
    defaults = collision_type.__defaults__
    collision_type.__defaults__ = (sp["collision_stopped_speed_threshold"],)
    LOG["types"] = []
    try:
        scorer = pdm_scorer.PDMScorer(TrajectorySampling(num_poses=A.T - 1, interval_length=ap["dt"]), config, vehicle)
        with np.errstate(invalid="ignore"):
            scorer._reset(states, Observation(tracks, collided), Centerline(line), ids,
                          Map(items, tokens, layer_enum, checks))
            exterior = scorer._ego_coords.copy()
            exterior[..., A.CENTER, :] = exterior[..., A.FRONT_LEFT, :]
            scorer._ego_polygons = polygons(exterior)
            scorer._calculate_ego_area()
            scorer._calculate_no_at_fault_collision()
            scorer._calculate_drivable_area_compliance()
            scorer._calculate_driving_direction_compliance()
            scorer._calculate_progress()
            scorer._calculate_ttc()
            scorer._calculate_is_comfortable()
            score = scorer._aggregate_scores()
    finally:
        collision_type.__defaults__ = defaults
    return dict(no_collision=scorer._multi_metrics[multi.NO_COLLISION].copy(),
                drivable_area=scorer._multi_metrics[multi.DRIVABLE_AREA].copy(),
                driving_direction=scorer._weighted_metrics[weighted.DRIVING_DIRECTION].copy(),
                progress=scorer._weighted_metrics[weighted.PROGRESS].copy(),
                ttc=scorer._weighted_metrics[weighted.TTC].copy(),
                comfortable=scorer._weighted_metrics[weighted.COMFORTABLE].copy(),
                collision_time_idx=scorer._collision_time_idcs.copy(), ttc_time_idx=scorer._ttc_time_idcs.copy(),
                raw_progress=scorer._progress_raw.copy(), score=np.asarray(score).copy(),
                areas=scorer._ego_areas.copy(), types=np.bincount(LOG["types"], minlength=5)[:5])


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    ref = install_reference()
    sims = {}
    for name in SIM_SETS:
        with np.load(os.path.join(HERE, f"pdm_sim_s3_{name}.npz")) as g:
            sims[name] = g["states"]
    P, ALT = A.params(), A.params(**A.ALT)
    S, SALT = R.score_params(), R.score_params(**R.SCORE_ALT)
    while True:
        for k in ("gap", "angle", "cosine", "axle", "tie"):
            LOG[k] = np.inf
        results, margins = {}, dict(speed=np.inf, pmax=np.inf, comfort=np.inf)

        def run(key, states, scene, ap, sp):
            out = run_reference(ref, states, scene, ap, sp)
            results[key] = out
            inter = [it[0] for it in scene[0] if it[1] == "INTERSECTION"]
            first = R.collisions(states, out["areas"], scene[4], inter, ap, sp, scene[5])["types"]
            out["first_types"] = np.bincount(first[first >= 0], minlength=5)[:5]   # the deciding first hits
            f = np.hypot(states[..., R.VX], states[..., R.VY])
            f = f[np.isfinite(f)]
            for th in (sp["ttc_stopped_speed_threshold"], sp["collision_stopped_speed_threshold"]):
                margins["speed"] = min(margins["speed"], float(np.abs(f - th).min()))
            with np.errstate(invalid="ignore"):
                pmax = np.max(out["raw_progress"] * out["no_collision"] * out["drivable_area"])
            if np.isfinite(pmax):
                margins["pmax"] = min(margins["pmax"], abs(float(pmax) - sp["progress_distance_threshold"]))
            cp = C.params(dt=ap["dt"])
            margins["comfort"] = min(margins["comfort"], C.margin(C.comfort(states, cp)[1], cp))
            return out

        for k, name in enumerate(SIM_SETS):
            run(name, sims[name], R.seeded_scene(seed + k, sims[name], lanes=3 if k != 1 else 2), P, S)
        synth = R.with_velocity(A.synthetic_states(seed))
        scene = R.seeded_scene(seed + 3, synth)
        run("synth", synth, scene, P, S)
        nan_states = synth[NAN_ROW:NAN_ROW + 1].copy()
        nan_states[0, NAN_AT, A.X] = np.nan
        results["nan"] = run_reference(ref, nan_states, scene, P, S)
        run("alt", sims["moving"][:ALT_ROWS], R.seeded_scene(seed, sims["moving"], dt=ALT["dt"]), ALT, SALT)
        # the pairs [candidate 0, candidate i] of the moving set: pdm_score.py's rule
        moving_scene = R.seeded_scene(seed, sims["moving"])
        pair = [run_reference(ref, sims["moving"][[0, i]], moving_scene, P, S) for i in range(len(sims["moving"]))]
        results["pair"] = {k: np.array([q[k][1] for q in pair]) for k in ("score", "progress", "raw_progress")}
        group = results["moving"]
        reference = float(group["raw_progress"][0] * group["no_collision"][0] * group["drivable_area"][0])
        margins["pmax"] = min(margins["pmax"], float(np.abs(np.maximum(
            reference, group["raw_progress"] * group["no_collision"] * group["drivable_area"]) - 5.0).min()))

        names = SIM_SETS + ("synth",)
        ncs = set(np.concatenate([results[n]["no_collision"] for n in names]).tolist())
        ttcs = set(np.concatenate([results[n]["ttc"] for n in names]).tolist())
        kinds = sum(results[n]["first_types"] for n in names)
        branches = {bool(np.max(results[n]["raw_progress"] * results[n]["no_collision"] * results[n]["drivable_area"])
                         > 5.0) for n in names + ("alt",)}
        differs = bool((results["pair"]["score"] != group["score"]).any())
        covered = (ncs == {0.0, 0.5, 1.0} and ttcs == {0.0, 1.0} and (kinds > 0).all() and branches == {True, False}
                   and differs)
        ok = (covered and LOG["gap"] >= MARGIN and margins["speed"] >= MARGIN and LOG["angle"] >= ANGLE_MARGIN
              and LOG["cosine"] >= 1e-12 and LOG["axle"] >= MARGIN and LOG["tie"] >= MARGIN and margins["pmax"] >= MARGIN
              and margins["comfort"] >= COMFORT_MARGIN)
        print(f"seed {seed}: no_collision {sorted(ncs)}, ttc {sorted(ttcs)}, types {kinds.tolist()}, branches "
              f"{sorted(branches)}, pair differs {differs}; margins: gap {LOG['gap']:.3e}, speed {margins['speed']:.3e}, "
              f"angle {LOG['angle']:.3e}, cosine {LOG['cosine']:.3e}, axle {LOG['axle']:.3e}, tie {LOG['tie']:.3e}, "
              f"pmax {margins['pmax']:.3e}, comfort {margins['comfort']:.3e}{'' if ok else ': next seed'}")
        if ok:
            break
        seed += 1

    rec = dict(seed=np.array(seed), gap_margin=np.array(LOG["gap"]), speed_margin=np.array(margins["speed"]),
               angle_margin=np.array(LOG["angle"]), axle_margin=np.array(LOG["axle"]), tie_margin=np.array(LOG["tie"]),
               pmax_margin=np.array(margins["pmax"]), comfort_margin=np.array(margins["comfort"]),
               pair_reference=np.array(reference),
               alt_names=np.array(list(R.SCORE_ALT)), alt_values=np.array([R.SCORE_ALT[k] for k in R.SCORE_ALT]))
    for key, out in results.items():
        for k, v in out.items():
            if k != "areas":   # the flags are pdm_area_s*.npz's business
                rec[f"{k}_{key}"] = np.asarray(v)
    for k, v in rec.items():   # numbers, booleans and short names: nothing of the reference's program text
        assert v.dtype.kind in "fib" or (v.dtype.kind == "U" and v.size <= 16 and max(map(len, v.ravel())) < 48), k
    path = os.path.join(HERE, f"pdm_score_s{seed}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path}: {size} bytes")
    for key in names + ("alt", "nan"):
        out = results[key]
        print(f"  {key}: no_collision {np.unique(out['no_collision'], return_counts=True)}, ttc "
              f"{np.unique(out['ttc'], return_counts=True)}, types {out['types'].tolist()}, raw progress "
              f"{np.nanmin(out['raw_progress']):.3f} .. {np.nanmax(out['raw_progress']):.3f}, score "
              f"{np.nanmin(out['score']):.4f} .. {np.nanmax(out['score']):.4f}")


if __name__ == "__main__":
    main()
