#!/usr/bin/env python3
"""Golden vectors of the PDM scorer's map compliance, from the REFERENCE's PDMScorer run unmodified (build container
only: it needs the reference tree).

shapely and nuPlan are not available, and ``refshim`` stubs them, so shapely's containment cannot be run; everything
else of the reference can. Before the import a stand-in for ``nuplan.common.maps.maps_datatypes`` is registered whose
``SemanticMapLayer`` is a real IntEnum (the stub classes do not compare equal to themselves, and
``get_indices_of_map_type`` compares layers). A ``PDMScorer`` is then built from the stand-in
``TrajectorySampling(num_poses=40, interval_length=dt)``, a ``PDMScorerConfig`` and a SimpleNamespace of vehicle
parameters, and ``_reset``, ``_calculate_ego_area``, ``_calculate_drivable_area_compliance`` and
``_calculate_driving_direction_compliance`` run as they are on a duck-typed map object with ``tokens``,
``get_indices_of_map_type`` and ``points_in_polygons``. Read back: ``_ego_coords``, ``_ego_areas``,
``_multi_metrics[DRIVABLE_AREA]``, ``_weighted_metrics[DRIVING_DIRECTION]``. The reference does not keep the windowed
progress m; it is formed here from the reference's own coords and flags (pdm_area_ref.oncoming_progress).

Only the containment primitive inside the duck-typed map stands in for shapely: pdm_area_ref.contains, an even-odd
crossing test. It is checked here on EVERY golden point against an independent predicate that shares no code with it:
all half-plane signs equal on convex rings; in the exterior and in no hole; in any convex part of a non-convex polygon.

Inputs:
  (a) the ``states`` of the three committed tests/golden/pdm_sim_s3_*.npz sets (not stored again: keyed by name), each
      on a seeded map laid around its start pose (pdm_area_ref.seeded_map: two or three lanes under a roadblock, an
      intersection with a hole and lane connectors, one of them non-convex, a carpark, an off-route lane); the
      ``global`` set's map sits at its 6.6e5 / 4.0e6 m coordinates;
  (b) 96 synthetic state arrays with large headings and lateral motion (pdm_area_ref.synthetic_states);
  (c) the hand-built cases (pdm_area_ref.hand_cases), each on its own map;
  (d) one row of (b) with a NaN pose;
  (e) the first 24 rows of (b) under non-default parameters (pdm_area_ref.ALT: other vehicle lengths, dt = 0.125,
      horizon 0.5, thresholds 1 / 3).
The maps are not stored: the tests rebuild them from the recorded seed. The coords of sets (a) and (b) are stored for
every third candidate (COORD_ROWS), to keep the file under the size limit; flags, scores and m for every candidate.

Asserted, a failing seed being replaced by the next one and no candidate excluded: every tested point is at least 1e-6
m from every edge of every polygon of its scene; every finite m is at least 1e-6 from both thresholds; each of the
three flags is both set and clear somewhere; the scores take all of {1, 0.5, 0} and {1, 0}.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_area_golden.py [seed]
Writes tests/golden/pdm_area_s{seed}.npz. Only data is stored; nothing of the reference's source.
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

import pdm_area_ref as R  # noqa: E402

SEED = 11
MARGIN = 1e-6
SIM_SETS = ("moving", "standing", "global")
COORD_ROWS = slice(0, 96, 3)
ALT_ROWS = 24
NAN_ROW, NAN_AT = 5, 17


def install_reference():
    """The stub finder, the real SemanticMapLayer, then the reference's scorer module."""
    import refshim
    from refshim import stubs
    refshim.install_stub_finder()
    name = "nuplan.common.maps.maps_datatypes"
    mod = stubs._StubModule(name)   # every other name of the module stays a stub
    mod.SemanticMapLayer = enum.IntEnum("SemanticMapLayer", R.LAYER_IDS)
    sys.modules[name] = mod
    sys.path.insert(0, REF)
    from navsim.planning.simulation.planner.pdm_planner.scoring import pdm_scorer
    from navsim.planning.simulation.planner.pdm_planner.utils.pdm_enums import MultiMetricIndex, WeightedMetricIndex
    assert pdm_scorer.SemanticMapLayer is mod.SemanticMapLayer
    return pdm_scorer, mod.SemanticMapLayer, MultiMetricIndex, WeightedMetricIndex


class DuckMap:
    """What _calculate_ego_area reads of a PDMDrivableMap; ``contains`` stands in for shapely.vectorized.contains."""

    def __init__(self, items, tokens, layer_enum):
        self.items, self.tokens = items, tokens
        self.map_types = [layer_enum[layer] for _, layer, _ in items]

    def get_indices_of_map_type(self, map_types):
        return [i for i, t in enumerate(self.map_types) if t in map_types]

    def points_in_polygons(self, points):
        return R.in_polygons(self.items, points)


def independent_inside(check, x, y):
    """Containment by half-plane signs, for the convex pieces a polygon is known to be made of."""
    def convex(ring):
        v = np.asarray(ring)
        w = np.roll(v, -1, axis=0)
        side = np.stack([(c - a) * (y - b) - (d - b) * (x - a) for (a, b), (c, d) in zip(v, w)])
        return (side > 0).all(0) | (side < 0).all(0)
    if check[0] == "convex":
        return convex(check[1])
    if check[0] == "union":
        return np.any([convex(r) for r in check[1]], axis=0)
    inside = convex(check[1])
    for hole in check[2]:
        inside &= ~convex(hole)
    return inside


def run_reference(ref, states, items, tokens, route_ids, p):
    pdm_scorer, layer_enum, multi, weighted = ref
    from refshim.stubs import TrajectorySampling
    config = pdm_scorer.PDMScorerConfig(
        driving_direction_horizon=p["driving_direction_horizon"],
        driving_direction_compliance_threshold=p["driving_direction_compliance_threshold"],
        driving_direction_violation_threshold=p["driving_direction_violation_threshold"])
    vehicle = types.SimpleNamespace(half_length=p["half_length"], half_width=p["half_width"],
                                    rear_axle_to_center=p["rear_axle_to_center"])
    scorer = pdm_scorer.PDMScorer(TrajectorySampling(num_poses=R.T - 1, interval_length=p["dt"]), config, vehicle)
    with np.errstate(invalid="ignore"):
        scorer._reset(states, None, None, route_ids, DuckMap(items, tokens, layer_enum))
        scorer._calculate_ego_area()
        scorer._calculate_drivable_area_compliance()
        scorer._calculate_driving_direction_compliance()
    pts, areas = scorer._ego_coords.copy(), scorer._ego_areas.copy()
    m = R.oncoming_progress(pts[:, :, R.CENTER], areas[..., R.ONCOMING], R.horizon_steps(p))
    return dict(coords=pts, areas=areas, drivable_area=scorer._multi_metrics[multi.DRIVABLE_AREA].copy(),
                driving_direction=scorer._weighted_metrics[weighted.DRIVING_DIRECTION].copy(), m=m)


def check_points(tag, items, checks, pts, p):
    """The margin to every edge, the margin of m, and the stand-in primitive against the independent predicate."""
    x, y = pts[..., 0], pts[..., 1]
    for i, (item, check) in enumerate(zip(items, checks)):
        a, b = R.contains(item[0], x, y), independent_inside(check, x, y)
        assert np.array_equal(a, b), f"{tag}: polygon {i}: the crossing test and the half-plane test differ"
    return R.edge_distance(items, pts)


def m_margin(m, p):
    f = m[np.isfinite(m)]
    th = np.array([p["driving_direction_compliance_threshold"], p["driving_direction_violation_threshold"]])
    return float(np.abs(f[:, None] - th).min()) if f.size else np.inf


def scene_pose(states):
    return tuple(states[0, 0, :3])


def convex_checks(items):
    return [("holes", it[0][0], list(it[0][1:])) for it in items]   # the hand-built rings are all rectangles


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    ref = install_reference()
    sims = {}
    for name in SIM_SETS:
        with np.load(os.path.join(HERE, f"pdm_sim_s3_{name}.npz")) as g:
            sims[name] = g["states"]
    P, ALT = R.params(), R.params(**R.ALT)
    while True:
        rec, edge, mm = {}, np.inf, np.inf
        results = {}
        for k, name in enumerate(SIM_SETS):
            items, tokens, ids, checks = R.seeded_map(seed + k, scene_pose(sims[name]), lanes=3 if k != 1 else 2)
            out = run_reference(ref, sims[name], items, tokens, ids, P)
            edge = min(edge, check_points(name, items, checks, out["coords"], P))
            mm = min(mm, m_margin(out["m"], P))
            results[name] = out
        items, tokens, ids, checks = R.seeded_map(seed + 3)
        synth = R.synthetic_states(seed)
        out = run_reference(ref, synth, items, tokens, ids, P)
        edge = min(edge, check_points("synth", items, checks, out["coords"], P))
        mm = min(mm, m_margin(out["m"], P))
        results["synth"] = out
        nan_states = synth[NAN_ROW:NAN_ROW + 1].copy()
        nan_states[0, NAN_AT, R.X] = np.nan
        results["nan"] = run_reference(ref, nan_states, items, tokens, ids, P)
        check_points("nan", items, checks, results["nan"]["coords"], P)   # a NaN point is outside for both predicates
        out = run_reference(ref, synth[:ALT_ROWS], items, tokens, ids, ALT)
        edge = min(edge, check_points("alt", items, checks, out["coords"], ALT))
        mm = min(mm, m_margin(out["m"], ALT))
        results["alt"] = out
        flags = np.concatenate([results[k]["areas"].reshape(-1, 3) for k in SIM_SETS + ("synth",)])
        dac = np.concatenate([results[k]["drivable_area"] for k in SIM_SETS + ("synth",)])
        ddc = np.concatenate([results[k]["driving_direction"] for k in SIM_SETS + ("synth",)])
        covered = (flags.any(0).all() and (~flags).any(0).all() and set(dac.tolist()) == {0.0, 1.0}
                   and set(ddc.tolist()) == {0.0, 0.5, 1.0})
        if covered and edge >= MARGIN and mm >= MARGIN:
            break
        print(f"seed {seed}: covered = {covered}, margin to an edge {edge:.3e}, of m {mm:.3e} (< {MARGIN}?); next seed")
        seed += 1

    for i, (name, items, states, _) in enumerate(R.hand_cases()):
        tokens = [f"h{i}_{j}" for j in range(len(items))]
        ids = [t for t, it in zip(tokens, items) if it[2]]      # a roadblock's token may be among them
        out = run_reference(ref, states, items, tokens, ids, P)
        edge = min(edge, check_points(name, items, convex_checks(items), out["coords"], P))
        mm = min(mm, m_margin(out["m"], P))
        results[f"hand_{name}"] = out
    assert edge >= MARGIN and mm >= MARGIN, (edge, mm)

    rec.update(seed=np.array(seed), edge_margin=np.array(edge), m_margin=np.array(mm), states_synth=synth,
               states_nan=nan_states, coord_rows=np.arange(96)[COORD_ROWS],
               alt_names=np.array(list(R.ALT)), alt_values=np.array([R.ALT[k] for k in R.ALT]),
               hand_names=np.array([c[0] for c in R.hand_cases()]))
    for key, out in results.items():
        thin = key in SIM_SETS + ("synth",)
        rec[f"coords_{key}"] = out["coords"][COORD_ROWS] if thin else out["coords"]
        for k in ("areas", "drivable_area", "driving_direction", "m"):
            rec[f"{k}_{key}"] = out[k]
    for k, v in rec.items():   # numbers, booleans and short names: nothing of the reference's program text
        assert v.dtype.kind in "fib" or (v.dtype.kind == "U" and v.size <= 16 and max(map(len, v.ravel())) < 48), k
    path = os.path.join(HERE, f"pdm_area_s{seed}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path}: {size} bytes; margin to an edge {edge:.3e}, of m {mm:.3e}")
    for key in SIM_SETS + ("synth", "alt", "nan"):
        out = results[key]
        print(f"  {key}: flags set {out['areas'].reshape(-1, 3).sum(0).tolist()} of {out['areas'][..., 0].size}, "
              f"drivable {np.unique(out['drivable_area'], return_counts=True)}, direction "
              f"{np.unique(out['driving_direction'], return_counts=True)}")


if __name__ == "__main__":
    main()
