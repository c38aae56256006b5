#!/usr/bin/env python3
"""Golden vectors of PDM's forecasted observation from the REFERENCE's PDMObservation.update and PDMObjectManager run
unmodified (build container only: it needs the reference tree): _get_object_manager, add_object, get_nearest_objects,
_get_nearest_dynamic_objects, _get_nearest_static_objects, the forecast loop, PDMOccupancyMap and the collided ids.

shapely and nuPlan are not available and ``refshim`` stubs them. Before the reference is imported, real stand-ins are
registered where the stub finder would hand out stubs: ``TrackedObjectType`` and ``AGENT_TYPES`` (as remembered: VEHICLE,
PEDESTRIAN, BICYCLE), ``shapely.creation.polygons`` (an object array of duck polygons over the first four of the five
points), ``shapely.geometry.Polygon`` and ``shapely.strtree.STRtree`` whose ``query(geometry, predicate="intersects")``
answers with tests/pdm_observation_ref.py's closed separating-axis test. The detections are duck ``TrackedObject``s:
``box.all_corners()`` gives front-left, rear-left, rear-right, front-right by the formula of tests/pdm_area_ref.py:60-69
(nuPlan's translate_longitudinally_and_laterally as this project quotes it), ``center.distance_to`` is the hypot of the
differences and ``velocity.magnitude()`` the hypot of the components (all three quoted from memory of nuPlan). The ego
state is a duck whose ``center`` is the rear axle moved by rear_axle_to_center along the heading and whose
``car_footprint.geometry`` is the ego quad by dd_ego_areas' corner formulas. No traffic light is passed: the red-light
rings stay host data in this project (diffusiondrive_amd.simulate.ring_holds_quad).

The intersection stand-in is checked on EVERY use against an independent predicate that shares no code with it: dense
samples of both boundaries tested against the other quad's four half-planes.

The update runs twice per scene on one PDMObservation, as a planner does: the second call starts from the first call's
collided ids, so the track that overlaps the ego no longer takes a place under its cap. Both calls are stored: the
inputs, the token list (the same in every one of a call's 26 maps, which is asserted, so it is stored once), the
polygons of every map and the collided ids after the call.

Asserted, a failing seed being replaced by the next: within every class the sorted distances are >= 1e-6 m apart; every
distance is >= 1e-6 m from the radius; every moving agent's |normalize(h - velocity_angle)| is >= 1e-6 rad from pi / 2;
every agent's speed is >= 1e-6 m/s from the stopped speed; every kept box is >= 5e-3 m clear of the ego quad or
overlaps it by as much; all four caps are passed, an agent reverses, a track overlaps the ego, an object lies beyond the
radius and an EGO row occurs; the restatement reproduces the reference (tokens and collided ids equal, boxes within
its bar).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_observation_golden.py [seed]
Writes tests/golden/pdm_observation_s{seed}.npz. Only data is stored; nothing of the reference's source.
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

import pdm_area_ref as A  # noqa: E402
import pdm_observation_ref as O  # noqa: E402

SEED = 1
LOG = dict(queries=0, pairs=0)


class TrackedObjectType(enum.Enum):
    VEHICLE = 0
    PEDESTRIAN = 1
    BICYCLE = 2
    TRAFFIC_CONE = 3
    BARRIER = 4
    CZONE_SIGN = 5
    GENERIC_OBJECT = 6
    EGO = 7


AGENT_TYPES = {TrackedObjectType.VEHICLE, TrackedObjectType.PEDESTRIAN, TrackedObjectType.BICYCLE}


# ---- shapely's duck classes

class Polygon:
    def __init__(self, coords):
        a = np.asarray(coords, dtype=np.float64)
        self.ring = a[:4] if a.shape == (5, 2) else a
        assert self.ring.shape == (4, 2), a.shape
        self.exterior = types.SimpleNamespace(coords=np.concatenate([self.ring, self.ring[:1]]))

    def within(self, other):
        raise AssertionError("within is asked of red lights only, and none is passed")


def polygons(coords):
    coords = np.asarray(coords, dtype=np.float64)
    assert coords.ndim == 3 and coords.shape[1:] == (5, 2), coords.shape
    assert np.array_equal(coords[:, 4], coords[:, 0]), "the fifth point closes the ring (CENTER := FRONT_LEFT)"
    out = np.empty(len(coords), dtype=np.object_)
    for i, c in enumerate(coords):
        out[i] = Polygon(c)
    return out


def _rim(ring, spacing=1e-3):
    pts = []
    for a, b in zip(ring, np.roll(ring, -1, axis=0)):
        n = max(int(np.ceil(np.hypot(*(b - a)) / spacing)), 1)
        pts.append(a + (b - a) * (np.arange(n) / n)[:, None])
    return np.concatenate(pts)


def _inside_closed(ring, pts):
    """Points in the closed convex quad, by its four half-planes (either orientation)."""
    a, b = ring, np.roll(ring, -1, axis=0)
    cross = ((b[:, 0] - a[:, 0])[None] * (pts[:, 1, None] - a[None, :, 1])
             - (b[:, 1] - a[:, 1])[None] * (pts[:, 0, None] - a[None, :, 0]))
    return (cross >= 0).all(1) | (cross <= 0).all(1)


def independent_intersects(q, b):
    o = q[0]   # both moved to the ego quad's first corner: the scenes sit at 4e6 m
    q, b = q - o, b - o
    return bool(_inside_closed(b, _rim(q)).any() or _inside_closed(q, _rim(b)).any())


class STRtree:
    def __init__(self, geometries, node_capacity=10):
        self.geometries = list(geometries)

    def query(self, geometry, predicate=None):
        assert predicate == "intersects", predicate
        LOG["queries"] += 1
        out = []
        for i, g in enumerate(self.geometries):
            met = O.quads_touch(geometry.ring, g.ring)
            if abs(O.separation(geometry.ring, g.ring)) >= O.MIN_EGO_GAP and \
                    max(np.abs(g.ring - geometry.ring[0]).max(), 0.0) < 20.0:
                assert met == independent_intersects(geometry.ring, g.ring), "the SAT test and the sampled one differ"
                LOG["pairs"] += 1
            if met:
                out.append(i)
        return np.asarray(out, dtype=np.int64)


# ---- nuPlan's duck classes

class Center:
    def __init__(self, x, y, heading):
        self.x, self.y, self.heading = x, y, heading

    @property
    def point(self):
        return types.SimpleNamespace(x=self.x, y=self.y, array=np.array([self.x, self.y], dtype=np.float64))

    def distance_to(self, other):
        return float(np.hypot(self.x - other.x, self.y - other.y))


class Box:
    def __init__(self, center, length, width):
        self.center, self.length, self.width = center, length, width

    def all_corners(self):
        c = O.corners(self.center.x, self.center.y, self.center.heading, self.length / 2.0, self.width / 2.0)
        return [types.SimpleNamespace(x=float(x), y=float(y)) for x, y in c]


class Velocity:
    def __init__(self, x, y):
        self.x, self.y = x, y

    def magnitude(self):
        return float(np.hypot(self.x, self.y))


class TrackedObject:
    def __init__(self, row):
        token, x, y, h, length, width, vx, vy, name = row
        self.track_token = token
        self.tracked_object_type = TrackedObjectType[name]
        self.center = Center(x, y, h)
        self.box = Box(self.center, length, width)
        if self.tracked_object_type in AGENT_TYPES or name == "EGO":
            self.velocity = Velocity(vx, vy)


def ego_state_of(ego, ap):
    cx, cy = O.ego_center(ego, ap)
    return types.SimpleNamespace(center=Center(float(cx), float(cy), float(ego[2])),
                                 car_footprint=types.SimpleNamespace(geometry=Polygon(O.ego_quad(ego, ap))))


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

    register("nuplan.common.actor_state.tracked_objects_types", TrackedObjectType=TrackedObjectType,
             AGENT_TYPES=AGENT_TYPES)
    creation = register("shapely.creation", polygons=polygons)
    geometry = register("shapely.geometry", Polygon=Polygon)
    strtree = register("shapely.strtree", STRtree=STRtree)
    vectorized = register("shapely.vectorized")
    register("shapely", creation=creation, geometry=geometry, strtree=strtree, vectorized=vectorized, Polygon=Polygon)
    sys.path.insert(0, REF)
    from navsim.planning.simulation.planner.pdm_planner.observation import pdm_object_manager, pdm_observation, \
        pdm_occupancy_map
    assert pdm_observation.shapely.creation.polygons is polygons and pdm_occupancy_map.STRtree is STRtree
    assert pdm_observation.TrackedObjectType is TrackedObjectType and pdm_object_manager.AGENT_TYPES is AGENT_TYPES
    assert pdm_observation.PDMObjectManager is pdm_object_manager.PDMObjectManager
    assert pdm_object_manager.MAX_DYNAMIC_OBJECTS == {TrackedObjectType.VEHICLE: 50, TrackedObjectType.PEDESTRIAN: 25,
                                                      TrackedObjectType.BICYCLE: 10}
    assert pdm_object_manager.MAX_STATIC_OBJECTS == 50
    return pdm_observation


def run_reference(pdm_observation, scene, ap, calls=2):
    """[per call: (tokens per map, polygons per map (maps, n, 4, 2), collided ids after the call)]"""
    from refshim.stubs import TrajectorySampling
    p = O.DEFAULTS
    obs = pdm_observation.PDMObservation(TrajectorySampling(num_poses=40, interval_length=p["dt"]),
                                         TrajectorySampling(num_poses=40, interval_length=p["dt"]),
                                         map_radius=p["map_radius"], observation_sample_res=p["sample_res"])
    assert obs._observation_samples == p["num_samples"] and len(obs._global_to_local_idcs) == O.t_obs(p)
    detections = types.SimpleNamespace(tracked_objects=[TrackedObject(r) for r in scene["dets"]])
    out = []
    for _ in range(calls):
        obs.update(ego_state_of(scene["ego"], ap), detections, [], {})
        maps = obs._occupancy_maps
        assert len(maps) == p["num_samples"] // p["sample_res"] + 1
        tokens = [list(m.tokens) for m in maps]
        polys = np.stack([np.stack([g.ring for g in m._geometries]) if len(m.tokens) else np.zeros((0, 4, 2))
                          for m in maps])
        assert set(obs.unique_objects) >= set(tokens[0])
        out.append((tokens, polys, list(obs.collided_track_ids)))
    # observation[t] reads map t // sample_res
    for t in range(O.t_obs(p)):
        assert obs[t] is obs._occupancy_maps[t // p["sample_res"]]
    return out


def compare_call(scene, tokens, polys, collided_ids, out64, outld):
    """The restatement against one call of the reference: tokens and collided ids EQUAL, boxes within the bar."""
    p = O.DEFAULTS
    names = scene["tokens"]
    kept = [names[d] for d, k in zip(out64["order"], out64["kept"]) if k]
    for m in tokens:
        assert m == kept, "token order"
    assert sorted(collided_ids) == sorted(names[d] for d in np.flatnonzero(out64["collided"])), "collided ids"
    worst = 0.0
    reach = O.reach_of(scene["boxes"], out64["order"], p)
    bar = O.box_bar(out64["boxes"], outld["boxes"], reach)
    slots = np.flatnonzero(out64["kept"])
    for t in range(O.t_obs(p)):
        ref = polys[t // p["sample_res"]]
        for i, k in enumerate(slots):
            if not out64["valid"][k]:
                continue   # newly collided: in the reference's maps, invalid here
            err = np.abs(out64["boxes"][k, t] - ref[i])
            assert (err <= bar[k, t]).all(), (scene["name"], t, k, err.max(), bar[k, t].min())
            worst = max(worst, float((err / bar[k, t]).max()))
    return worst


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    pdm_observation = install_reference()
    ap = A.DEFAULTS
    while True:
        scenes = O.golden_scenes(seed)
        firsts = [O.observe(s["boxes"], s["types"], s["ego"]) for s in scenes]
        seconds = [O.observe(s["boxes"], s["types"], s["ego"], f["collided"]) for s, f in zip(scenes, firsts)]
        margins = {k: min(o["margins"][k] for o in firsts + seconds) for k in firsts[0]["margins"]}
        crowded = scenes[-1]
        cover = dict(
            caps=all((crowded["types"] == c).sum() - 3 > O.DEFAULTS[O.CAP_FIELD[c]]
                     for c in (O.VEHICLE, O.PEDESTRIAN, O.BICYCLE, O.STATIC)),
            overlap=bool(firsts[-1]["collided"].any()) and not any(f["collided"].any() for f in firsts[:-1]),
            ego_row=all((s["types"] == O.SKIP).any() for s in scenes))
        if O.margins_hold(margins) and all(cover.values()):
            break
        print(f"seed {seed}: margins {margins} cover {cover}: next")
        seed += 1
    data = dict(seed=np.int64(seed), scene_names=np.array([s["name"] for s in scenes]),
                type_names=np.array(sorted(O.TYPE_IDS)), **{f"margin_{k}": np.float64(v) for k, v in margins.items()})
    worst = 0.0
    for s, f64, s64 in zip(scenes, firsts, seconds):
        calls = run_reference(pdm_observation, s, ap)
        fld = O.observe(s["boxes"], s["types"], s["ego"], ft=np.longdouble)
        sld = O.observe(s["boxes"], s["types"], s["ego"], f64["collided"], ft=np.longdouble)
        n = s["name"]
        data[f"{n}_ego"] = s["ego"]
        data[f"{n}_boxes"] = s["boxes"]
        data[f"{n}_type_names"] = np.array([r[8] for r in s["dets"]])
        data[f"{n}_tokens"] = np.array(s["tokens"])
        for c, ((tokens, polys, collided_ids), (o64, old)) in enumerate(zip(calls, ((f64, fld), (s64, sld)))):
            worst = max(worst, compare_call(s, tokens, polys, collided_ids, o64, old))
            assert all(m == tokens[0] for m in tokens)
            data[f"{n}_call{c}_map_tokens"] = np.array(tokens[0])
            data[f"{n}_call{c}_polygons"] = polys
            data[f"{n}_call{c}_collided"] = np.array(collided_ids, dtype=str)
    # the branches the golden must cover, from the reference's own answers
    first_tokens = set(data["crowded_call0_map_tokens"].tolist())
    assert "crowded_reversing" in first_tokens and "crowded_overlapping" in first_tokens
    assert data["crowded_call0_collided"].tolist() == ["crowded_overlapping"]
    assert "crowded_overlapping" not in set(data["crowded_call1_map_tokens"].tolist())
    assert len(data["crowded_call0_map_tokens"]) == 50 + 50 + 25 + 10
    assert LOG["pairs"] > 0
    path = os.path.join(HERE, f"pdm_observation_s{seed}.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, margins {margins}, worst error / bar {worst:.3f}, "
          f"{LOG['queries']} queries, {LOG['pairs']} pairs checked independently")


if __name__ == "__main__":
    main()
