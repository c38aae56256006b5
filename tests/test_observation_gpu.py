"""dd_observe and dd_detections_from_agents on the GPU against the numpy restatement (tests/pdm_observation_ref.py), which
tests/test_observation.py holds to the reference's own PDMObservation.update. Every case runs twice and must be
bit-equal.

Bars, derived, never tuned to the device, printed before each assert:
  order, valid, flags, collided   EQUAL: every decision behind them (a place within a class, the radius, forward or
      reversing, stopped, meeting the ego quad) is taken at a margin the restatement reports, and the inputs keep the
      margins far above the arithmetic's error (distances, radius, speed >= 1e-6; the ego quad >= 5e-3 m).
  heading                         bit-equal: it is the detection's own value.
  speed                           4 ulp: one hypot on each side, each within 2 ulp of the true value.
  a box coordinate                the larger of a floor and 16 x |float64 - longdouble| of the restatement on the case.
      The floor: device and numpy run the same IEEE products and sums in the same order (no contraction), so they can
      differ only through sin, cos, atan2 and hypot, each within 2 ulp of the true value on either side. A coordinate is
      center + (lat cos(h + pi/2) + lon cos h) + delta (cos(track_heading) speed). The lever arm moves by at most 4 ulp
      of the half diagonal (two ulp on each side). The displacement moves by the cosine's 4 ulp, the hypot's 4 ulp and,
      for a reversing agent, by track_heading = atan2(sin, cos)(h + pi) being 4 ulp of pi off, which a cosine's slope of
      at most 1 turns into less than 8 ulp of the displacement: 16 ulp of delta speed <= T_obs dt speed. Both together:
      16 ulp of (half diagonal + speed T_obs dt). Each of the two final additions can then round one spacing of the
      coordinate differently: 2 spacings of the coordinate. There is no share-of-values cap: every value is held.
  the agent head's center         2 spacings of the coordinate + 16 ulp of (|x| + |y|), by the same argument (cos h0 and
      sin h0 once each); its heading, length and width come from the same single operations and are bit-equal.
The chain (observe -> pdm_score, observe -> pdm_closed) against the same calls fed pack_observations /
pack_lead_objects of the restatement's boxes: EQUAL.
"""
import ctypes
import glob
import os
import types

import numpy as np
import pytest
import torch

import pdm_area_ref as A
import pdm_observation_ref as O
import pdm_proposal_ref as Q

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("boxes", "valid", "heading", "speed", "flags", "order", "collided")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def rows_of(scene):
    return scene["dets"]


def device_observe(scenes, collided=None, **kw):
    """observe twice over the scenes (lists of detection rows): bit-equal; numpy arrays."""
    from diffusiondrive_amd import simulate as S
    det = S.pack_detections([rows_of(s) for s in scenes], "cuda")
    ego = dev(np.stack([s["ego"] for s in scenes]))
    col = None if collided is None else dev(np.asarray(collided, dtype=np.uint8))
    a = S.observe(det, ego, collided=col, **kw)
    b = S.observe(det, ego, collided=col, **kw)
    torch.cuda.synchronize()
    pick = lambda o: dict(boxes=o.observations.boxes, valid=o.observations.valid, heading=o.observations.heading,  # noqa: E731
                          speed=o.lead_objects.speed, flags=o.observations.flags, order=o.order, collided=o.collided)
    x, y = pick(a), pick(b)
    for k in FIELDS:
        assert torch.equal(bits(x[k]), bits(y[k])), (k, "two calls differ")
    assert a.observations.boxes.data_ptr() == a.lead_objects.boxes.data_ptr()   # one set of tensors, two views
    assert a.observations.scene_track_off is det.scene_det_off and a.observations.tokens == ()
    out = {k: v.cpu().numpy() for k, v in x.items()}
    out["observed"] = a
    return out


def hold(tag, got, scenes, collided=None, p=None):
    """The device's answer against the restatement's, by the bars of the module docstring."""
    ref = O.observe_scenes(scenes, p, collided_in=collided)
    refld = O.observe_scenes(scenes, p, ft=np.longdouble, collided_in=collided)
    times = O.t_obs(p)
    k = len(ref["order"])
    assert got["boxes"].shape == (k, times, 4, 2) and got["valid"].shape == (k, times)
    m = ref["margins"]
    print(f"{tag}: K = {k}, margins distance {m['distance']:.3e} radius {m['radius']:.3e} angle {m['angle']:.3e} "
          f"speed {m['speed']:.3e} ego {m['ego']:.3e}")
    assert O.margins_hold(m), (tag, m)
    for key in ("order", "valid", "flags", "collided"):
        assert np.array_equal(ref[key], refld[key]), (tag, key, "float64 and longdouble disagree")
    assert np.array_equal(got["order"], ref["order"]), (tag, "order")
    assert np.array_equal(got["valid"], np.repeat(ref["valid"][:, None], times, 1).astype(np.uint8)), (tag, "valid")
    assert np.array_equal(got["flags"], ref["flags"]), (tag, "flags")
    assert np.array_equal(got["collided"], ref["collided"].astype(np.uint8)), (tag, "collided")
    if k == 0:
        return ref
    assert np.array_equal(got["heading"].view(np.int64), ref["heading"].view(np.int64)), (tag, "heading")
    ulps = np.abs(got["speed"] - ref["speed"]) / np.spacing(np.maximum(np.abs(ref["speed"]), np.finfo(float).tiny))
    print(f"{tag}: speed within {float(ulps.max()):.1f} ulp (bar 4)")
    assert (ulps <= 4.0).all(), (tag, "speed")
    flat = np.concatenate([s["boxes"] for s in scenes])
    bar = O.box_bar(ref["boxes"], refld["boxes"], O.reach_of(flat, ref["order"], p))
    err = np.abs(got["boxes"] - ref["boxes"])
    live = ref["valid"]
    if live.any():
        print(f"{tag}: boxes within {float(err[live].max()):.3e} m, worst error / bar "
              f"{float((err[live] / bar[live]).max()):.3f}, least bar {float(bar[live].min()):.3e} m, "
              f"{int(live.sum())} valid tracks")
    assert (err <= bar).all(), (tag, "boxes")
    assert not got["boxes"][~live].any(), (tag, "an invalid track's boxes are not zero")
    return ref


# ---- the golden scenes

@pytest.fixture(scope="module")
def golden():
    path, = glob.glob(os.path.join(HERE, "golden", "pdm_observation_s*.npz"))
    g = np.load(path)
    return g, O.golden_scenes(int(g["seed"]))


@pytest.mark.parametrize("index", [0, 1, 2])
def test_golden_scenes_alone(gpu, golden, index):
    g, scenes = golden
    s = scenes[index]
    collided = None
    for call in range(2):   # the second call takes the first call's collided ids, on the device
        got = device_observe([s], collided)
        hold(f"golden {s['name']} call {call}", got, [s], collided)
        tokens = got["observed"].tokens()[0]
        before = np.zeros(len(tokens), dtype=bool) if collided is None else collided.astype(bool)
        newly = (got["collided"].astype(bool) & ~before)[got["order"]]   # per slot: in the maps, collided after them
        in_maps = [t for k, t in enumerate(tokens) if got["valid"][k, 0] or newly[k]]
        assert in_maps == g[f"{s['name']}_call{call}_map_tokens"].tolist()   # the reference's own token order
        assert sorted(np.array(s["tokens"])[got["collided"].astype(bool)].tolist()) == \
            sorted(g[f"{s['name']}_call{call}_collided"].tolist())
        collided = got["collided"]
    assert index != 2 or collided.any()


def test_golden_scenes_in_one_call_and_reversed(gpu, golden):
    _, scenes = golden
    alone = [device_observe([s]) for s in scenes]
    for tag, pick in (("one call", [0, 1, 2]), ("reversed", [2, 1, 0])):
        got = device_observe([scenes[i] for i in pick])
        hold(f"golden {tag}", got, [scenes[i] for i in pick])
        k = d = 0
        for i in pick:   # scene independence: the same bits as alone, the order shifted by the scene's first detection
            n = len(scenes[i]["types"])
            for key in ("boxes", "valid", "heading", "speed", "flags"):
                assert np.array_equal(got[key][k:k + n].view(np.uint8), alone[i][key].view(np.uint8)), (tag, i, key)
            assert np.array_equal(got["order"][k:k + n], alone[i]["order"] + d), (tag, i)
            assert np.array_equal(got["collided"][d:d + n], alone[i]["collided"]), (tag, i)
            k, d = k + n, d + n


@pytest.mark.parametrize("case", O.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(gpu, case):
    name, scene, p, collided, expected = case
    over = None if p is None else {k: v for k, v in p.items() if v != O.DEFAULTS[k]}
    got = device_observe([scene], collided, params=over)
    hold(f"hand {name}", got, [scene], collided, p)
    O.check_hand_case(name, got, expected, scene, p)


# ---- sizes: the chunk of 256 rows, one wavefront, the caps

def crowd(seed, counts, fill=0, pose=(40.0, -20.0, 1.1)):
    """A scene of ``counts[type name]`` objects 7 .. 95 m from the ego center, and ``fill`` rows that are dropped before
    the selection (beyond the radius, or EGO-typed)."""
    rng = np.random.default_rng(seed)
    s = O.seeded_scene(rng, f"crowd{seed}", pose, counts, far=0, ego_row=False)
    dets = list(s["dets"])
    cx, cy = O.ego_center(s["ego"])
    for i in range(fill):
        r, phi = rng.uniform(105.0, 140.0), rng.uniform(-np.pi, np.pi)
        dets.append(O._row(f"fill_{i}", cx + r * np.cos(phi), cy + r * np.sin(phi), 0.3, 4.0, 1.8, 1.0, 0.5,
                           "EGO" if i % 3 == 0 else "VEHICLE"))
    rng.shuffle(dets)
    return O.scene_arrays(dict(name=s["name"], ego=s["ego"], dets=[tuple(d) for d in dets]))


SIZES = [
    (0, {}, 0), (1, dict(VEHICLE=1), 0),
    (63, dict(VEHICLE=50, BICYCLE=10, PEDESTRIAN=3), 0),               # vehicles and bicycles at their caps
    (64, dict(VEHICLE=51, BICYCLE=11, BARRIER=2), 0),                  # one over
    (65, dict(PEDESTRIAN=25, TRAFFIC_CONE=40), 0),                     # pedestrians at the cap
    (65, dict(PEDESTRIAN=26, GENERIC_OBJECT=39), 0),                   # one over
    (257, dict(TRAFFIC_CONE=30, BARRIER=20, VEHICLE=51, PEDESTRIAN=26, BICYCLE=11), 119),   # static at the cap
    (257, dict(TRAFFIC_CONE=30, BARRIER=21, VEHICLE=50, PEDESTRIAN=25, BICYCLE=10), 121),   # static one over
]


@pytest.mark.parametrize("size, counts, fill", SIZES, ids=[f"D{s[0]}_{i}" for i, s in enumerate(SIZES)])
def test_scene_sizes_and_caps(gpu, size, counts, fill):
    scene = crowd(100 + size + len(counts), counts, fill)
    assert len(scene["types"]) == size
    got = device_observe([scene])
    ref = hold(f"D = {size}", got, [scene])
    kept = np.bincount(scene["types"][ref["order"]][ref["valid"]], minlength=4)
    want = {O.VEHICLE: counts.get("VEHICLE", 0), O.PEDESTRIAN: counts.get("PEDESTRIAN", 0),
            O.BICYCLE: counts.get("BICYCLE", 0),
            O.STATIC: sum(v for k, v in counts.items() if k in O.STATIC_NAMES)}
    for cls, n in want.items():
        assert kept[cls] == min(n, O.DEFAULTS[O.CAP_FIELD[cls]]), (cls, kept)


def test_scene_counts(gpu):
    a, b = crowd(7, dict(VEHICLE=4, TRAFFIC_CONE=2)), crowd(8, dict(PEDESTRIAN=3, BICYCLE=2), fill=2)
    empty = O.scene_arrays(dict(name="empty", ego=a["ego"].copy(), dets=[]))
    hold("G = 3, the middle scene empty", device_observe([a, empty, b]), [a, empty, b])
    many = [crowd(300 + i, dict(VEHICLE=1 + i % 3, CZONE_SIGN=i % 2, PEDESTRIAN=i % 4),
                  pose=(10.0 * i, -3.0 * i, 0.1 * i)) for i in range(65)]
    hold("G = 65", device_observe(many), many)
    hold("every scene empty", device_observe([empty, empty]), [empty, empty])


@pytest.mark.parametrize("over", [dict(sample_res=1), dict(num_samples=60, sample_res=3), dict(map_radius=0.0),
                                  dict(max_vehicles=0, max_pedestrians=0, max_bicycles=0, max_static=0),
                                  dict(max_vehicles=0), dict(max_static=1, max_bicycles=3, stopped_speed=0.5, dt=0.25)],
                         ids=["res1", "60x3", "radius0", "caps0", "vehicles0", "mixed"])
def test_non_default_parameters(gpu, golden, over):
    _, scenes = golden
    p = O.params(**over)
    got = device_observe(scenes, params=over)
    ref = hold(f"params {over}", got, scenes, p=p)
    assert got["boxes"].shape[1] == p["num_samples"] + p["sample_res"]
    if "map_radius" in over:
        assert ref["valid"].sum() > O.observe_scenes(scenes)["valid"].sum()   # the far rows are kept now
    if over.get("max_static") == 0:
        assert not ref["valid"].any() and not got["collided"].any()


def test_collided_fed_back_frees_the_slot(gpu):
    name, scene, p, _, _ = [c for c in O.hand_cases() if c[0] == "overlap_counts"][0]
    first = device_observe([scene])
    hold("feedback first", first, [scene])
    second = device_observe([scene], first["collided"])
    hold("feedback second", second, [scene], first["collided"])
    valid = lambda o: set(o["order"][o["valid"][:, 0].astype(bool)].tolist())   # noqa: E731
    assert first["collided"].tolist() == [1] + [0] * 50 and second["collided"].tolist() == first["collided"].tolist()
    assert valid(first) == set(range(1, 50)) and valid(second) == set(range(1, 51))


# ---- the agent head

@pytest.mark.parametrize("scenes", [1, 3])
def test_detections_from_agent_head(gpu, scenes):
    from diffusiondrive_amd import simulate as S
    rng = np.random.default_rng(40 + scenes)
    states = np.stack([rng.uniform(-32.0, 32.0, (scenes, 30)), rng.uniform(-32.0, 32.0, (scenes, 30)),
                       rng.uniform(-np.pi, np.pi, (scenes, 30)), rng.uniform(0.5, 6.0, (scenes, 30)),
                       rng.uniform(0.4, 2.5, (scenes, 30))], axis=-1).astype(np.float32)
    labels = rng.normal(0.0, 2.0, (scenes, 30)).astype(np.float32)
    labels[0, :4] = (0.0, np.nextafter(np.float32(0.0), np.float32(1.0)), 3.0, -3.0)   # both sides of the threshold
    states[0, 5, 1] = np.nan
    states[0, 6, 3] = 0.0
    states[0, 7, 4] = -1.0
    states[0, 8, 2] = np.inf
    labels[0, 4:9] = (2.0, 4.0, 4.0, 4.0, 4.0)
    labels[0, 9] = np.nan
    ego = np.zeros((scenes, 11))
    ego[:, :3] = [(664431.37 + 30.0 * i, 3997675.12 - 11.0 * i, 2.3 - 1.7 * i) for i in range(scenes)]
    for threshold in (0.0, 1.5):
        a = S.detections_from_agent_head(dev(states), dev(labels), dev(ego), threshold)
        b = S.detections_from_agent_head(dev(states), dev(labels), dev(ego), threshold)
        torch.cuda.synchronize()
        assert torch.equal(bits(a.boxes), bits(b.boxes)) and torch.equal(a.type, b.type)
        assert a.scene_det_off.tolist() == [30 * i for i in range(scenes + 1)]
        assert a.tokens[0][:2] == ("agent_0", "agent_1") and len(a.tokens) == scenes
        want, kinds = O.detections_from_agents(states, labels, ego, threshold)
        wantld, _ = O.detections_from_agents(states, labels, ego, threshold, ft=np.longdouble)
        got = a.boxes.cpu().numpy()
        assert np.array_equal(a.type.cpu().numpy(), kinds)   # EQUAL
        assert kinds[:10].tolist() == ([255, 0, 0, 255] if threshold == 0.0 else [255, 255, 0, 255]) + [0] + [255] * 5
        reach = np.abs(states[..., 0].astype(np.float64)) + np.abs(states[..., 1].astype(np.float64))
        reach = np.where(np.isfinite(reach), reach, 0.0).reshape(-1, 1)
        bar = np.maximum(2.0 * np.spacing(np.abs(want[:, :2])) + 16.0 * np.spacing(reach),
                         16.0 * np.abs(want[:, :2] - wantld[:, :2].astype(np.float64)))
        err = np.abs(got[:, :2] - want[:, :2])
        print(f"agent head B = {scenes} threshold {threshold}: {int((kinds == 0).sum())} vehicles, centers within "
              f"{float(err.max()):.3e} m, worst error / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all()
        assert np.array_equal(got[:, 2:].view(np.int64), want[:, 2:].view(np.int64))   # heading, sizes, velocity: bits
    # through observe: a zero-velocity agent is flagged stopped and forecast in place
    seen = S.observe(a, dev(ego))
    torch.cuda.synchronize()
    boxes, valid = seen.observations.boxes.cpu().numpy(), seen.observations.valid.cpu().numpy().astype(bool)
    assert valid.any() and (boxes[valid[:, 0]] == boxes[valid[:, 0]][:, :1]).all()
    flags = seen.observations.flags.cpu().numpy()
    assert (flags[valid[:, 0]] == (O.FLAG_STOPPED | O.FLAG_AGENT)).all()
    scene_list = [O.scene_arrays(dict(name=f"head{i}", ego=ego[i], dets=[
        O._row(f"agent_{j}", *want[30 * i + j], "VEHICLE" if kinds[30 * i + j] == 0 else "EGO")
        for j in range(30)])) for i in range(scenes)]
    ref = O.observe_scenes(scene_list)
    assert np.array_equal(seen.order.cpu().numpy(), ref["order"]) and np.array_equal(valid[:, 0], ref["valid"])
    me = types.SimpleNamespace(_transfuser_model=types.SimpleNamespace(device=torch.cuda.current_device()))
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    via = DiffusionDriveAgent.observe_predictions(me, dict(agent_states=torch.from_numpy(states),
                                                           agent_labels=torch.from_numpy(labels)),
                                                  torch.from_numpy(ego), threshold=1.5)
    assert torch.equal(bits(via.observations.boxes), bits(seen.observations.boxes))
    assert torch.equal(via.order, seen.order)


# ---- the chain

def detection_rows(scene):
    """The chain scenes' tracks as detections at t = 0 with a constant velocity along the heading; the token hit
    before is marked in the returned ``collided``."""
    rows, collided = [], []
    for tr in scene["tracks"]:
        b = tr["boxes"][int(np.argmax(tr["valid"]))]
        center = b.mean(0)
        length, width = np.hypot(*(b[0] - b[1])), np.hypot(*(b[0] - b[3]))
        v = tr["speed"] or 0.0
        rows.append(O._row(tr["token"], center[0], center[1], tr["heading"], length, width, v * np.cos(tr["heading"]),
                           v * np.sin(tr["heading"]), tr["kind"]))
        collided.append(tr["token"] in scene["collided"])
    return rows, collided


def restated_items(scene_dets, ref, g, tokens):
    """The restatement's slots of scene g as the list forms pack_observations / pack_lead_objects take. EVERY slot is
    listed, the invalid ones with an all-false mask, so that the object indices are the device's."""
    lo, hi = int(ref["off"][g]), int(ref["off"][g + 1])
    obs, lead = [], []
    for k in range(lo, hi):
        d = int(ref["order"][k]) - lo
        mask = np.full(ref["boxes"].shape[1], bool(ref["valid"][k]))
        agent, stopped = bool(ref["flags"][k] & O.FLAG_AGENT), bool(ref["flags"][k] & O.FLAG_STOPPED)
        obs.append((tokens[d], (ref["boxes"][k], mask), float(ref["heading"][k]), agent, stopped))
        lead.append(obs[-1] + (float(ref["speed"][k]),))
    return obs, lead


def test_chain_matches_the_host_packed_chain(gpu):
    from diffusiondrive_amd import simulate as S
    g = np.load(os.path.join(HERE, "golden", "pdm_proposals_s3.npz"), allow_pickle=False)
    all_scenes = Q.golden_scenes(int(g["seed"]))
    names = ("origin", "far", "light")
    scenes = [dict(all_scenes[k], tracks=[t for t in all_scenes[k]["tracks"] if not t["token"].startswith("cut_")])
              for k in names]
    maps = [A.seeded_map(int(g["seed"]) + i, tuple(s["ego"][:3]), lanes=3)[0] for i, s in enumerate(scenes)]
    lines = [s["paths"][0]["xyh"][:, :2] for s in scenes]
    dets, collided = zip(*(detection_rows(s) for s in scenes))
    obs_scenes = [O.scene_arrays(dict(name=n, ego=s["ego"], dets=list(d))) for n, s, d in zip(names, scenes, dets)]
    flat_collided = np.concatenate([np.asarray(c, dtype=np.uint8) for c in collided])
    rings = [s["rings"] for s in scenes]
    ego = dev(np.stack([s["ego"] for s in scenes]))
    targets = np.stack([s["targets"] for s in scenes])
    paths = S.pack_paths([[q["xyh"] for q in s["paths"]] for s in scenes], "cuda")

    got = device_observe(obs_scenes, flat_collided, stop_polygons=rings)
    ref = hold("chain scenes", got, obs_scenes, flat_collided)
    seen = got["observed"]
    assert seen.ignored_rings == ((), (), ()) and seen.ring_tokens == (("red_light_0",),) * 3
    assert all(t[-1] == "red_light_0" and len(t) == len(d) + 1 for t, d in zip(seen.tokens(), dets))
    items = [restated_items(d, ref, i, [r[0] for r in d]) for i, d in enumerate(dets)]
    host_obs = S.pack_observations([i[0] for i in items], "cuda")
    host_lead = S.pack_lead_objects([i[1] for i in items], "cuda", stop_polygons=rings)
    assert host_obs.boxes.shape == seen.observations.boxes.shape

    mine = S.generate_proposals(paths, seen.lead_objects, ego, targets, details=True)
    theirs = S.generate_proposals(paths, host_lead, ego, targets, details=True)
    assert torch.equal(mine.lead_index, theirs.lead_index)                                   # EQUAL
    assert int((mine.lead_index >= 0).sum()) > 0
    a = S.pdm_closed(paths, seen.lead_objects, ego, targets, maps, seen.observations, lines)
    again = S.pdm_closed(paths, seen.lead_objects, ego, targets, maps, seen.observations, lines)
    b = S.pdm_closed(paths, host_lead, ego, targets, maps, host_obs, lines)
    torch.cuda.synchronize()
    print("pdm_closed best", a.best_index.tolist(), "host-packed", b.best_index.tolist())
    for name in S.PDMScores._fields:
        x, y, z = getattr(a.scores, name), getattr(b.scores, name), getattr(again.scores, name)
        assert torch.equal(bits(x), bits(z)), (name, "two calls differ")
        print(f"pdm_closed {name}: equal {bool(torch.equal(bits(x), bits(y)))}, max |diff| "
              f"{float((x.double() - y.double()).abs().nan_to_num(0.0).max()):.3e}")
    for name in S.PDMScores._fields:
        assert torch.equal(bits(getattr(a.scores, name)), bits(getattr(b.scores, name))), name  # EQUAL
    assert torch.equal(a.best_index, b.best_index)                                           # EQUAL
    assert len(set(a.best_index.tolist())) > 1 or float(a.scores.score.max()) > 0.0
    # pdm_score of given states against the planner's own observation and the host-packed one
    x = S.pdm_score(b.states, maps, seen.observations, lines, progress_reference=b.progress_reference)
    y = S.pdm_score(b.states, maps, host_obs, lines, progress_reference=b.progress_reference)
    for name in S.PDMScores._fields:
        assert torch.equal(bits(getattr(x, name)), bits(getattr(y, name))), name             # EQUAL
    me = types.SimpleNamespace(_transfuser_model=types.SimpleNamespace(device=torch.cuda.current_device()))
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    via = DiffusionDriveAgent.observe(me, [list(d) for d in dets], ego.cpu(), collided=dev(flat_collided),
                                      stop_polygons=rings)
    assert torch.equal(bits(via.observations.boxes), bits(seen.observations.boxes))


# ---- rejections

GUARD = 64


def call_entry(lib, **over):
    """dd_observe directly on a two-row scene; ``over`` replaces arguments or struct fields. Outputs are pre-filled."""
    from diffusiondrive_amd import _lib, simulate as S
    boxes = dev(np.array([[20.0, 3.0, 0.1, 4.6, 1.9, 2.0, 0.0], [30.0, -3.0, 0.2, 0.5, 0.5, 0.0, 0.0]]))
    kinds, off = dev(np.array([0, 3], dtype=np.uint8)), dev(np.array([0, 2], dtype=np.int32))
    ego = dev(np.zeros((1, 11)))
    det = _lib.DDDetections(boxes.data_ptr(), kinds.data_ptr(), off.data_ptr(), None, 2)
    p, ap = S.default_observe_params(lib), S.default_area_params(lib)
    for name, value in over.items():
        for struct in (det, p, ap):
            if name in dict(struct._fields_):
                setattr(struct, name, value)
    # T_obs = 52: every output is followed by a guard of GUARD values that no call may touch
    keep = call_entry.keep = dict(
        inputs=(boxes, kinds, off, ego), work=torch.full((lib.dd_observe_work(2) + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
        out_boxes=torch.full((2 * 52 * 8 + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
        out_valid=torch.full((2 * 52 + GUARD,), 7, dtype=torch.uint8, device="cuda"),
        out_heading=torch.full((2 + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
        out_speed=torch.full((2 + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
        out_flags=torch.full((2 + GUARD,), 7, dtype=torch.uint8, device="cuda"),
        out_order=torch.full((2 + GUARD,), -7, dtype=torch.int32, device="cuda"),
        out_collided=torch.full((2 + GUARD,), 7, dtype=torch.uint8, device="cuda"))
    a = dict(det=ctypes.byref(det), ego=ego.data_ptr(), G=1, params=ctypes.byref(p), ap=ctypes.byref(ap))
    a.update({k: v.data_ptr() for k, v in keep.items() if k != "inputs"})
    if over.get("misaligned"):
        a["out_boxes"] += 8
    if over.get("alias"):
        det.collided_in = a["out_collided"]
    a.update({k: v for k, v in over.items() if k in a})
    rc = lib.dd_observe(a["det"], a["ego"], a["G"], a["params"], a["ap"], a["work"], a["out_boxes"], a["out_valid"],
                        a["out_heading"], a["out_speed"], a["out_flags"], a["out_order"], a["out_collided"],
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    untouched = all(bool((v == (-7 if v.dtype != torch.uint8 else 7)).all()) for k, v in keep.items() if k != "inputs")
    return rc, (lib.dd_last_error() or b"").decode(), untouched, keep


def test_rejections_launch_nothing(gpu):
    from diffusiondrive_amd import simulate as S
    lib = gpu
    rc, msg, untouched, keep = call_entry(lib)
    assert rc == 0 and not untouched, msg
    assert keep["out_order"][:2].tolist() == [1, 0] and bool((keep["out_valid"][:104] == 1).all())   # cone, vehicle
    assert not bool((keep["out_boxes"][:832] == -7.0).any()) and keep["out_collided"][:2].tolist() == [0, 0]
    for name, t in keep.items():   # nothing behind the outputs is written
        assert name == "inputs" or bool((t[-GUARD:] == (7 if t.dtype == torch.uint8 else -7)).all()), name
    nan, inf = float("nan"), float("inf")
    cases = [(dict(G=0), "G = 0"), (dict(det=None), "det is null"), (dict(ego=None), "ego_states is null"),
             (dict(params=None), "params is null"), (dict(ap=None), "area_params is null"),
             (dict(num_dets=-1), "num_dets"), (dict(scene_det_off=None), "scene_det_off"),
             (dict(boxes=None), "dd_detections.boxes"), (dict(type=None), "dd_detections.type"),
             (dict(work=None), "work is null"), (dict(out_boxes=None), "out_boxes"), (dict(out_valid=None), "out_valid"),
             (dict(out_heading=None), "out_heading"), (dict(out_speed=None), "out_speed"),
             (dict(out_flags=None), "out_flags"), (dict(out_order=None), "out_order"),
             (dict(out_collided=None), "out_collided"), (dict(misaligned=True), "16-byte"),
             (dict(alias=True), "collided_in is out_collided"),
             (dict(sample_res=0), "sample_res"), (dict(sample_res=51), "sample_res"),
             (dict(num_samples=40, sample_res=2), "below 50"), (dict(num_samples=0), "num_samples"),
             (dict(max_vehicles=-1), "max_vehicles"), (dict(max_pedestrians=-1), "max_pedestrians"),
             (dict(max_bicycles=-2), "max_bicycles"), (dict(max_static=-1), "max_static"),
             (dict(dt=-0.1), "dd_observe_params.dt"), (dict(dt=nan), "dd_observe_params.dt"),
             (dict(map_radius=-1.0), "map_radius"), (dict(map_radius=inf), "map_radius"),
             (dict(stopped_speed=nan), "stopped_speed"), (dict(half_length=-1.0), "half_length"),
             (dict(half_width=inf), "half_width"), (dict(rear_axle_to_center=nan), "rear_axle_to_center")]
    for over, text in cases:
        rc, msg, untouched, _ = call_entry(lib, **over)
        assert rc == -1 and text in msg and msg.startswith("dd_observe: "), (over, rc, msg)
        assert untouched, over
    det = S.pack_detections([[("a", 20.0, 3.0, 0.1, 4.6, 1.9, 2.0, 0.0, "VEHICLE")]], "cuda")
    ego = dev(np.zeros((1, 11)))
    with pytest.raises(ValueError, match="unknown observe parameter"):
        S.observe(det, ego, params=dict(radius=1.0))
    with pytest.raises(ValueError, match="sample_res"):
        S.observe(det, ego, params=dict(sample_res=0))
    with pytest.raises(ValueError, match="detections hold"):
        S.observe(det, torch.cat([ego, ego]))
    with pytest.raises(ValueError, match="collided must be"):
        S.observe(det, ego, collided=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="stop_polygons holds"):
        S.observe(det, ego, stop_polygons=[[], []])
    f = dev(np.zeros((1, 30, 5), dtype=np.float32))
    rc = lib.dd_detections_from_agents(f.data_ptr(), None, ego.data_ptr(), 1, 30, 0.0, None, None, None, None)
    assert rc == -1 and b"agent_labels is null" in lib.dd_last_error()
    rc = lib.dd_detections_from_agents(f.data_ptr(), f.data_ptr(), ego.data_ptr(), 0, 30, 0.0, f.data_ptr(),
                                       f.data_ptr(), f.data_ptr(), None)
    assert rc == -1 and b"B = 0" in lib.dd_last_error()
    with pytest.raises(ValueError, match="agent_labels must be"):
        S.detections_from_agent_head(f, dev(np.zeros((1, 29), dtype=np.float32)), ego)
