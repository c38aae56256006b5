"""CPU tests of PDM's forecasted observation: the numpy restatement (tests/pdm_observation_ref.py) against the golden
the reference's own PDMObservation.update and PDMObjectManager wrote (tests/golden/make_observation_golden.py), the hand
cases, pack_detections' checks and the rule by which a red light that holds the ego is ignored.

Bars. Token order and collided ids are EQUAL. A box coordinate is held within the bar of test_observation_gpu.py's
docstring (2 spacings of the coordinate + 16 ulp of the track's reach, or 16 x |float64 - longdouble| of the restatement
where that is larger); the golden's boxes come from the same float64 operations in the same order, so the error seen is
0 and the bar only says how far it may move."""
import glob
import os
import types

import numpy as np
import pytest

import pdm_area_ref as A
import pdm_observation_ref as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "pdm_observation_s*.npz")))


@pytest.fixture(scope="module")
def golden():
    assert len(GOLDEN) == 1, GOLDEN
    return np.load(GOLDEN[0])


def _scene(golden, name):
    return dict(name=name, ego=golden[f"{name}_ego"], boxes=golden[f"{name}_boxes"],
                types=np.array([O.TYPE_IDS[t] for t in golden[f"{name}_type_names"]], dtype=np.uint8),
                tokens=golden[f"{name}_tokens"].tolist())


def test_golden_inputs_are_the_seeded_scenes(golden):
    scenes = O.golden_scenes(int(golden["seed"]))
    assert [s["name"] for s in scenes] == golden["scene_names"].tolist() == ["origin", "far", "crowded"]
    for s in scenes:
        g = _scene(golden, s["name"])
        assert np.array_equal(s["boxes"], g["boxes"]) and np.array_equal(s["types"], g["types"])
        assert s["tokens"] == g["tokens"] and np.array_equal(s["ego"], g["ego"])
    assert abs(scenes[1]["ego"][0]) > 6e5 and abs(scenes[1]["ego"][1]) > 3.9e6


@pytest.mark.parametrize("name", ["origin", "far", "crowded"])
def test_restatement_reproduces_the_reference(golden, name):
    s = _scene(golden, name)
    p = O.DEFAULTS
    collided = None
    for call in range(2):
        o64 = O.observe(s["boxes"], s["types"], s["ego"], collided)
        old = O.observe(s["boxes"], s["types"], s["ego"], collided, ft=np.longdouble)
        for key in ("order", "valid", "kept", "flags", "collided"):
            assert np.array_equal(o64[key], old[key]), (key, "float64 and longdouble disagree")
        tokens = golden[f"{name}_call{call}_map_tokens"].tolist()
        polys = golden[f"{name}_call{call}_polygons"]
        ids = golden[f"{name}_call{call}_collided"].tolist()
        kept = [s["tokens"][d] for d, k in zip(o64["order"], o64["kept"]) if k]
        assert kept == tokens, "token order"   # EQUAL
        assert sorted(s["tokens"][d] for d in np.flatnonzero(o64["collided"])) == sorted(ids), "collided ids"   # EQUAL
        assert polys.shape == (p["num_samples"] // p["sample_res"] + 1, len(tokens), 4, 2)
        bar = O.box_bar(o64["boxes"], old["boxes"], O.reach_of(s["boxes"], o64["order"]))
        worst, worst_bar = 0.0, np.inf
        for t in range(O.t_obs()):   # observation[t] is map t // sample_res
            ref = polys[t // p["sample_res"]]
            for k in np.flatnonzero(o64["valid"]):
                err = np.abs(o64["boxes"][k, t] - ref[k])
                worst, worst_bar = max(worst, float(err.max())), min(worst_bar, float(bar[k, t].min()))
                assert (err <= bar[k, t]).all(), (name, call, t, k, err.max(), bar[k, t].min())
        print(f"{name} call {call}: {len(tokens)} tokens, worst box error {worst:.3e} m, least bar {worst_bar:.3e} m")
        # a newly collided track is in the reference's maps (it counted toward its cap) and invalid here
        assert set(np.flatnonzero(o64["kept"] & ~o64["valid"]).tolist()) == \
            {k for k, d in enumerate(o64["order"]) if o64["collided"][d] and o64["kept"][k]}
        collided = o64["collided"]


def test_golden_margins_and_branches(golden):
    assert golden["margin_distance"] >= O.MIN_DISTANCE_GAP and golden["margin_radius"] >= O.MIN_RADIUS_GAP
    assert golden["margin_angle"] >= O.MIN_ANGLE_GAP and golden["margin_speed"] >= O.MIN_SPEED_GAP
    assert golden["margin_ego"] >= O.MIN_EGO_GAP
    scenes = [_scene(golden, n) for n in ("origin", "far", "crowded")]
    outs = [O.observe(s["boxes"], s["types"], s["ego"]) for s in scenes]
    margins = {k: min(o["margins"][k] for o in outs) for k in outs[0]["margins"]}
    assert O.margins_hold(margins), margins   # the restatement's own margins on the same inputs
    crowded, out = scenes[2], outs[2]
    p = O.DEFAULTS
    typed = crowded["types"][out["order"]]
    for cls in O.CLASS_ORDER:   # every cap is hit: more rows of the class are in range than it keeps
        assert (typed[out["kept"]] == cls).sum() == p[O.CAP_FIELD[cls]], cls
        assert (typed[~out["kept"]] == cls).sum() > 0, cls
    tokens = crowded["tokens"]
    rev = out["order"].tolist().index(tokens.index("crowded_reversing"))
    b = crowded["boxes"][tokens.index("crowded_reversing")]
    move = out["boxes"][rev, -1, 0] - out["boxes"][rev, 0, 0]
    assert out["valid"][rev] and move @ b[5:7] > 0 and move @ np.array([np.cos(b[2]), np.sin(b[2])]) < 0   # backwards
    assert out["collided"][tokens.index("crowded_overlapping")]
    assert (crowded["types"] == O.SKIP).any()                                      # an EGO row
    far = np.hypot(*(crowded["boxes"][:, :2] - np.array(O.ego_center(crowded["ego"]))).T) > p["map_radius"]
    assert far.any() and not out["kept"][np.isin(out["order"], np.flatnonzero(far))].any()   # beyond the radius
    flags = out["flags"][out["kept"]]
    assert {int(f) for f in flags} == {O.FLAG_STOPPED, O.FLAG_AGENT, O.FLAG_STOPPED | O.FLAG_AGENT}
    # the slot order: static, vehicles, pedestrians, bicycles, each by distance
    kept_types = typed[out["kept"]].tolist()
    assert kept_types == sorted(kept_types, key=O.CLASS_ORDER.index)


@pytest.mark.parametrize("case", O.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, scene, p, collided, expected = case
    for ft in (np.float64, np.longdouble):
        out = O.observe(scene["boxes"], scene["types"], scene["ego"], collided, p, ft=ft)
        O.check_hand_case(name, out, expected, scene, p)


def test_agent_head_restatement():
    states = np.zeros((2, 4, 5), dtype=np.float32)
    states[..., 3:] = (4.0, 2.0)
    states[0, 0, :3] = (10.0, 2.0, 0.5)
    states[0, 1, 0] = np.nan
    states[0, 2, 3] = 0.0
    labels = np.array([[1.0, 1.0, 1.0, -1.0], [0.0, 0.5, 2.0, 3.0]], dtype=np.float32)
    ego = np.zeros((2, 11))
    ego[0, :3] = (100.0, 50.0, np.pi / 2)
    boxes, kinds = O.detections_from_agents(states, labels, ego)
    assert kinds.tolist() == [O.VEHICLE, O.SKIP, O.SKIP, O.SKIP, O.SKIP, O.VEHICLE, O.VEHICLE, O.VEHICLE]
    assert np.allclose(boxes[0], [98.0, 60.0, np.pi / 2 + 0.5, 4.0, 2.0, 0.0, 0.0], atol=1e-12)
    assert not boxes[1:5].any()


# ---- the host side of diffusiondrive_amd.simulate: no library is loaded

def _rows():
    return [("a", 1.0, 2.0, 0.1, 4.0, 2.0, 1.0, 0.0, "VEHICLE"), ("b", 5.0, 2.0, 0.1, 0.5, 0.5, 0.0, 0.0, "TRAFFIC_CONE"),
            ("c", 0.0, 0.0, 0.0, 5.0, 2.0, 3.0, 0.0, "EGO")]


def test_pack_detections_packs_lists_and_ducks():
    from diffusiondrive_amd import simulate as S
    duck = []
    for token, x, y, h, length, width, vx, vy, name in _rows():
        obj = types.SimpleNamespace(track_token=token, center=types.SimpleNamespace(x=x, y=y, heading=h),
                                    box=types.SimpleNamespace(length=length, width=width),
                                    tracked_object_type=types.SimpleNamespace(name=name))
        if name != "TRAFFIC_CONE":
            obj.velocity = types.SimpleNamespace(x=vx, y=vy)
        duck.append(obj)
    tracks = types.SimpleNamespace(tracked_objects=types.SimpleNamespace(tracked_objects=duck))
    packed = S.pack_detections([_rows(), tracks, []], "cpu")
    assert packed.scene_det_off.tolist() == [0, 3, 6, 6] and packed.type.tolist() == [0, 3, 255] * 2
    assert np.array_equal(packed.boxes[:3].numpy(), packed.boxes[3:].numpy())
    assert np.array_equal(packed.boxes[:3].numpy(), np.array([r[1:8] for r in _rows()]))
    assert packed.tokens == (("a", "b", "c"), ("a", "b", "c"), ())


@pytest.mark.parametrize("column, value, word", [(1, np.nan, "non-finite"), (6, np.inf, "non-finite"),
                                                 (4, 0.0, "non-positive"), (5, -1.0, "non-positive"),
                                                 (0, "b", "duplicate token"), (8, "TRUCK", "unknown type name")])
def test_pack_detections_rejects(column, value, word):
    from diffusiondrive_amd import simulate as S
    rows = [list(r) for r in _rows()]
    rows[0][column] = value
    with pytest.raises(ValueError, match=word):
        S.pack_detections([[tuple(r) for r in rows]], "cpu")
    with pytest.raises(ValueError, match="expected"):
        S.pack_detections([[("a", 1.0)]], "cpu")


def test_ring_that_holds_the_ego_is_ignored():
    from diffusiondrive_amd import simulate as S
    ap = A.DEFAULTS
    ego = np.array([[3.0, -2.0, 0.4] + [0.0] * 8])
    quad = S.ego_quad(ego[0, :3], ap["half_length"], ap["half_width"], ap["rear_axle_to_center"])
    assert np.abs(quad - O.ego_quad(ego[0])).max() == 0.0
    center = quad.mean(0)
    square = lambda r: center + r * np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])  # noqa: E731
    holds = square(10.0)                       # the whole quad strictly inside
    touches = quad[0] + np.array([[0.0, 0.0], [5.0, 0.0], [5.0, 5.0], [0.0, 5.0]]) @ \
        np.array([[np.cos(0.4), np.sin(0.4)], [-np.sin(0.4), np.cos(0.4)]])   # shares the front-left corner only
    cuts = square(2.0)                         # overlaps the quad without holding it
    apart = square(3.0) + 100.0
    closed = np.concatenate([holds, holds[:1]])   # shapely's closed ring
    notch = np.array([[-10.0, -10.0], [10.0, -10.0], [10.0, 10.0], [0.0, 10.0], [0.0, -1.0], [-0.2, -1.0], [-0.2, 10.0],
                      [-10.0, 10.0]]) + center   # every corner inside, but a slot of the ring cuts through the quad
    assert S.ring_holds_quad(holds, quad) and S.ring_holds_quad(closed, quad)
    assert not S.ring_holds_quad(touches, quad) and not S.ring_holds_quad(cuts, quad)
    assert not S.ring_holds_quad(apart, quad) and not S.ring_holds_quad(notch, quad)
    kept, names, ignored = S.split_stop_polygons([[holds, touches, apart, cuts]], ego, ap["half_length"],
                                                 ap["half_width"], ap["rear_axle_to_center"])
    assert ignored == (("red_light_0",),) and names == (("red_light_1", "red_light_2", "red_light_3"),)
    assert len(kept[0]) == 3 and np.array_equal(kept[0][0], touches)
