"""numpy restatement of PDM's forecasted observation from raw detections (dd_observe, include/ddmi.h) and of the agent
head's detections (dd_detections_from_agents).

Restates, with every quirk kept:
  PDMObservation.update / _get_object_manager      pdm_planner/observation/pdm_observation.py:105-205, 262-281 (the ego,
                                far and previously collided objects dropped; `self._map_radius and ...`: radius 0 = no
                                filter; the maps at sample_res (t // sample_res) through _global_to_local_idcs; the
                                token order static + dynamic; the tracks that meet the ego quad at t = 0 appended to the
                                collided ids AFTER the maps are built, so they counted toward their cap)
  PDMObjectManager.add_object / get_nearest_objects  observation/pdm_object_manager.py:50-217 (a reversing agent is
                                forecast backwards along its own axis; ((c - p) ** 2).sum() ** 0.5; the caps 50 / 25 / 10
                                / 50; the dynamic classes in the order vehicle, pedestrian, bicycle)
Quoted from memory of nuPlan, which is not part of this tree: OrientedBox.all_corners (front-left, rear-left,
rear-right, front-right by translate_longitudinally_and_laterally, the formula of tests/pdm_area_ref.py:60-69),
Point2D.distance_to (hypot of the differences), velocity.magnitude() (hypot). np.argsort is an unstable introsort: a tie
goes to the lower detection index here, and the inputs keep their distances apart.

Runs in float64 and in numpy.longdouble (``ft``) and reports its own margins: how far every decision it takes is from
going the other way. tests/golden/make_observation_golden.py runs the reference's own code on the seeded scenes below;
tests/test_observation.py holds this file to that golden.
"""
import numpy as np

import pdm_area_ref as A

VEHICLE, PEDESTRIAN, BICYCLE, STATIC, SKIP = 0, 1, 2, 3, 255
TYPE_IDS = dict(VEHICLE=VEHICLE, PEDESTRIAN=PEDESTRIAN, BICYCLE=BICYCLE, TRAFFIC_CONE=STATIC, BARRIER=STATIC,
                CZONE_SIGN=STATIC, GENERIC_OBJECT=STATIC, EGO=SKIP)
FLAG_STOPPED, FLAG_AGENT = 1, 2
DEFAULTS = dict(map_radius=100.0, dt=0.1, num_samples=50, sample_res=2, max_vehicles=50, max_pedestrians=25,
                max_bicycles=10, max_static=50, stopped_speed=5e-2)
CLASS_ORDER = (STATIC, VEHICLE, PEDESTRIAN, BICYCLE)   # the slot order: static + dynamic (pdm_observation.py:186)
CAP_FIELD = {VEHICLE: "max_vehicles", PEDESTRIAN: "max_pedestrians", BICYCLE: "max_bicycles", STATIC: "max_static"}
# the margins the golden's seed is chosen for (tests/golden/make_observation_golden.py)
MIN_DISTANCE_GAP, MIN_RADIUS_GAP, MIN_ANGLE_GAP, MIN_SPEED_GAP, MIN_EGO_GAP = 1e-6, 1e-6, 1e-6, 1e-6, 5e-3


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        assert k in p, k
        p[k] = v
    return p


def t_obs(p=None):
    p = p or DEFAULTS
    return p["num_samples"] + p["sample_res"]


def corners(cx, cy, h, half_length, half_width, ft=np.float64):
    """(..., 4, 2): front-left, rear-left, rear-right, front-right (tests/pdm_area_ref.py:60-69's formula)."""
    cx, cy, h = (np.asarray(v, dtype=ft) for v in (cx, cy, h))
    hl, hw = np.asarray(half_length, dtype=ft), np.asarray(half_width, dtype=ft)
    cos, sin = np.cos(h), np.sin(h)
    half_pi = ft(np.pi) / ft(2.0)
    cq, sq = np.cos(h + half_pi), np.sin(h + half_pi)
    out = []
    for lon, lat in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw)):
        out.append(np.stack([cx + ((lat * cq) + (lon * cos)), cy + ((lat * sq) + (lon * sin))], axis=-1))
    return np.stack(out, axis=-2)


def ego_center(ego, ap=None, ft=np.float64):
    ap = ap or A.DEFAULTS
    x, y, h = (ft(v) for v in ego[:3])
    r = ft(ap["rear_axle_to_center"])
    return x + r * np.cos(h), y + r * np.sin(h)


def ego_quad(ego, ap=None, ft=np.float64):
    ap = ap or A.DEFAULTS
    cx, cy = ego_center(ego, ap, ft)
    return corners(cx, cy, ft(ego[2]), ap["half_length"], ap["half_width"], ft)


def normalize_angle(a):
    return np.arctan2(np.sin(a), np.cos(a))


def separation(q, b):
    """The greatest separation of two convex quads over their eight edge normals, on coordinates relative to q's first
    corner: positive = a gap of at least that much, negative = they overlap by that much along the best axis, 0 = they
    touch. Closed intersection is ``separation <= 0``: dd_collisions' separating-axis test."""
    q, b = np.asarray(q), np.asarray(b)
    o = q[0]
    a, c = q - o, b - o
    best = -np.inf
    for poly in (a, c):
        for e in range(4):
            f = (e + 1) % 4
            nx, ny = -(poly[f, 1] - poly[e, 1]), poly[f, 0] - poly[e, 0]
            norm = np.hypot(nx, ny)
            if not norm > 0:
                continue
            pa, pc = (nx * a[:, 0] + ny * a[:, 1]) / norm, (nx * c[:, 0] + ny * c[:, 1]) / norm
            best = max(best, pc.min() - pa.max(), pa.min() - pc.max())
    return best


def quads_touch(q, b):
    """dd_collisions' closed separating-axis test, with its arithmetic (no normalisation of the axes)."""
    q, b = np.asarray(q), np.asarray(b)
    if not (np.isfinite(q).all() and np.isfinite(b).all()):
        return False
    o = q[0]
    a, c = q - o, b - o
    for poly in (a, c):
        for e in range(4):
            f = (e + 1) % 4
            nx, ny = -(poly[f, 1] - poly[e, 1]), poly[f, 0] - poly[e, 0]
            pa, pc = nx * a[:, 0] + ny * a[:, 1], nx * c[:, 0] + ny * c[:, 1]
            if pa.max() < pc.min() or pc.max() < pa.min():
                return False
    return True


def observe(boxes, types, ego, collided_in=None, p=None, ap=None, ft=np.float64):
    """One scene. ``boxes`` (D, 7) center x, y, heading, length, width, vx, vy; ``types`` (D) type ids; ``ego`` the
    rear-axle pose (>= 3 values); ``collided_in`` (D) bool or None. Returns a dict: ``order`` (K = D) the detection
    index of every slot, ``valid`` (K) bool, ``boxes`` (K, T_obs, 4, 2) (0 where not valid), ``heading``, ``speed``
    (K), ``flags`` (K) uint8, ``collided`` (D) bool, ``kept`` (K) bool (kept by the selection: valid or newly
    collided), ``margins``."""
    p, ap = p or DEFAULTS, ap or A.DEFAULTS
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    types = np.asarray(types, dtype=np.int64).reshape(-1)
    n = len(types)
    collided_in = np.zeros(n, dtype=bool) if collided_in is None else np.asarray(collided_in, dtype=bool)
    b = boxes.astype(ft)
    px, py = ego_center(ego, ap, ft)
    quad = ego_quad(ego, ap, ft)
    dx, dy = b[:, 0] - px, b[:, 1] - py
    rank_dist = ((dx * dx) + (dy * dy)) ** ft(0.5)
    far_dist = np.hypot(dx, dy)
    radius = ft(p["map_radius"])
    typed = (types >= 0) & (types <= STATIC)
    far = (far_dist > radius) if p["map_radius"] else np.zeros(n, dtype=bool)
    eligible = typed & ~collided_in & ~far
    margins = dict(distance=np.inf, radius=np.inf, angle=np.inf, speed=np.inf, ego=np.inf)
    if p["map_radius"] and (typed & ~collided_in).any():
        margins["radius"] = float(np.abs(far_dist - radius)[typed & ~collided_in].min())

    agent = typed & (types < STATIC)
    speed = np.where(agent, np.hypot(b[:, 5], b[:, 6]), ft(0.0))
    velocity_angle = np.arctan2(b[:, 6], b[:, 5])
    turn = np.abs(normalize_angle(b[:, 2] - velocity_angle))
    forward = turn < ft(np.pi) / ft(2.0)
    track_heading = np.where(forward, b[:, 2], normalize_angle(b[:, 2] + ft(np.pi)))
    dxy = np.stack([np.cos(track_heading) * speed, np.sin(track_heading) * speed], axis=-1)
    dxy[~agent] = 0.0
    moving = agent & eligible & (speed > 0)
    if moving.any():
        margins["angle"] = float(np.abs(turn - ft(np.pi) / ft(2.0))[moving].min())
    if (agent & eligible).any():
        margins["speed"] = float(np.abs(speed - ft(p["stopped_speed"]))[agent & eligible].min())
    flags = (np.where(~agent | (speed <= ft(p["stopped_speed"])), FLAG_STOPPED, 0)
             | np.where(agent, FLAG_AGENT, 0)).astype(np.uint8)

    order, kept = [], []
    for cls in CLASS_ORDER:
        idx = np.flatnonzero(eligible & (types == cls))
        idx = idx[np.argsort(rank_dist[idx], kind="stable")]   # a tie goes to the lower detection index
        if len(idx) > 1:
            margins["distance"] = min(margins["distance"], float(np.diff(rank_dist[idx]).min()))
        order.extend(idx[:p[CAP_FIELD[cls]]].tolist())
    kept = [True] * len(order)
    taken = set(order)
    rest = [d for d in range(n) if d not in taken]
    order, kept = np.asarray(order + rest, dtype=np.int64), np.asarray(kept + [False] * len(rest), dtype=bool)

    times = t_obs(p)
    base = corners(b[:, 0], b[:, 1], b[:, 2], b[:, 3] / ft(2.0), b[:, 4] / ft(2.0), ft) if n else np.zeros((0, 4, 2), ft)
    out = np.zeros((n, times, 4, 2), dtype=ft)
    valid = np.zeros(n, dtype=bool)
    collided = collided_in.copy()
    for k, d in enumerate(order):
        if not kept[k]:
            continue
        sep = float(separation(quad.astype(np.float64), base[d].astype(np.float64)))
        margins["ego"] = min(margins["ego"], abs(sep))
        if quads_touch(quad, base[d]):
            collided[d] = True   # it counted toward its cap and is valid at no time
            continue
        valid[k] = True
        for t in range(times):
            delta = ft(float(p["sample_res"] * (t // p["sample_res"]))) * ft(p["dt"])
            out[k, t] = base[d] + delta * dxy[d]
    return dict(order=order, valid=valid, kept=kept, boxes=out, heading=b[order, 2], speed=speed[order],
                flags=flags[order], collided=collided, margins=margins)


def observe_scenes(scenes, p=None, ap=None, ft=np.float64, collided_in=None):
    """Several scenes (dicts of ``boxes``, ``types``, ``ego``) as dd_observe packs them: the slots of scene g follow
    those of scene g - 1, ``order`` holds flat detection indices. ``collided_in``: flat (D) or None."""
    outs, off = [], [0]
    for g, sc in enumerate(scenes):
        n = len(sc["types"])
        ci = None if collided_in is None else np.asarray(collided_in)[off[-1]:off[-1] + n]
        outs.append(observe(sc["boxes"], sc["types"], sc["ego"], ci, p, ap, ft))
        off.append(off[-1] + n)
    times = t_obs(p)
    cat = lambda key, empty: np.concatenate([o[key] for o in outs]) if outs else empty   # noqa: E731
    margins = {k: min([o["margins"][k] for o in outs] + [np.inf]) for k in ("distance", "radius", "angle", "speed", "ego")}
    return dict(order=np.concatenate([o["order"] + off[g] for g, o in enumerate(outs)]).astype(np.int64),
                valid=cat("valid", None), kept=cat("kept", None), boxes=cat("boxes", np.zeros((0, times, 4, 2))),
                heading=cat("heading", None), speed=cat("speed", None), flags=cat("flags", None),
                collided=cat("collided", None), off=np.asarray(off, dtype=np.int32), margins=margins)


def detections_from_agents(agent_states, agent_labels, ego_states, threshold=0.0, ft=np.float64):
    """dd_detections_from_agents: (B, A, 5) float32 ego-frame boxes and (B, A) logits -> boxes (B A, 7), types (B A)."""
    s = np.asarray(agent_states, dtype=np.float32).astype(ft)
    logit = np.asarray(agent_labels, dtype=np.float32).astype(ft)
    ego = np.asarray(ego_states, dtype=np.float64).astype(ft)
    x0, y0, h0 = ego[:, None, 0], ego[:, None, 1], ego[:, None, 2]
    c0, s0 = np.cos(h0), np.sin(h0)
    with np.errstate(invalid="ignore"):
        cx = x0 + ((c0 * s[..., 0]) - (s0 * s[..., 1]))
        cy = y0 + ((s0 * s[..., 0]) + (c0 * s[..., 1]))
        heading = h0 + s[..., 2]
        ok = (np.isfinite(s).all(-1) & np.isfinite(logit) & np.isfinite(cx) & np.isfinite(cy) & np.isfinite(heading)
              & (logit > ft(np.float32(threshold))) & (s[..., 3] > 0) & (s[..., 4] > 0))
    zero = np.zeros_like(cx)
    boxes = np.stack([cx, cy, heading, s[..., 3], s[..., 4], zero, zero], axis=-1)
    boxes = np.where(ok[..., None], boxes, ft(0.0)).reshape(-1, 7)
    return boxes, np.where(ok, VEHICLE, SKIP).reshape(-1).astype(np.uint8)


# ---- the derived bars (tests/test_observation_gpu.py's docstring has the derivation)

def box_floor(ref64, reach):
    """Per coordinate: 2 spacings of the coordinate plus 16 ulp of ``reach`` = half diagonal + speed * T_obs * dt."""
    return 2.0 * np.spacing(np.abs(ref64)) + 16.0 * np.spacing(np.asarray(reach, dtype=np.float64))


def box_bar(ref64, refld, reach):
    return np.maximum(box_floor(ref64, reach), 16.0 * np.abs(ref64 - refld.astype(np.float64)))


def reach_of(boxes7, order, p=None):
    """(K, 1, 1, 1): half diagonal + speed * T_obs * dt of the detection each slot holds."""
    p = p or DEFAULTS
    b = np.asarray(boxes7, dtype=np.float64).reshape(-1, 7)[np.asarray(order, dtype=np.int64)]
    reach = 0.5 * np.hypot(b[:, 3], b[:, 4]) + np.hypot(b[:, 5], b[:, 6]) * (t_obs(p) * p["dt"])
    return reach[:, None, None, None]


# ---- the seeded scenes the golden and the tests share

def _row(token, x, y, h, length, width, vx, vy, type_name):
    return (token, float(x), float(y), float(h), float(length), float(width), float(vx), float(vy), type_name)


def scene_arrays(scene):
    """A scene dict with ``dets`` rows -> adds ``boxes`` (D, 7), ``types`` (D), ``tokens``."""
    dets = scene["dets"]
    scene["boxes"] = np.array([r[1:8] for r in dets], dtype=np.float64).reshape(-1, 7)
    scene["types"] = np.array([TYPE_IDS[r[8]] for r in dets], dtype=np.uint8)
    scene["tokens"] = [r[0] for r in dets]
    return scene


SIZES = dict(VEHICLE=(4.6, 1.9), PEDESTRIAN=(0.7, 0.7), BICYCLE=(1.8, 0.6), TRAFFIC_CONE=(0.4, 0.4),
             BARRIER=(2.5, 0.6), CZONE_SIGN=(0.6, 0.6), GENERIC_OBJECT=(1.2, 1.0))
STATIC_NAMES = ("TRAFFIC_CONE", "BARRIER", "CZONE_SIGN", "GENERIC_OBJECT")


def seeded_scene(rng, name, pose, counts, ap=None, reversing=False, overlapping=False, ego_row=True, far=3):
    """Objects scattered 7 .. 95 m around the ego center (further than any two boxes can touch the ego quad), ``far``
    more per class beyond the 100 m radius, optionally a vehicle driving backwards and one that overlaps the ego."""
    ap = ap or A.DEFAULTS
    ego = np.zeros(11)
    ego[:3] = pose
    ego[3] = 4.0
    cx, cy = ego_center(ego, ap)
    dets = []

    def place(kind, tag, lo, hi, count):
        for i in range(count):
            r, phi = rng.uniform(lo, hi), rng.uniform(-np.pi, np.pi)
            length, width = (s * rng.uniform(0.9, 1.1) for s in SIZES[kind])
            h = rng.uniform(-np.pi, np.pi)
            if kind in STATIC_NAMES:
                vx = vy = 0.0
            else:
                v = rng.choice([0.0, 0.02, rng.uniform(0.2, 9.0)], p=[0.1, 0.1, 0.8])
                course = h + rng.normal(0.0, 0.2)   # mostly along the heading
                vx, vy = v * np.cos(course), v * np.sin(course)
            dets.append(_row(f"{name}_{tag}_{i}", cx + r * np.cos(phi), cy + r * np.sin(phi), h, length, width, vx, vy,
                             kind))

    for kind, count in counts.items():
        place(kind, kind.lower(), 7.0, 95.0, count)
        place(kind, kind.lower() + "_far", 101.0, 130.0, far)
    if reversing:
        h = rng.uniform(-np.pi, np.pi)
        dets.append(_row(f"{name}_reversing", cx + 20.0 * np.cos(h + 1.0), cy + 20.0 * np.sin(h + 1.0), h, 4.6, 1.9,
                         -2.5 * np.cos(h + 0.1), -2.5 * np.sin(h + 0.1), "VEHICLE"))
    if overlapping:
        dets.append(_row(f"{name}_overlapping", cx + 1.5 * np.cos(pose[2] + 0.7), cy + 1.5 * np.sin(pose[2] + 0.7),
                         pose[2] + 0.4, 4.6, 1.9, 1.0 * np.cos(pose[2] + 0.4), 1.0 * np.sin(pose[2] + 0.4), "VEHICLE"))
    if ego_row:
        dets.append(_row(f"{name}_ego", cx, cy, pose[2], 2.0 * ap["half_length"], 2.0 * ap["half_width"], 4.0, 0.0, "EGO"))
    rng.shuffle(dets)   # a scene is no sorted list: the detection order is not the distance order
    return scene_arrays(dict(name=name, ego=ego, dets=[tuple(d) for d in dets]))


def golden_scenes(seed):
    """The three scenes of tests/golden/pdm_observation_s<seed>.npz: at the origin, at 6.6e5 / 4.0e6 m, and a crowded
    one that passes all four caps, with a reversing agent and a track that overlaps the ego."""
    rng = np.random.default_rng(seed)
    few = dict(VEHICLE=9, PEDESTRIAN=5, BICYCLE=3, TRAFFIC_CONE=3, BARRIER=2)
    many = dict(VEHICLE=55, PEDESTRIAN=29, BICYCLE=13, TRAFFIC_CONE=20, BARRIER=14, CZONE_SIGN=10, GENERIC_OBJECT=10)
    return [seeded_scene(rng, "origin", (0.0, 0.0, 0.3), few),
            seeded_scene(rng, "far", (6.6e5 + 12.25, 4.0e6 - 7.5, -2.1), few, reversing=True),
            seeded_scene(rng, "crowded", (312.5, -48.25, 2.6), many, reversing=True, overlapping=True, far=2)]


def margins_hold(m):
    return (m["distance"] >= MIN_DISTANCE_GAP and m["radius"] >= MIN_RADIUS_GAP and m["angle"] >= MIN_ANGLE_GAP
            and m["speed"] >= MIN_SPEED_GAP and m["ego"] >= MIN_EGO_GAP)


# ---- hand cases whose answers are known by construction

def hand_cases():
    """[(name, scene, params, collided_in, expected)]: ``expected`` holds ``valid`` (the set of detection indices that
    are valid tracks), ``collided`` (the set of detection indices in collided_out), ``t_obs``, and optionally
    ``shift``: {detection: (dx, dy) per second} of the forecast."""
    ego = np.zeros(11)
    ego[3] = 5.0
    cases = []

    def scene(name, dets):
        return scene_arrays(dict(name=name, ego=ego.copy(), dets=dets))

    def ring(kind, count, r0, step=1.0, tag=None):
        # `count` objects on the x axis ahead of the ego center at r0, r0 + step, ...: the distance order is the index order
        cx = A.DEFAULTS["rear_axle_to_center"]
        length, width = SIZES[kind]
        return [_row(f"{tag or kind.lower()}_{i}", cx + r0 + step * i, 30.0 if i % 2 else -30.0, 0.5, length * 0.2,
                     width * 0.2, 0.0, 0.0, kind) for i in range(count)]

    # a vehicle heading along +x whose velocity points along -x: forecast backwards along its own axis
    cases.append(("reversing", scene("reversing", [_row("rev", 20.0, 5.0, 0.0, 4.6, 1.9, -3.0, 0.0, "VEHICLE"),
                                                   _row("fwd", 23.0, -5.0, 0.0, 4.6, 1.9, 3.0, 0.0, "VEHICLE")]),
                  None, None, dict(valid={0, 1}, collided=set(), t_obs=52, shift={0: (-3.0, 0.0), 1: (3.0, 0.0)})))
    # 51 vehicles and 26 pedestrians: the farthest of each is dropped, independently
    dets = ring("VEHICLE", 51, 10.0) + ring("PEDESTRIAN", 26, 10.5)
    cases.append(("caps", scene("caps", dets), None, None,
                  dict(valid=set(range(77)) - {50, 76}, collided=set(), t_obs=52)))
    # the nearest of 51 vehicles overlaps the ego: it counted toward the cap (the 51st stays dropped) and is invalid
    over = [_row("over", 1.0, 0.0, 0.0, 4.6, 1.9, 0.0, 0.0, "VEHICLE")]
    dets = over + ring("VEHICLE", 50, 10.0)
    cases.append(("overlap_counts", scene("overlap_counts", dets), None, None,
                  dict(valid=set(range(1, 50)), collided={0}, t_obs=52)))
    # the same with the overlapping track already collided: it frees its slot and the 51st is kept
    collided = np.zeros(51, dtype=bool)
    collided[0] = True
    cases.append(("collided_frees", scene("collided_frees", dets), None, collided,
                  dict(valid=set(range(1, 51)), collided={0}, t_obs=52)))
    # an EGO-typed row is dropped, wherever it is
    cases.append(("ego_row", scene("ego_row", [_row("me", 30.0, 0.0, 0.0, 5.0, 2.0, 0.0, 0.0, "EGO"),
                                               _row("cone", 12.0, 3.0, 0.0, 0.4, 0.4, 0.0, 0.0, "TRAFFIC_CONE")]),
                  None, None, dict(valid={1}, collided=set(), t_obs=52)))
    # radius 0 keeps what the default radius drops
    dets = [_row("near", 40.0, 0.0, 0.0, 4.6, 1.9, 1.0, 0.0, "VEHICLE"),
            _row("beyond", 500.0, 0.0, 0.0, 4.6, 1.9, 1.0, 0.0, "VEHICLE")]
    cases.append(("radius_default", scene("radius_default", dets), None, None,
                  dict(valid={0}, collided=set(), t_obs=52)))
    cases.append(("radius_zero", scene("radius_zero", dets), params(map_radius=0.0), None,
                  dict(valid={0, 1}, collided=set(), t_obs=52)))
    # sample_res 3 with 60 samples: T_obs 63, the maps at 3 (t // 3)
    cases.append(("res3", scene("res3", [_row("v", 20.0, 5.0, 0.0, 4.6, 1.9, 2.0, 0.0, "VEHICLE")]),
                  params(num_samples=60, sample_res=3), None,
                  dict(valid={0}, collided=set(), t_obs=63, shift={0: (2.0, 0.0)})))
    return cases


def check_hand_case(name, out, expected, scene, p=None):
    """``out``: observe()'s dict, or the same fields taken from the device."""
    p = p or DEFAULTS
    order = np.asarray(out["order"], dtype=np.int64)
    valid = np.asarray(out["valid"]).astype(bool)
    if valid.ndim == 2:
        assert (valid == valid[:, :1]).all(), name
        valid = valid[:, 0]
    assert sorted(order.tolist()) == list(range(len(scene["types"]))), (name, "order is no permutation")
    assert set(order[valid].tolist()) == expected["valid"], (name, sorted(order[valid].tolist()))
    assert set(np.flatnonzero(np.asarray(out["collided"])).tolist()) == expected["collided"], name
    boxes = np.asarray(out["boxes"], dtype=np.float64)
    assert boxes.shape[1] == expected["t_obs"] == t_obs(p), (name, boxes.shape)
    for d, (vx, vy) in expected.get("shift", {}).items():
        k = int(np.flatnonzero(order == d)[0])
        for t in range(boxes.shape[1]):
            delta = p["sample_res"] * (t // p["sample_res"]) * p["dt"]
            move = boxes[k, t] - boxes[k, 0]
            assert np.abs(move - np.array([vx, vy]) * delta).max() < 1e-9, (name, d, t, move)
