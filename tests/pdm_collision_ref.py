"""numpy restatement of the rest of the PDM score: no-at-fault collision, time-to-collision, progress and the
aggregation (dd_collisions, dd_progress, dd_pdm_aggregate, include/ddmi.h).

Restates, with every quirk kept:
  PDMScorer._calculate_no_at_fault_collision   pdm_planner/scoring/pdm_scorer.py:293-349
  get_collision_type                           scoring/pdm_scorer_utils.py:13-65
  PDMScorer._calculate_ttc                     pdm_scorer.py:414-498 (the shift is dxy * (float(k) * dt); the k = 0
                                               quad is corner + dxy * 0.0)
  PDMScorer._calculate_progress                :398-412
  PDMScorer._aggregate_scores                  :156-183, and the pair rule of navsim/evaluate/pdm_score.py:99-130
Per (candidate, track) only the first hit decides (the reference's per-candidate token list, restated as a first-hit
search), so the pairs are scored independently.

The primitives stand in for shapely, which cannot be run here: closed quad - quad and segment - quad intersection
(separating axes over differences), the quad's area centroid, strict point-in-polygon (pdm_area_ref.contains) and the
polyline projection (LineString.project as GEOS is remembered to do it). tests/golden/make_collision_golden.py runs the
reference's own scorer over these primitives and checks each of them, on every use, against an independent predicate
below that shares no code with it: vertex containment by half-plane signs plus proper edge crossings by orientation;
the corner mean; a dense-sampling bound for the projection.

nuPlan is not part of the reference tree either: is_agent_ahead / is_agent_behind / is_track_stopped and AGENT_TYPES
are quoted from memory (ddmi.h).

Also the seeded inputs the golden and the tests share: tracks laid around a set's paths, the centerline, the
hand-built quirk cases.
"""
import numpy as np

import pdm_area_ref as A
import pdm_comfort_ref as C

T = A.T
T_OBS = 51                     # metric_cache_processor.py:200-206: 51 occupancy maps
STEPS = (0, 3, 6, 9)           # np.arange(0, 10, 3)
VX, VY = 3, 4
STOPPED_EGO, STOPPED_TRACK, ACTIVE_FRONT, ACTIVE_REAR, ACTIVE_LATERAL = range(5)   # nuPlan's CollisionType
TYPE_NAMES = ("STOPPED_EGO_COLLISION", "STOPPED_TRACK_COLLISION", "ACTIVE_FRONT_COLLISION", "ACTIVE_REAR_COLLISION",
              "ACTIVE_LATERAL_COLLISION")
AGENT_TYPE_NAMES = ("VEHICLE", "PEDESTRIAN", "BICYCLE")
TRACK_STOPPED_SPEED = 5e-2
RED_LIGHT = "red_light"

SCORE_DEFAULTS = dict(progress_weight=5.0, ttc_weight=5.0, comfortable_weight=2.0, driving_direction_weight=0.0,
                      progress_distance_threshold=5.0, ttc_stopped_speed_threshold=5e-3,
                      collision_stopped_speed_threshold=5e-2, ahead_angle=float(np.deg2rad(30.0)),
                      behind_angle=float(np.deg2rad(150.0)))
# the non-default set of the golden: other weights (the driving-direction term counts), thresholds and angle bounds
SCORE_ALT = dict(progress_weight=4.0, ttc_weight=3.0, comfortable_weight=2.0, driving_direction_weight=1.0,
                 progress_distance_threshold=12.0, ttc_stopped_speed_threshold=0.5,
                 collision_stopped_speed_threshold=1.0, ahead_angle=float(np.deg2rad(45.0)),
                 behind_angle=float(np.deg2rad(120.0)))


def score_params(**over):
    p = dict(SCORE_DEFAULTS)
    for k, v in over.items():
        assert k in p, k
        p[k] = v
    return p


# ---- the stand-in primitives

def _separation(pa, pb):
    """The largest signed separation of point sets pa (..., na, 2) and pb (..., 4, 2) over the edge normals of both,
    in metres (negative: the least penetration), everything relative to pa's first point; and whether any axis
    separates them by the unnormalised comparison the device makes."""
    o = pa[..., :1, :]
    ra, rb = pa - o, pb - o
    best = np.full(np.broadcast_shapes(ra.shape[:-2], rb.shape[:-2]), -np.inf)
    sep = np.zeros(best.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for poly in (ra, rb):
            n = poly.shape[-2]
            for e in range(n if n > 2 else 1):
                d = poly[..., (e + 1) % n, :] - poly[..., e, :]
                nx, ny = -d[..., 1], d[..., 0]
                a = nx[..., None] * ra[..., 0] + ny[..., None] * ra[..., 1]
                b = nx[..., None] * rb[..., 0] + ny[..., None] * rb[..., 1]
                sep |= (a.max(-1) < b.min(-1)) | (b.max(-1) < a.min(-1))
                length = np.hypot(nx, ny)
                gap = np.maximum(b.min(-1) - a.max(-1), a.min(-1) - b.max(-1)) / length
                best = np.where(length > 0, np.maximum(best, gap), best)
    return best, sep


def _finite(pa, pb):
    return np.isfinite(pa).all((-1, -2)) & np.isfinite(pb).all((-1, -2))


def quads_touch(a, b):
    """Closed intersection of convex quads a and b (..., 4, 2): touching counts; a non-finite corner intersects
    nothing."""
    return _finite(a, b) & ~_separation(a, b)[1]


def segment_touches(seg, b):
    """Closed intersection of the segment seg (..., 2, 2) with the convex quad b."""
    return _finite(seg, b) & ~_separation(seg, b)[1]


def gap(a, b):
    """Signed distance-like margin of the test above (positive: apart, negative: overlapping), inf where non-finite."""
    g = _separation(a, b)[0]
    return np.where(_finite(a, b), g, np.inf)


def centroid_rel(b):
    """The area centroid of quad b (..., 4, 2) relative to its first corner (the corner mean for a zero-area quad)."""
    u, v, w = b[..., 1, :] - b[..., 0, :], b[..., 2, :] - b[..., 0, :], b[..., 3, :] - b[..., 0, :]
    a1 = u[..., 0] * v[..., 1] - v[..., 0] * u[..., 1]
    a2 = v[..., 0] * w[..., 1] - w[..., 0] * v[..., 1]
    a = a1 + a2
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (a1[..., None] * (u + v) + a2[..., None] * (v + w)) / (3.0 * a)[..., None]
    return np.where((a == 0.0)[..., None], ((u + v) + w) / 4.0, c)


def centroid(b):
    return b[..., 0, :] + centroid_rel(b)


def relative_angle(x, y, h, b):
    """nuPlan's get_agent_relative_angle from the rear-axle pose to the centroid of quad b."""
    c = centroid_rel(b)
    v = np.stack([(b[..., 0, 0] - x) + c[..., 0], (b[..., 0, 1] - y) + c[..., 1]], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = v / np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])[..., None]
        return np.arccos(np.cos(h) * u[..., 0] + np.sin(h) * u[..., 1])


def project(line, x, y):
    """LineString(line).project(Point(x, y)) for arrays x, y: the nearest segment (the first on a tie), the parameter
    clamped to [0, 1], the summed lengths before it plus the partial length; differences against the segment start."""
    line = np.asarray(line, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    best = np.full(x.shape, np.inf)
    at = np.full(x.shape, np.nan)
    passed = 0.0
    with np.errstate(invalid="ignore"):
        for a, b in zip(line[:-1], line[1:]):
            dx, dy = b[0] - a[0], b[1] - a[1]
            len2 = dx * dx + dy * dy
            length = np.sqrt(len2)
            wx, wy = x - a[0], y - a[1]
            s = (wx * dx + wy * dy) / len2 if len2 > 0.0 else np.zeros(x.shape)
            s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
            ex, ey = wx - s * dx, wy - s * dy
            d2 = ex * ex + ey * ey
            nearer = d2 < best
            best = np.where(nearer, d2, best)
            at = np.where(nearer, passed + s * length, at)
            passed = passed + length
    return at


# ---- the independent predicates (no code shared with the primitives above)

def _in_closed_convex(ring, p):
    v = np.asarray(ring)
    w = np.roll(v, -1, axis=0)
    side = np.array([(c - a) * (p[1] - b) - (d - b) * (p[0] - a) for (a, b), (c, d) in zip(v, w)])
    return bool((side >= 0).all() or (side <= 0).all())


def _orient(p, q, r):
    return np.sign((q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]))


def _segments_cross(p1, p2, p3, p4):
    return _orient(p1, p2, p3) * _orient(p1, p2, p4) < 0 and _orient(p3, p4, p1) * _orient(p3, p4, p2) < 0


def independent_touch(a, b):
    """One pair: a (na, 2) - a quad or a segment - against the quad b, by vertex containment and proper crossings.
    Coordinates relative to b's first corner (an exact shift, no shared rounding with the separating axes)."""
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return False
    o = b[0]
    a, b = a - o, b - o
    if any(_in_closed_convex(b, p) for p in a):
        return True
    if len(a) > 2 and any(_in_closed_convex(a, p) for p in b):
        return True
    ea = [(a[i], a[(i + 1) % len(a)]) for i in range(len(a) if len(a) > 2 else 1)]
    eb = [(b[i], b[(i + 1) % 4]) for i in range(4)]
    return any(_segments_cross(p1, p2, p3, p4) for p1, p2 in ea for p3, p4 in eb)


def independent_project(line, x, y, per_metre=2000):
    """Arc length of the nearest of dense samples of the polyline, and the bound of its error: the sample spacing
    plus what a near-tie between two samples can hide. x, y: one point (a float comes back) or arrays of points."""
    line = np.asarray(line, dtype=np.float64)
    seg = np.linalg.norm(np.diff(line, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    pts, arc = [], []
    for i, length in enumerate(seg):
        m = max(2, int(np.ceil(length * per_metre)) + 1)
        f = np.linspace(0.0, 1.0, m)
        pts.append(line[i] + f[:, None] * (line[i + 1] - line[i]))
        arc.append(cum[i] + f * length)
    pts, arc = np.concatenate(pts), np.concatenate(arc)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.empty(x.size)
    for at in range(0, x.size, 16):       # the samples against 16 points at a time
        qx, qy = x.reshape(-1)[at:at + 16], y.reshape(-1)[at:at + 16]
        out[at:at + 16] = arc[np.argmin((pts[:, :1] - qx) ** 2 + (pts[:, 1:] - qy) ** 2, axis=0)]
    return (float(out[0]) if x.ndim == 0 else out.reshape(x.shape)), 1.0 / per_metre


# ---- the restatement

def ego_quads(states, ap=None):
    """(N, T, 4, 2) ego quads, (N, T) speeds and the (N, T, 4, 4, 2) shifted TTC quads."""
    ap = ap or A.DEFAULTS
    corners = A.coords(states, ap)[..., :4, :]
    with np.errstate(invalid="ignore", over="ignore"):
        speeds = np.hypot(states[..., VX], states[..., VY])
        dxy = np.stack([np.cos(states[..., A.HEADING]) * speeds, np.sin(states[..., A.HEADING]) * speeds], axis=-1)
        shifted = np.stack([corners + dxy[..., None, :] * (float(k) * ap["dt"]) for k in STEPS], axis=2)
    return corners, speeds, shifted


def drop_tokens(tracks, collided=()):
    """The tracks both metrics can ever count: not a red light, not collided before the horizon."""
    return [tr for tr in tracks if RED_LIGHT not in tr["token"] and tr["token"] not in collided]


def collisions(states, areas, tracks, inter_rings, ap=None, sp=None, collided=()):
    """One scene. tracks: dicts(token, boxes (T_obs, 4, 2), valid (T_obs), heading, is_agent, stopped); inter_rings:
    the rings lists of the INTERSECTION polygons. Returns dict(no_collision, collision_time_idx, ttc, ttc_time_idx,
    types (N, K): the deciding first hit's collision type or -1, ttc_hits (N, K): 1 infraction, 0 shielding hit, -1
    none, margin: the smallest |gap| of every tested pair, speed / angle margins)."""
    ap, sp = ap or A.DEFAULTS, sp or SCORE_DEFAULTS
    tracks = drop_tokens(tracks, collided)
    n = states.shape[0]
    corners, speeds, shifted = ego_quads(states, ap)
    off_lane = areas[..., A.MULTIPLE_LANES] | areas[..., A.NON_DRIVABLE]
    x, y, h = states[..., A.X], states[..., A.Y], states[..., A.HEADING]
    out = dict(no_collision=np.ones(n), collision_time_idx=np.full(n, np.inf), ttc=np.ones(n),
               ttc_time_idx=np.full(n, np.inf), types=np.full((n, len(tracks)), -1),
               ttc_hits=np.full((n, len(tracks)), -1))
    gap_margin, angle_margin, axle_points = np.inf, np.inf, []
    with np.errstate(invalid="ignore"):
        live = ~(speeds < sp["ttc_stopped_speed_threshold"])
    tidx = np.arange(T)
    for j, tr in enumerate(tracks):
        boxes, valid = tr["boxes"], np.asarray(tr["valid"], dtype=bool)
        hit = valid[None, :T] & quads_touch(corners, boxes[None, :T])
        gap_margin = min(gap_margin, float(np.abs(gap(corners, boxes[None, :T])[:, valid[:T]]).min(initial=np.inf)))
        for i in np.flatnonzero(hit.any(1)):
            t = int(np.argmax(hit[i]))
            b = boxes[t]
            if speeds[i, t] <= sp["collision_stopped_speed_threshold"]:
                kind = STOPPED_EGO
            elif tr["stopped"]:
                kind = STOPPED_TRACK
            else:
                angle = float(relative_angle(x[i, t], y[i, t], h[i, t], b))
                angle_margin = min(angle_margin, abs(angle - sp["behind_angle"]))
                if angle > sp["behind_angle"]:
                    kind = ACTIVE_REAR
                else:
                    bumper = corners[i, t][[A.FRONT_LEFT, A.FRONT_RIGHT]]
                    gap_margin = min(gap_margin, abs(float(gap(bumper, b))))
                    kind = ACTIVE_FRONT if segment_touches(bumper, b) else ACTIVE_LATERAL
            out["types"][i, j] = kind
            if kind in (ACTIVE_FRONT, STOPPED_TRACK) or (kind == ACTIVE_LATERAL and off_lane[i, t]):
                out["no_collision"][i] = min(out["no_collision"][i], 0.0 if tr["is_agent"] else 0.5)
                out["collision_time_idx"][i] = min(out["collision_time_idx"][i], t)
        # TTC: (N, T, 4) hits of the shifted quads against map t + k
        at = tidx[:, None] + np.asarray(STEPS)[None, :]
        future = boxes[at]                                     # (T, 4, 4, 2)
        there = valid[at]
        hits = there[None] & quads_touch(shifted, future[None])
        gap_margin = min(gap_margin, float(np.abs(gap(shifted, future[None])[:, there]).min(initial=np.inf)))
        hits &= live[..., None]
        flat = hits.reshape(n, -1)
        for i in np.flatnonzero(flat.any(1)):
            t, q = divmod(int(np.argmax(flat[i])), len(STEPS))
            angle = float(relative_angle(x[i, t], y[i, t], h[i, t], future[t, q]))
            angle_margin = min(angle_margin, abs(angle - sp["ahead_angle"]), abs(angle - sp["behind_angle"]))
            infraction = angle < sp["ahead_angle"]
            if not infraction and not angle > sp["behind_angle"]:
                axle_points.append((x[i, t], y[i, t]))
                infraction = bool(off_lane[i, t]) or any(
                    bool(A.contains(rings, x[i, t], y[i, t])) for rings in inter_rings)
            out["ttc_hits"][i, j] = int(infraction)
            if infraction:
                out["ttc"][i] = 0.0
                out["ttc_time_idx"][i] = min(out["ttc_time_idx"][i], t)
    f = speeds[np.isfinite(speeds)]
    out["gap_margin"], out["angle_margin"] = gap_margin, angle_margin
    out["speed_margin"] = float(min(np.abs(f - sp["ttc_stopped_speed_threshold"]).min(initial=np.inf),
                                    np.abs(f - sp["collision_stopped_speed_threshold"]).min(initial=np.inf)))
    out["axle_points"] = np.array(axle_points).reshape(-1, 2)
    return out


def raw_progress(states, line, ap=None):
    ap = ap or A.DEFAULTS
    c = A.coords(states, ap)[:, :, A.CENTER]
    with np.errstate(invalid="ignore"):
        d = project(line, c[:, -1, 0], c[:, -1, 1]) - project(line, c[:, 0, 0], c[:, 0, 1])
        return np.where(d < 0.0, 0.0, d)


def aggregate(no_collision, drivable_area, driving_direction, raw, ttc, comfortable, sp=None, reference=None):
    """_aggregate_scores over one group (``reference`` None), or per candidate as the pair [reference, candidate]
    (``reference`` = the PDM-closed trajectory's raw * multi). Returns (score, progress term, pmax)."""
    sp = sp or SCORE_DEFAULTS
    multi = no_collision * drivable_area
    p = raw * multi
    with np.errstate(invalid="ignore", divide="ignore"):
        pmax = np.full(p.shape, np.max(p)) if reference is None else np.max(np.stack([np.full(p.shape, reference), p]), 0)
        term = np.where(pmax > sp["progress_distance_threshold"], p / pmax, np.where(multi == 0.0, 0.0, 1.0))
        w = np.array([sp["progress_weight"], sp["ttc_weight"], sp["comfortable_weight"], sp["driving_direction_weight"]])
        weighted = (np.stack([term, ttc, comfortable.astype(np.float64), driving_direction]) * w[:, None]).sum(axis=0)
        weighted /= w.sum()
        return multi * weighted, term, pmax


def pdm_score(states, items, tracks, line, ap=None, sp=None, cp=None, reference=None, collided=()):
    """One scene, every stage: dict of the seven sub-scores, the time indices, raw progress, score and the margins."""
    ap, sp = ap or A.DEFAULTS, sp or SCORE_DEFAULTS
    ego = A.ego_areas(states, items, ap)
    inter = [it[0] for it in items if it[1] == "INTERSECTION"]
    col = collisions(states, ego["areas"], tracks, inter, ap, sp, collided)
    comfort = C.comfort(states, cp or C.params(dt=ap["dt"]))[0]
    raw = raw_progress(states, line, ap)
    score, term, pmax = aggregate(col["no_collision"], ego["drivable_area"], ego["driving_direction"], raw, col["ttc"],
                                  comfort.all(-1), sp, reference)
    return dict(col, areas=ego["areas"], drivable_area=ego["drivable_area"], driving_direction=ego["driving_direction"],
                comfort=comfort, raw_progress=raw, progress=term, score=score, pmax=pmax)


def pdm_score_grouped(states, maps, tracks, lines, **kw):
    """(G, n, T, 11) states, scene g on maps[g], tracks[g], lines[g]; the results stacked over the scenes."""
    parts = [pdm_score(states[g], maps[g], tracks[g], lines[g], **kw) for g in range(len(maps))]
    keys = ("no_collision", "collision_time_idx", "ttc", "ttc_time_idx", "drivable_area", "driving_direction",
            "comfort", "raw_progress", "progress", "score", "areas")
    out = {k: np.stack([q[k] for q in parts]) for k in keys}
    for k in ("gap_margin", "angle_margin", "speed_margin"):
        out[k] = min(q[k] for q in parts)
    return out


# ---- the bars of the GPU tests

def raw_progress_bar(states, line, ap=None):
    """Per projection: the center (two roundings at the coordinate's magnitude and a few ulp of sin / cos on the lever
    arm), the two segment ends (one rounding each in the differences), the parameter's products (relative 8 ulp of
    the segment length) and one rounding per summed segment at the path length; twice, for the two projections."""
    ap = ap or A.DEFAULTS
    line = np.asarray(line)
    big = max(float(np.nanmax(np.abs(line))), float(np.nanmax(np.abs(np.nan_to_num(states[..., :2])))))
    length = float(np.linalg.norm(np.diff(line, axis=0), axis=1).sum())
    one = (4.0 * np.spacing(big) + 16.0 * 2.0 ** -52 * ap["rear_axle_to_center"] + 8.0 * 2.0 ** -52 * length
           + len(line) * np.spacing(length))
    return 2.0 * one


def score_bars(ref, raw_bar, sp=None):
    """The raw bound through p / pmax (numerator and denominator each off by raw_bar, relative to pmax) and through
    the weights, plus four units in the last place of a value at 1."""
    sp = sp or SCORE_DEFAULTS
    with np.errstate(invalid="ignore", divide="ignore"):
        term_bar = np.where(ref["pmax"] > sp["progress_distance_threshold"], 2.0 * raw_bar / ref["pmax"], 0.0) + 4 * 2.0 ** -52
    wsum = sp["progress_weight"] + sp["ttc_weight"] + sp["comfortable_weight"] + sp["driving_direction_weight"]
    return term_bar, term_bar * sp["progress_weight"] / wsum + 4 * 2.0 ** -52


# ---- seeded inputs

def box(cx, cy, h, length, width):
    """(..., 4, 2): front-left, rear-left, rear-right, front-right of an oriented box."""
    cx, cy, h = np.broadcast_arrays(np.asarray(cx, dtype=np.float64), cy, h)
    c, s = np.cos(h), np.sin(h)
    out = []
    for lon, lat in ((0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5), (0.5, -0.5)):
        out.append(np.stack([cx + lon * length * c - lat * width * s, cy + lon * length * s + lat * width * c], -1))
    return np.stack(out, axis=-2)


def track(token, cx, cy, h, length, width, kind, speed, valid=None, t_obs=T_OBS):
    """A track dict from per-time centers. ``kind``: a tracked-object type name; an object that is not a
    VEHICLE / PEDESTRIAN / BICYCLE is no Agent: it has no velocity and counts as stopped."""
    cx, cy = np.broadcast_to(cx, (t_obs,)).astype(np.float64), np.broadcast_to(cy, (t_obs,)).astype(np.float64)
    is_agent = kind in AGENT_TYPE_NAMES
    return dict(token=token, boxes=box(cx, cy, np.broadcast_to(h, (t_obs,)), length, width),
                valid=np.ones(t_obs, dtype=bool) if valid is None else np.asarray(valid, dtype=bool),
                heading=float(np.broadcast_to(h, (t_obs,))[int(np.argmax(valid)) if valid is not None else 0]),
                is_agent=is_agent, stopped=(not is_agent) or speed <= TRACK_STOPPED_SPEED, kind=kind,
                speed=float(speed) if is_agent else None)


def seeded_tracks(seed, states, dt=0.1, t_obs=T_OBS):
    """Tracks laid around the paths of ``states`` (N, T, 11): for each kind an anchor candidate and time are drawn
    and the track is placed against that candidate's pose there. Returns (tracks, collided): a slower vehicle met
    from behind, a faster one that runs into the rear, a stopped vehicle beside a path, a pedestrian crossing one, a
    static non-agent object, a vehicle alongside that is absent for part of the horizon, a red-light token across
    the start and a previously collided token on it."""
    rng = np.random.default_rng(seed)
    n = states.shape[0]
    times = np.arange(t_obs)
    tracks = []

    def anchor(lo, hi):
        i, t = int(rng.integers(n)), int(rng.integers(lo, hi))
        x, y, h = states[i, t, :3]
        v = float(np.hypot(states[i, t, VX], states[i, t, VY]))
        return t, x, y, h, v

    def moving(token, kind, t0, x0, y0, course, speed, length, width, valid=None, heading=None):
        d = (times - t0) * dt * speed
        return track(token, x0 + d * np.cos(course), y0 + d * np.sin(course), course if heading is None else heading,
                     length, width, kind, speed, valid, t_obs)

    fwd = lambda x, y, h, lon, lat: (x + lon * np.cos(h) - lat * np.sin(h), y + lon * np.sin(h) + lat * np.cos(h))  # noqa: E731
    t, x, y, h, v = anchor(12, 30)      # met from behind: its rear 0.3 m inside the ego's front bumper at t
    px, py = fwd(x, y, h, 4.049 + 2.3 - rng.uniform(0.2, 0.5), rng.uniform(-0.6, 0.6))
    tracks.append(moving(f"veh_front_{seed}", "VEHICLE", t, px, py, h, max(0.3 * v, 0.3), 4.6, 1.9))
    t, x, y, h, v = anchor(10, 30)      # runs into the rear
    px, py = fwd(x, y, h, -1.127 - 2.3 + rng.uniform(0.2, 0.5), rng.uniform(-0.5, 0.5))
    tracks.append(moving(f"veh_rear_{seed}", "VEHICLE", t, px, py, h, v + 4.0, 4.6, 1.9))
    t, x, y, h, v = anchor(15, 38)      # stopped beside the path, half a metre into the ego's swept width
    px, py = fwd(x, y, h, 1.5, rng.choice([-1.0, 1.0]) * (1.1485 + 0.95 - rng.uniform(0.3, 0.6)))
    tracks.append(moving(f"veh_parked_{seed}", "VEHICLE", t, px, py, h + rng.uniform(-0.1, 0.1), 0.0, 4.4, 1.9))
    t, x, y, h, v = anchor(10, 36)      # a pedestrian crossing from the right, at the ego's side at t
    px, py = fwd(x, y, h, rng.uniform(0.0, 2.5), -1.1485 - 0.35 + rng.uniform(0.05, 0.3))
    tracks.append(moving(f"ped_{seed}", "PEDESTRIAN", t, px, py, h + np.pi / 2, 1.4, 0.7, 0.7))
    t, x, y, h, v = anchor(8, 38)       # a static object that is no agent: 0.5, not 0
    px, py = fwd(x, y, h, 4.049 + 0.4 - rng.uniform(0.1, 0.3), rng.uniform(-0.8, 0.8))
    tracks.append(moving(f"cone_{seed}", "TRAFFIC_CONE", t, px, py, rng.uniform(-3.0, 3.0), 0.0, 0.5, 0.5))
    t, x, y, h, v = anchor(14, 30)      # alongside, present for part of the horizon only, cutting in at t
    valid = (times >= t - 6) & (times < t + 12)
    px, py = fwd(x, y, h, rng.uniform(1.0, 3.0), 1.1485 + 1.0 - rng.uniform(0.2, 0.5))
    tracks.append(moving(f"veh_part_{seed}", "VEHICLE", t, px, py, h - 0.05, max(v, 1.0), 4.8, 2.0, valid))
    t, x, y, h, v = anchor(20, 40)      # oncoming, passing close
    px, py = fwd(x, y, h, 6.0, 1.1485 + 1.0 + rng.uniform(0.2, 1.5))
    tracks.append(moving(f"bike_{seed}", "BICYCLE", t, px, py, h + np.pi, 5.0, 1.8, 0.6))
    x, y, h = states[0, 0, :3]          # never counted: a red light across the start and a token collided before
    px, py = fwd(x, y, h, 8.0 + rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3))
    tracks.append(moving(f"{RED_LIGHT}_{seed}", "VEHICLE", 0, px, py, h + rng.uniform(-0.05, 0.05), 0.0, 12.0, 6.0))
    px, py = fwd(x, y, h, 1.0 + rng.uniform(-0.3, 0.3), 0.5 + rng.uniform(-0.3, 0.3))
    tracks.append(moving(f"hit_before_{seed}", "VEHICLE", 0, px, py, h + rng.uniform(-0.05, 0.05), 0.0, 4.0, 1.8))
    return tracks, [f"hit_before_{seed}"]


def seeded_centerline(seed, pose=(0.0, 0.0, 0.0), vertices=24):
    """A gently winding polyline that starts 15 m behind the pose and runs about 90 m ahead, uneven segments."""
    rng = np.random.default_rng(seed)
    xs = np.cumsum(rng.uniform(2.0, 7.0, vertices)) - 15.0
    ys = np.cumsum(rng.normal(0.0, 0.25, vertices))
    return A.to_frame(np.stack([xs, ys], -1), pose)


def with_velocity(states, speed_scale=10.0):
    """pdm_area_ref's synthetic states carry poses only: give them the speed of their own motion (metres per step x
    10), along the heading - the TTC shift follows the heading, whatever the course."""
    s = states.copy()
    step = np.linalg.norm(np.diff(s[..., :2], axis=1), axis=-1)
    s[..., VX] = np.concatenate([step[:, :1], step], axis=1) * speed_scale
    return s


def seeded_scene(seed, states, lanes=3, dt=0.1):
    """Everything a set is scored on, from one seed: (items, tokens, route ids, checks) of pdm_area_ref.seeded_map
    around the set's start pose, then tracks, collided ids and the centerline."""
    pose = tuple(states[0, 0, :3])
    tracks, collided = seeded_tracks(seed, states, dt)
    return A.seeded_map(seed, pose, lanes=lanes) + (tracks, collided, seeded_centerline(seed, pose))


def duck_observation(tracks, collided=()):
    """A duck-typed PDMObservation over ``tracks``, read by the packer through the attributes the issue lists."""
    import types
    t_obs = len(tracks[0]["valid"]) if tracks else T_OBS
    maps = []
    for t in range(t_obs):
        here = [tr for tr in tracks if tr["valid"][t]]
        maps.append(types.SimpleNamespace(
            tokens=[tr["token"] for tr in here],
            _geometries=[types.SimpleNamespace(exterior=types.SimpleNamespace(
                coords=np.concatenate([tr["boxes"][t], tr["boxes"][t][:1]]))) for tr in here]))
    objects = {}
    for tr in tracks:
        obj = types.SimpleNamespace(box=types.SimpleNamespace(center=types.SimpleNamespace(heading=tr["heading"])),
                                    tracked_object_type=types.SimpleNamespace(name=tr["kind"]))
        if tr["is_agent"]:
            obj.velocity = types.SimpleNamespace(magnitude=lambda s=tr["speed"]: s)
        objects[tr["token"]] = obj
    return types.SimpleNamespace(_occupancy_maps=maps, collided_track_ids=list(collided), unique_objects=objects)


def track_items(tracks):
    """The list form ``pack_observations`` takes: absent times as NaN rows."""
    return [(tr["token"], np.where(np.asarray(tr["valid"])[:, None, None], tr["boxes"], np.nan), tr["heading"],
             tr["is_agent"], tr["stopped"]) for tr in tracks]


# ---- the hand-built quirk cases (default parameters: corners 4.049 m ahead of / 1.127 m behind the rear axle and
# 1.1485 m beside it)

def straight(speed, x0=0.0, y=0.0, h=0.0, n=1):
    """(n, T, 11): driving along +x at ``speed`` m/s (per candidate if an array) from x0."""
    s = np.zeros((n, T, 11))
    v = np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,))
    s[..., A.X] = x0 + v[:, None] * 0.1 * np.arange(T)
    s[..., A.Y], s[..., A.HEADING], s[..., VX] = y, h, v[:, None]
    return s


def hand_cases():
    """[(name, dict(states, items, tracks, collided, line, areas override or None), expected)]: answers known by
    construction. ``expected`` pins entries of the results for candidate 0 (or arrays over the candidates)."""
    road = [([A.rect(-50, -8, 150, 8)], "ROADBLOCK", False), ([A.rect(-50, -2, 150, 2)], "LANE", True)]
    two_lanes = [([A.rect(-50, -8, 150, 8)], "ROADBLOCK", False), ([A.rect(-50, -2, 150, 0.5)], "LANE", True),
                 ([A.rect(-50, 0.5, 150, 4)], "LANE", True)]
    line = np.array([[-20.0, 0.0], [200.0, 0.0]])
    times = np.arange(T_OBS) * 0.1
    inf = np.inf
    cases = []

    def case(name, states, tracks, expected, items=road, collided=(), centerline=line, reference=None):
        cases.append((name, dict(states=states, items=items, tracks=tracks, collided=list(collided), line=centerline,
                                 reference=reference), expected))

    # 1. a faster vehicle runs into the rear at index 10 (its front passes the ego's rear at t = 0.943 s: not at fault, it
    # joins the list); the same track then stands at x = 20 and the ego's bumper meets it at index 28: shielded
    ego = straight(5.0)
    case("rear_contact_shields_front", ego,
         [track("a", np.where(times < 2.0, -7.2 + 9.0 * times, 20.0), 0.0, 0.0, 4.6, 1.9, "VEHICLE", 9.0)],
         dict(no_collision=1.0, collision_time_idx=inf, types=[ACTIVE_REAR]))
    # 1b. without the rear contact the front contact counts (the case above is not vacuous)
    case("front_contact_alone", ego, [track("a", np.where(times < 2.0, -40.0, 20.0), 0.0, 0.0, 4.6, 1.9, "VEHICLE", 9.0)],
         dict(no_collision=0.0, collision_time_idx=28.0, types=[ACTIVE_FRONT]))
    # 2. an at-fault contact does not shield, and the FIRST time index is kept: a slow vehicle ahead is met when
    # 5 t + 4.049 >= 12 + t - 2.3, t >= 1.41275 s: index 15; a parked one at 5 t + 4.049 >= 19.7: index 32
    slow = track("slow", 12.0 + 1.0 * times, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 1.0)
    parked = track("parked", 22.0, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)
    case("first_index_kept", ego, [slow, parked], dict(no_collision=0.0, collision_time_idx=15.0,
                                                       types=[ACTIVE_FRONT, STOPPED_TRACK]))
    # 3. a lateral hit (a pedestrian walking into the ego's side) is at fault only off-lane: one lane holds the ego,
    # or the ego straddles two lanes
    ped = track("ped", 1.5 + 5.0 * times, np.minimum(-4.0 + 2.0 * times, -1.3), np.pi / 2, 0.6, 0.6, "PEDESTRIAN", 2.0)
    case("lateral_in_lane", ego, [ped], dict(no_collision=1.0, types=[ACTIVE_LATERAL]))
    case("lateral_straddling", ego, [ped], dict(no_collision=0.0, types=[ACTIVE_LATERAL]), items=two_lanes)
    # 4. a non-agent object gives 0.5, and min with a later agent hit gives 0
    cone = track("cone", 10.0, 0.0, 0.3, 0.5, 0.5, "TRAFFIC_CONE", 0.0)
    case("non_agent_half", ego, [cone], dict(no_collision=0.5, collision_time_idx=12.0, types=[STOPPED_TRACK]))
    case("non_agent_then_agent", ego, [cone, parked], dict(no_collision=0.0, collision_time_idx=12.0))
    # 5. stopped ego at contact is never at fault, and the track is shielded afterwards: a vehicle backs into the
    # standing ego and stays; the ego then drives on into it
    stand_then_go = straight(0.0)
    stand_then_go[0, 20:, VX] = 3.0
    stand_then_go[0, 20:, A.X] = 0.3 * np.arange(1, T - 19)
    backing = track("backing", np.maximum(12.0 - 6.0 * times, 6.2), 0.0, 0.0, 4.6, 1.9, "VEHICLE", 6.0)
    case("stopped_ego_shields", stand_then_go, [backing], dict(no_collision=1.0, types=[STOPPED_EGO]))
    # 6. TTC below 5e-3 m/s neither counts nor shields: creeping at 1e-3 m/s under a vehicle that overlaps the ego (a
    # hit at k = 0 at every t); from index 25 the ego moves, and the same track, ahead, is an infraction there
    creep = straight(1e-3)
    creep[0, 25:, VX] = 4.0
    creep[0, 25:, A.X] = creep[0, 24, A.X] + 0.4 * np.arange(1, T - 24)
    case("ttc_slow_neither_counts_nor_shields", creep, [track("on_top", 2.0, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)],
         dict(ttc=0.0, ttc_time_idx=25.0))
    # 7. TTC takes the first k at a t; a non-infraction at k = 0 shields k = 3 of the same t: the track overlaps the
    # ego's rear in maps 0..2 (k = 0 hit, behind: no infraction) and stands 9 m ahead from map 3 on (k = 3 hit, ahead)
    jump = np.where(np.arange(T_OBS) < 3, -3.0, 9.0)
    fast = straight(10.0)
    fast[0, :, A.X] = 0.0      # the pose stands still (the quads' shifts come from the velocity alone)
    case("ttc_behind_at_k0_shields_k3", fast, [track("jump", jump, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)],
         dict(ttc=1.0, ttc_hits=[0]))
    case("ttc_ahead_at_k3", fast, [track("far", 9.0, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)],
         dict(ttc=0.0, ttc_time_idx=0.0, ttc_hits=[1]))
    # 8. the intersection rule uses the REAR AXLE against INTERSECTION polygons only: a track to the side (neither
    # ahead nor behind) overlapping the ego; the rear axle inside an INTERSECTION polygon -> infraction; the same
    # polygon as a ROADBLOCK, or an INTERSECTION that holds the corners' front half but not the rear axle -> none
    side = track("side", 1.5, 2.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)
    lane = ([A.rect(-50, -2, 150, 2)], "LANE", True)
    case("ttc_axle_in_intersection", fast, [side], dict(ttc=0.0, ttc_hits=[1]),
         items=[([A.rect(-50, -8, 150, 8)], "INTERSECTION", False), lane])
    case("ttc_axle_in_roadblock", fast, [side], dict(ttc=1.0, ttc_hits=[0]))
    case("ttc_axle_outside_intersection", fast, [side], dict(ttc=1.0, ttc_hits=[0]),
         items=road + [([A.rect(0.5, -8, 150, 8)], "INTERSECTION", False)])
    # 9. a track valid at t but absent at t + 3: the k = 3 quad would meet it
    gone = track("gone", 9.0, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0, valid=np.arange(T_OBS) < 3)
    case("ttc_absent_at_t_plus_3", fast, [gone], dict(ttc=1.0, ttc_hits=[-1]))
    # 10. a red-light token and a previously collided token are dropped
    case("dropped_tokens", ego, [track(f"{RED_LIGHT}_7", 10.0, 0.0, 0.0, 6.0, 6.0, "VEHICLE", 0.0),
                                 track("before", 12.0, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)],
         dict(no_collision=1.0, ttc=1.0), collided=["before"])
    # 11. progress: against the centerline it clips at 0; past both ends it clamps
    back = straight(5.0, x0=30.0, h=np.pi)
    back[0, :, A.X] = 30.0 - 0.5 * np.arange(T)
    case("progress_backwards", back, [], dict(raw_progress=0.0))
    short = np.array([[3.0, 0.0], [8.0, 0.0], [11.0, 0.0]])
    case("progress_clamped", ego, [], dict(raw_progress=8.0), centerline=short)
    # 12. pmax <= 5: the progress term is 1 or 0 by multiplier (three candidates: slow, slow off-road, slow)
    slow3 = straight(np.array([0.5, 0.6, 0.4]), n=3)
    slow3[1, :, A.Y] = 20.0     # off the roadblock: drivable_area 0
    case("small_pmax", slow3, [], dict(progress=np.array([1.0, 0.0, 1.0]), drivable_area=np.array([1.0, 0.0, 1.0])))
    # 13. a NaN p takes the second branch for the whole group
    nan3 = straight(np.array([5.0, 6.0, 7.0]), n=3)
    nan3[2, T - 1, A.X] = np.nan
    case("nan_progress", nan3, [], dict(progress=np.array([1.0, 1.0, 0.0])))
    # group versus pair: with a reference of 30 m the 20 m candidate scores 20 / 30 of the progress weight
    case("pair_reference", straight(5.0), [], dict(progress=20.0 / 30.0), reference=30.0)
    return cases
