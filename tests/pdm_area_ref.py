"""numpy restatement of the PDM scorer's map compliance: the five points of every state, the three ego-area flags and
the two scores that need nothing else (dd_ego_areas, include/ddmi.h).

Restates, with every quirk kept:
  state_array_to_coords_array   pdm_planner/utils/pdm_array_representation.py:142-181 (translate_lon_and_lat,
                                utils/pdm_geometry_utils.py:36-58: cos(h + pi/2) of the rounded sum, not -sin h)
  PDMScorer._calculate_ego_area                        pdm_planner/scoring/pdm_scorer.py:240-291
  PDMScorer._calculate_drivable_area_compliance        :351-358
  PDMScorer._calculate_driving_direction_compliance    :360-396 (a window of int(horizon / dt) + 1 samples; the
                                progress of step t counts where the flag AT t is set; p[0] = 0)
Containment stands in for shapely.vectorized.contains (interior only: a point on an edge or a vertex is outside, a
point in a hole is outside): an even-odd crossing count over coordinate differences. tests/golden/make_area_golden.py
runs the reference's own code over the same primitive and checks the primitive on every golden point against an
independent half-plane predicate; tests/test_ego_areas.py holds this file to those goldens.

Also the seeded inputs the goldens and the tests share: the map laid around a start pose (``seeded_map``), the
synthetic states, the hand-built cases and the star polygon.
"""
import numpy as np

T = 41
X, Y, HEADING = 0, 1, 2
MULTIPLE_LANES, NON_DRIVABLE, ONCOMING = 0, 1, 2          # EgoAreaIndex
FRONT_LEFT, REAR_LEFT, REAR_RIGHT, FRONT_RIGHT, CENTER = range(5)   # BBCoordsIndex
LANE_LAYERS = ("LANE", "LANE_CONNECTOR")
DRIVABLE_LAYERS = ("ROADBLOCK", "INTERSECTION", "DRIVABLE_AREA", "CARPARK_AREA")
# SemanticMapLayer's values for the six names (nuPlan's maps_datatypes; only their identity matters)
LAYER_IDS = dict(LANE=0, INTERSECTION=1, CARPARK_AREA=5, ROADBLOCK=14, LANE_CONNECTOR=16, DRIVABLE_AREA=18)

_FRONT, _REAR, _WIDTH = 4.049, 1.127, 2.297   # get_pacifica_parameters, as include/ddmi.h quotes them
DEFAULTS = dict(half_length=(_FRONT + _REAR) / 2.0, half_width=_WIDTH / 2.0,
                rear_axle_to_center=abs((_FRONT + _REAR) / 2.0 - _REAR), dt=0.1, driving_direction_horizon=1.0,
                driving_direction_compliance_threshold=2.0, driving_direction_violation_threshold=6.0)
# the non-default set of the goldens: other vehicle lengths, dt, horizon and thresholds
ALT = dict(half_length=2.2, half_width=0.95, rear_axle_to_center=1.3, dt=0.125, driving_direction_horizon=0.5,
           driving_direction_compliance_threshold=1.0, driving_direction_violation_threshold=3.0)


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        assert k in p, k
        p[k] = v
    return p


def horizon_steps(p):
    return int(p["driving_direction_horizon"] / p["dt"])


def coords(states, p=None):
    """(N, T, 11) states -> (N, T, 5, 2) points in BBCoordsIndex order."""
    p = p or DEFAULTS
    h = states[..., HEADING]
    cos, sin = np.cos(h), np.sin(h)
    r = p["rear_axle_to_center"]
    centers = states[..., :2] + np.stack([r * cos, r * sin], axis=-1)
    half_pi = np.pi / 2.0

    def corner(lon, lat):
        return centers + np.stack([(lat * np.cos(h + half_pi)) + (lon * cos),
                                   (lat * np.sin(h + half_pi)) + (lon * sin)], axis=-1)

    out = np.zeros(states.shape[:-1] + (5, 2))
    out[..., CENTER, :] = centers
    out[..., FRONT_LEFT, :] = corner(p["half_length"], p["half_width"])
    out[..., FRONT_RIGHT, :] = corner(p["half_length"], -p["half_width"])
    out[..., REAR_LEFT, :] = corner(-p["half_length"], p["half_width"])
    out[..., REAR_RIGHT, :] = corner(-p["half_length"], -p["half_width"])
    return out


def contains(rings, x, y, block=2048):
    """Points strictly inside the polygon made of ``rings`` under the even-odd rule (the closing edge of a ring is
    implied). Differences before products: map coordinates sit at 1e6 m, where a product of absolute coordinates is
    good to 1e-3 m^2 only. A NaN coordinate is outside. Edges are taken ``block`` at a time against all points."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    px, py = x.reshape(-1, 1), y.reshape(-1, 1)
    parity = np.zeros(px.shape[0], dtype=bool)
    on_edge = np.zeros(px.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for ring in rings:
            v = np.asarray(ring, dtype=np.float64)
            w = np.roll(v, -1, axis=0)
            for e in range(0, len(v), block):
                a, b, c, d = v[e:e + block, 0], v[e:e + block, 1], w[e:e + block, 0], w[e:e + block, 1]
                cross = (c - a) * (py - b) - (px - a) * (d - b)
                flips = ((b > py) != (d > py)) & np.where(d > b, cross > 0.0, cross < 0.0)
                parity ^= (flips.sum(-1) & 1).astype(bool)
                on_edge |= ((cross == 0.0) & (px >= np.minimum(a, c)) & (px <= np.maximum(a, c))
                            & (py >= np.minimum(b, d)) & (py <= np.maximum(b, d))).any(-1)
    return (parity & ~on_edge).reshape(x.shape)


def in_polygons(items, pts):
    """(polygons, ...) bool: PDMDrivableMap.points_in_polygons over ``items`` = [(rings, layer, on_route), ...]."""
    out = np.zeros((len(items),) + pts.shape[:-1], dtype=bool)
    for i, (rings, _, _) in enumerate(items):
        out[i] = contains(rings, pts[..., 0], pts[..., 1])
    return out


def areas_from(inside, items):
    """(polygons, N, T, 5) containment -> (N, T, 3) flags, as _calculate_ego_area takes them."""
    lane = [i for i, it in enumerate(items) if it[1] in LANE_LAYERS]
    drivable = [i for i, it in enumerate(items) if it[1] in DRIVABLE_LAYERS]
    route = [i for i in lane if items[i][2]]
    corners, center = inside[..., :4], inside[..., 4]
    per_lane = corners[lane].sum(-1)                         # (lanes, N, T): corners held by each lane polygon
    out = np.zeros(inside.shape[1:3] + (3,), dtype=bool)
    out[..., MULTIPLE_LANES] = ((per_lane > 0).sum(0) > 1) & (per_lane != 4).all(0)
    out[..., NON_DRIVABLE] = (corners[drivable].sum(0) > 0).sum(-1) < 4
    out[..., ONCOMING] = center[route].sum(0) == 0
    return out


def oncoming_progress(centers, oncoming, h):
    """m: the largest sum of h + 1 consecutive per-step progresses, a step counting where the flag at its END is
    set. np.max keeps a NaN."""
    p = np.zeros(centers.shape[:2])
    with np.errstate(invalid="ignore"):
        p[:, 1:] = np.linalg.norm(centers[:, 1:] - centers[:, :-1], axis=-1)
    p[~oncoming] = 0.0
    w = np.stack([p[:, max(0, t - h):t + 1].sum(-1) for t in range(p.shape[1])], axis=-1)
    return w.max(-1)


def direction_score(m, p=None):
    p = p or DEFAULTS
    out = np.zeros(m.shape)
    with np.errstate(invalid="ignore"):
        out[m < p["driving_direction_violation_threshold"]] = 0.5
        out[m < p["driving_direction_compliance_threshold"]] = 1.0
    return out


def ego_areas(states, items, p=None):
    """One scene: (N, T, 11) states against ``items``. Returns dict(coords, areas, drivable_area, driving_direction,
    m)."""
    p = p or DEFAULTS
    pts = coords(states, p)
    areas = areas_from(in_polygons(items, pts), items)
    m = oncoming_progress(pts[:, :, CENTER], areas[..., ONCOMING], horizon_steps(p))
    return dict(coords=pts, areas=areas, drivable_area=np.where(areas[..., NON_DRIVABLE].any(-1), 0.0, 1.0),
                driving_direction=direction_score(m, p), m=m)


def ego_areas_grouped(states, maps, p=None):
    """(G, n, T, 11) states, scene g on maps[g]; the results stacked over the scenes."""
    parts = [ego_areas(states[g], maps[g], p) for g in range(len(maps))]
    return {k: np.stack([q[k] for q in parts]) for k in parts[0]}


# ---- the bars of the GPU tests (derived in the issue)

def coords_bar(ref, p=None):
    """Per value: two roundings at the coordinate's magnitude and a few ulp of sin / cos error on the lever arms."""
    p = p or DEFAULTS
    arms = p["half_length"] + p["half_width"] + p["rear_axle_to_center"]
    with np.errstate(invalid="ignore"):
        return 2.0 * np.spacing(np.abs(ref)) + 16.0 * 2.0 ** -52 * arms


def progress_bar(ref_coords):
    """Eleven steps, each a difference of two centers that may each sit one rounding off."""
    return 44.0 * np.spacing(np.nanmax(np.abs(ref_coords))) + 1e-12


# ---- distance to the map's edges (the goldens keep every point 1e-6 m away from every edge)

def edge_distance(items, pts, block=2048):
    """Smallest distance of any finite point of ``pts`` (..., 2) to any edge of any polygon of ``items``."""
    q = pts.reshape(-1, 2)
    q = q[np.isfinite(q).all(-1)][:, None, :]
    best = np.inf
    if not len(q):
        return best
    for rings, _, _ in items:
        for ring in rings:
            v = np.asarray(ring, dtype=np.float64)
            w = np.roll(v, -1, axis=0)
            for e in range(0, len(v), block):
                a, ab = v[e:e + block], w[e:e + block] - v[e:e + block]
                den = (ab * ab).sum(-1)
                s = np.clip(((q - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
                best = min(best, float(np.linalg.norm(q - (a + s[..., None] * ab), axis=-1).min()))
    return best


# ---- seeded inputs

def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def to_frame(ring, pose):
    """Local (x forward, y left) -> the frame of pose = (x0, y0, h0)."""
    x0, y0, h0 = pose
    c, s = np.cos(h0), np.sin(h0)
    r = np.asarray(ring, dtype=np.float64)
    return np.stack([x0 + c * r[:, 0] - s * r[:, 1], y0 + s * r[:, 0] + c * r[:, 1]], axis=-1)


def seeded_map(seed, pose=(0.0, 0.0, 0.0), lanes=3):
    """A map laid around a start pose: ``lanes`` adjacent lanes under a roadblock (the one to the left off route), an
    intersection with a hole (a traffic island), a straight on-route lane connector and an L-shaped (non-convex)
    off-route one across it, an exit lane under a second roadblock, a carpark behind a 1 m strip of nothing, and a
    drivable-area patch flush with the first roadblock. Returns (items, tokens, route_lane_ids, checks): items =
    [(rings, layer, on_route)], checks[i] = how the generator re-derives containment in polygon i independently -
    ("convex", ring), ("union", [convex rings]) or ("holes", exterior, [holes]), all rings convex.
    One roadblock's token is among the route ids: only lane-class polygons may count for the route."""
    rng = np.random.default_rng(seed)
    j = lambda: float(rng.uniform(-0.2, 0.2))  # noqa: E731
    w = 3.5 + j()
    low = -0.5 * w - (w if lanes == 3 else 0.0)
    top = low + lanes * w
    xa, xb, xc, xd = -12.0 + j(), 22.0 + j(), 46.0 + j(), 75.0 + j()
    local, layers, route, checks = [], [], [], []

    def add(rings, layer, on_route, check=None):
        local.append(rings), layers.append(layer), route.append(on_route)
        checks.append(check if check is not None else ("convex", rings[0]))

    add([rect(xa, low, xb, top)], "ROADBLOCK", True)     # its token is in the route ids, and must not count
    for i in range(lanes):
        y0 = low + i * w
        add([rect(xa, y0, xb, y0 + w)], "LANE", y0 + w <= 0.5 * w + 1e-9)   # the lane(s) left of the ego's: off route
    hole = rect(30.0 + j(), 6.0 + j(), 33.0 + j(), 9.0 + j())
    inter = rect(xb, -14.0 + j(), xc, 14.0 + j())
    add([inter, hole], "INTERSECTION", False, ("holes", inter, [hole]))
    add([rect(xb, -0.5 * w, xc, 0.5 * w)], "LANE_CONNECTOR", True)
    x1, x2, ytop = 30.0 + j(), 34.0 + j(), float(inter[2, 1])
    ell = np.array([[xb, -0.5 * w], [x2, -0.5 * w], [x2, ytop], [x1, ytop], [x1, 0.5 * w], [xb, 0.5 * w]])
    add([ell], "LANE_CONNECTOR", False, ("union", [rect(xb, -0.5 * w, x2, 0.5 * w), rect(x1, -0.5 * w, x2, ytop)]))
    add([rect(xc, -1.5 * w, xd, 1.5 * w)], "ROADBLOCK", False)
    add([rect(xc, -0.5 * w, xd, 0.5 * w)], "LANE", True)
    add([rect(0.0 + j(), low - 9.0 + j(), 18.0 + j(), low - 1.0)], "CARPARK_AREA", False)
    add([rect(0.0 + j(), top, 10.0 + j(), top + 5.0 + j())], "DRIVABLE_AREA", False)
    tokens = [f"{seed}_{i}" for i in range(len(local))]
    ids = [t for t, r in zip(tokens, route) if r]
    move = lambda c: (c[0],) + tuple(to_frame(r, pose) if isinstance(r, np.ndarray)  # noqa: E731
                                     else [to_frame(q, pose) for q in r] for r in c[1:])
    items = [([to_frame(r, pose) for r in rings], layer, on and layer in LANE_LAYERS)
             for rings, layer, on in zip(local, layers, route)]
    return items, tokens, ids, [move(c) for c in checks]


def synthetic_states(seed, n=96):
    """(n, T, 11): x, y, heading only. Large headings (several turns, nothing to do with the direction of travel) and
    lateral motion over the seeded map at the origin."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, T, 11))
    speed = rng.uniform(0.0, 1.6, (n, 1))                          # metres per step
    course = rng.uniform(-0.9, 0.9, (n, 1)) + np.cumsum(rng.normal(0.0, 0.05, (n, T)), axis=1)
    step = speed[..., None] * np.stack([np.cos(course), np.sin(course)], axis=-1)
    step[:, 0] = 0.0
    start = np.stack([rng.uniform(-6.0, 20.0, n), rng.uniform(-7.0, 7.0, n)], axis=-1)
    s[..., :2] = start[:, None] + np.cumsum(step, axis=1)
    s[..., HEADING] = rng.uniform(-7.0, 7.0, (n, 1)) + np.cumsum(rng.normal(0.0, 0.15, (n, T)), axis=1)
    return s


def pose_states(xs, ys=0.0, hs=0.0):
    s = np.zeros((1, T, 11))
    s[0, :, X], s[0, :, Y], s[0, :, HEADING] = xs, ys, hs
    return s


def hand_cases():
    """[(name, items, states (1, T, 11), expected)]: answers known by construction, under the default parameters (the
    center is 1.461 m ahead of the rear axle; the corners 2.588 m ahead of / behind and 1.1485 m beside the center).
    ``expected`` holds what the case pins: areas columns constant over time as {flag index: bool}, and scores."""
    big = rect(-10.0, -5.0, 10.0, 5.0)
    t = np.arange(T)
    cases = []
    # 1. straddling two lanes while a lane connector holds all four corners: not in multiple lanes
    cases.append(("straddle_under_connector",
                  [([rect(-10, -5, 10, 0)], "LANE", True), ([rect(-10, 0, 10, 5)], "LANE", False),
                   ([rect(-10, -3, 10, 3)], "LANE_CONNECTOR", False), ([big], "ROADBLOCK", False)],
                  pose_states(0.0, 0.2), dict(areas={MULTIPLE_LANES: False, NON_DRIVABLE: False}, drivable_area=1.0)))
    # 1b. the same without the connector: in multiple lanes (the case above is not vacuous)
    cases.append(("straddle",
                  [([rect(-10, -5, 10, 0)], "LANE", True), ([rect(-10, 0, 10, 5)], "LANE", False),
                   ([big], "ROADBLOCK", False)],
                  pose_states(0.0, 0.2), dict(areas={MULTIPLE_LANES: True, NON_DRIVABLE: False}, drivable_area=1.0)))
    # 2. inside a lane with no drivable-class polygon under it: non-drivable
    cases.append(("lane_without_roadblock", [([rect(-10, -3, 10, 3)], "LANE", True)], pose_states(0.0),
                  dict(areas={MULTIPLE_LANES: False, NON_DRIVABLE: True, ONCOMING: False}, drivable_area=0.0,
                       driving_direction=1.0)))
    # 3. the four corners in four different drivable polygons: drivable
    cases.append(("four_polygons",
                  [([rect(-10, -10, 1, 0.3)], "ROADBLOCK", False), ([rect(1, -10, 10, 0.3)], "INTERSECTION", False),
                   ([rect(-10, 0.3, 1, 10)], "DRIVABLE_AREA", False), ([rect(1, 0.3, 10, 10)], "CARPARK_AREA", False)],
                  pose_states(0.0), dict(areas={NON_DRIVABLE: False, ONCOMING: True}, drivable_area=1.0)))
    # 4. the center on route, the rear axle off route: not oncoming
    cases.append(("center_not_rear_axle",
                  [([rect(1, -3, 10, 3)], "LANE", True), ([rect(-10, -3, 1, 3)], "LANE", False)], pose_states(0.0),
                  dict(areas={ONCOMING: False}, driving_direction=1.0)))
    # 5. a roadblock whose token is in the route ids, a lane that is not: oncoming
    cases.append(("roadblock_on_route", [([big], "ROADBLOCK", True), ([big], "LANE", False)],
                  pose_states(0.1 * t), dict(areas={ONCOMING: True, NON_DRIVABLE: False}, drivable_area=1.0,
                                             driving_direction=1.0)))
    # 6. the front-left corner (4.049, 1.1485) in a hole: non-drivable
    cases.append(("corner_in_hole", [([big, rect(3.5, 0.8, 4.5, 1.5)], "ROADBLOCK", False)], pose_states(0.0),
                  dict(areas={NON_DRIVABLE: True}, drivable_area=0.0)))
    # 7. always oncoming at 0.19 m per step: eleven samples reach 2.09, ten only 1.9 -> 0.5
    cases.append(("eleven_samples", [([rect(-10, -5, 30, 5)], "ROADBLOCK", False)], pose_states(0.19 * t),
                  dict(areas={ONCOMING: True}, driving_direction=0.5, m=11 * 0.19)))
    # 8. the route has a gap over center x in (10, 12.5): the center enters it by a 2.5 m step (t = 11), moves 0.1 m
    # inside (t = 12) and leaves by a 0.2 m step. With the flag AT t: 2.5 + 0.1 = 2.6 -> 0.5 (the flag at t - 1 would
    # give 0.1 + 0.2 -> 1.0)
    cx = np.concatenate([np.linspace(8.8, 9.8, 11), [12.3, 12.4, 12.6], 12.6 + 0.1 * np.arange(1, T - 13)])
    cases.append(("flag_at_t",
                  [([rect(-10, -3, 10, 3)], "LANE", True), ([rect(12.5, -3, 40, 3)], "LANE_CONNECTOR", True)],
                  pose_states(cx - DEFAULTS["rear_axle_to_center"]),
                  dict(driving_direction=0.5, m=2.6, oncoming_at=[11, 12])))
    # 9. an empty map: every state non-drivable and oncoming, never in multiple lanes
    cases.append(("empty_map", [], pose_states(0.1 * t),
                  dict(areas={MULTIPLE_LANES: False, NON_DRIVABLE: True, ONCOMING: True}, drivable_area=0.0,
                       driving_direction=1.0, m=1.1)))
    return cases


def star_polygon(seed, n=40000, center=(3.0, 1.0), radius=(6.0, 14.0)):
    """One ring of n vertices: a star around ``center`` whose radius alternates at random between the two bounds."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * (np.arange(n) + rng.uniform(0.1, 0.9, n)) / n
    rad = rng.uniform(radius[0], radius[1], n)
    return np.stack([center[0] + rad * np.cos(ang), center[1] + rad * np.sin(ang)], axis=-1)
