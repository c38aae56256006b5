"""numpy restatement of PDM-Closed's proposal generation (dd_proposals, include/ddmi.h).

Restates, with every quirk kept:
  PDMGenerator.generate_proposals, _initialize_states, _update_leading_agents, _get_driving_corridor,
  _get_leading_agent_velocity, _update_idm_states, _update_states_se2    proposal/pdm_generator.py:68-95,185-366
  BatchIDMPolicy.propagate                                                proposal/batch_idm_policy.py:102-168
  PDMPath.interpolate / substring                                         utils/pdm_path.py:67-105
Quirks beyond the obvious ones:
  * the leading-agent row of time index 1 is the zero row the arrays are created with (index 1 is odd: it copies row 0),
    so the first IDM step runs against a leader at progress 0, velocity 0;
  * _update_leading_agents fills ONE scratch row for all proposals of a path at a time index and never clears it: a
    track or red-light leader keeps the rear length a free-driving proposal before it wrote, and a red-light leader
    keeps the velocity a track leader before it wrote. The proposals of a path are therefore walked in order and the
    two values carried (``carry``).
  * the corridor's fast path keeps vertices only; shapely's substring (restated from memory) takes over with one or no
    vertex inside.

shapely cannot be run here. The corridor is this project's exact offset region (one rectangle per segment, lengthened
by r at the two free ends; a closed disc of radius r at every interior vertex; a single point gives a disc), the
projection is pdm_collision_ref.project's rule, the distance is the least point-to-segment distance of the two
boundaries, zero where they intersect, on coordinates relative to the ego quad's first corner.

Every continuous chain (projection, interpolation, distance, IDM) runs in the float type ``ft``: float64 is the
restatement, numpy.longdouble measures its conditioning for the bars. The discrete predicates on the inputs alone
(corridor membership) are float64 in both.
"""
import numpy as np

import pdm_area_ref as A
import pdm_collision_ref as R

T = A.T                          # 41 states per proposal
IDM_DEFAULTS = dict(min_gap_to_lead_agent=1.0, headway_time=1.5, accel_max=1.5, decel_max=3.0, dt=0.1,
                    acceleration_exponent=10, leading_agent_update_rate=2, corridor_poses=50)
SPEED_LIMIT_FRACTIONS = (0.2, 0.4, 0.6, 0.8, 1.0)
CORRIDOR_MARGIN = 5e-3           # metres: membership must not change when r moves by this much
FREE = -1


def idm_params(**over):
    p = dict(IDM_DEFAULTS)
    for k, v in over.items():
        assert k in p, k
        p[k] = v
    return p


# ---- paths

def path_of(xyh):
    """What pack_paths makes of a (V, 3) array: the heading unwrapped, the cumulative progress as the reference's
    calculate_progress forms it (diff, norm over the coordinate axis, cumsum)."""
    a = np.array(xyh, dtype=np.float64)
    a[:, 2] = np.unwrap(a[:, 2], axis=0)
    diff = np.concatenate(([np.diff(a[:, 0])], [np.diff(a[:, 1])]), axis=0, dtype=np.float64)
    progress = np.cumsum(np.append(0.0, np.linalg.norm(diff, axis=0)), dtype=np.float64)
    return dict(xyh=a, progress=progress)


def parallel_path(xyh, offset):
    """parallel_discrete_path's arithmetic on a (V, 3) array."""
    a = np.array(xyh, dtype=np.float64)
    theta = a[:, 2] + np.pi / 2
    return np.stack([a[:, 0] + np.cos(theta) * offset, a[:, 1] + np.sin(theta) * offset, a[:, 2]], axis=-1)


def interpolate(path, distances, ft=np.float64):
    """PDMPath.interpolate(distances, as_array=True): clip, scipy's linear interp1d, arctan2(sin, cos), NaN -> 0."""
    s, y = path["progress"].astype(ft), path["xyh"].astype(ft)
    d = np.atleast_1d(np.asarray(distances, dtype=ft))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.clip(d, ft(1e-5), s[-1])
        hi = np.clip(np.searchsorted(s, c), 1, len(s) - 1)
        lo = hi - 1
        slope = (y[hi] - y[lo]) / (s[hi] - s[lo])[:, None]
        out = slope * (c - s[lo])[:, None] + y[lo]
        out[:, 2] = np.arctan2(np.sin(out[:, 2]), np.cos(out[:, 2]))
    out[np.isnan(out)] = 0.0
    return out


def project(line, x, y, ft=np.float64):
    """pdm_collision_ref.project's rule for one point, in ``ft``."""
    line = np.asarray(line).astype(ft)
    x, y = ft(x), ft(y)
    best, at, passed = ft(np.inf), ft(np.nan), ft(0.0)
    for a, b in zip(line[:-1], line[1:]):
        dx, dy = b[0] - a[0], b[1] - a[1]
        len2 = dx * dx + dy * dy
        length = np.sqrt(len2)
        wx, wy = x - a[0], y - a[1]
        s = (wx * dx + wy * dy) / len2 if len2 > 0.0 else ft(0.0)
        s = ft(0.0) if s < 0.0 else (ft(1.0) if s > 1.0 else s)
        ex, ey = wx - s * dx, wy - s * dy
        d2 = ex * ex + ey * ey
        if d2 < best:
            best, at = d2, passed + s * length
        passed = passed + length
    return at


# ---- the corridor

def _point_at(path, d):
    """The point of the polyline at arc length d, by the path's own cumulative progress (shapely's interpolate)."""
    s, xy = path["progress"], path["xyh"][:, :2]
    hi = int(np.clip(np.searchsorted(s, d), 1, len(s) - 1))
    lo = hi - 1
    if s[hi] == s[lo]:
        return xy[lo].copy()
    return xy[lo] + ((d - s[lo]) / (s[hi] - s[lo])) * (xy[hi] - xy[lo])


def corridor_points(path, ego_progress, max_target, p):
    """(points (M, 2), fallback): PDMPath.substring(ego, ego + |max target| * corridor_poses * dt)."""
    s, xy = path["progress"], path["xyh"][:, :2]
    far = ego_progress + abs(max_target) * p["corridor_poses"] * p["dt"]
    start, end = float(np.clip(ego_progress, 0.0, s[-1])), float(np.clip(far, 0.0, s[-1]))
    inside = (start <= s) & (s <= end)
    if inside.sum() > 1:
        return xy[inside].copy(), False
    if start == end:
        return _point_at(path, start)[None], True
    between = xy[(start < s) & (s < end)]
    return np.concatenate([_point_at(path, start)[None], between, _point_at(path, end)[None]]), True


def corridor_pieces(points, r):
    """(rectangles (n, 4, 2), disc centres (m, 2)) of the exact offset region with square caps."""
    pts = np.asarray(points, dtype=np.float64)
    seg = [(i, pts[i + 1] - pts[i]) for i in range(len(pts) - 1)]
    seg = [(i, d) for i, d in seg if (d * d).sum() > 0.0]
    if not seg:
        return np.zeros((0, 4, 2)), pts[:1].copy()
    rects = []
    for k, (i, d) in enumerate(seg):
        u = d / np.sqrt((d * d).sum())
        n = np.array([-u[1], u[0]])
        a = pts[i] - (r * u if k == 0 else 0.0)
        b = pts[i + 1] + (r * u if k == len(seg) - 1 else 0.0)
        rects.append(np.stack([a + r * n, b + r * n, b - r * n, a - r * n]))
    return np.stack(rects), pts[1:-1].copy()


def _point_segment(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    len2 = dx * dx + dy * dy
    wx, wy = px - ax, py - ay
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(len2 > 0.0, (wx * dx + wy * dy) / np.where(len2 > 0.0, len2, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)
    ex, ey = wx - s * dx, wy - s * dy
    return ex * ex + ey * ey


def ring_meets_pieces(ring, rects, discs, r):
    """Closed intersection of the simple ring (n, 2) - a box is a ring of four - with the region."""
    ring = np.asarray(ring, dtype=np.float64)
    nxt = np.roll(ring, -1, axis=0)
    edges = np.stack([ring, nxt], axis=1)                       # (n, 2, 2)
    for q in rects:
        if R.segment_touches(edges, q[None]).any() or bool(A.contains([ring], q[0, 0], q[0, 1])):
            return True
    for c in discs:
        rel, rel_n = ring - c, nxt - c
        if bool(A.contains([rel], 0.0, 0.0)):
            return True
        if (_point_segment(0.0, 0.0, rel[:, 0], rel[:, 1], rel_n[:, 0], rel_n[:, 1]) <= r * r).any():
            return True
    return False


def meets_corridor(ring, points, r, margin=CORRIDOR_MARGIN):
    """(met, steady): membership, and whether it is the same with r - margin and r + margin."""
    ring, pts = np.asarray(ring, dtype=np.float64), np.asarray(points, dtype=np.float64)
    reach = 2.0 * r + 1.0        # far outside the region's bounding box: nothing to test
    if ((ring.min(0) > pts.max(0) + reach) | (ring.max(0) < pts.min(0) - reach)).any():
        return False, True
    got = [ring_meets_pieces(ring, *corridor_pieces(points, rr), rr) for rr in (r, r - margin, r + margin)]
    return got[0], got[0] == got[1] == got[2]


def _winding(ring, p):
    """The winding number of the ring about p by summed angles (independent of the crossing rule)."""
    v = np.asarray(ring, dtype=np.float64) - p
    w = np.roll(v, -1, axis=0)
    ang = np.arctan2(v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0], v[:, 0] * w[:, 0] + v[:, 1] * w[:, 1])
    return int(np.rint(ang.sum() / (2.0 * np.pi)))


def _rim(ring, spacing):
    out = []
    for a, b in zip(ring, np.roll(ring, -1, axis=0)):
        m = max(2, int(np.hypot(*(b - a)) / spacing) + 2)
        out.append(a + np.linspace(0.0, 1.0, m)[:, None] * (b - a))
    return np.concatenate(out)


def independent_meets(ring, points, r, spacing=1e-3):
    """No code shared with ring_meets_pieces: dense samples of the object's boundary (every millimetre, the vertices
    among them) tested POINT by point against the region (along / across coordinates of every segment, the distance to
    every interior vertex), and the centre line's vertices tested against the object by a summed-angle winding number
    (an object that swallows the corridor). Right wherever the object is CORRIDOR_MARGIN inside or outside."""
    pts = np.asarray(points, dtype=np.float64)
    ring = np.asarray(ring, dtype=np.float64)
    o = pts[0]
    pts, ring = pts - o, ring - o
    keep = [0] + [i for i in range(1, len(pts)) if np.hypot(*(pts[i] - pts[i - 1])) > 0.0]
    pts = pts[keep]
    reach = np.hypot(*(ring - ring.mean(0)).T).max()
    far = min(np.hypot(*(ring.mean(0) - q)) for q in _rim(np.concatenate([pts, pts[::-1]]), 0.5)) if len(pts) > 1 \
        else np.hypot(*(ring.mean(0) - pts[0]))
    if far > reach + 2.0 * r + 1.0:
        return False
    rim = _rim(ring, spacing)
    if len(pts) == 1:
        inside = np.hypot(rim[:, 0] - pts[0, 0], rim[:, 1] - pts[0, 1]) <= r
    else:
        inside = np.zeros(len(rim), dtype=bool)
        for i, (a, b) in enumerate(zip(pts[:-1], pts[1:])):
            length = np.hypot(*(b - a))
            u = (b - a) / length
            along = (rim[:, 0] - a[0]) * u[0] + (rim[:, 1] - a[1]) * u[1]
            across = (rim[:, 1] - a[1]) * u[0] - (rim[:, 0] - a[0]) * u[1]
            lo = -r if i == 0 else 0.0
            hi = length + (r if i == len(pts) - 2 else 0.0)
            inside |= (along >= lo) & (along <= hi) & (np.abs(across) <= r)
        for c in pts[1:-1]:
            inside |= np.hypot(rim[:, 0] - c[0], rim[:, 1] - c[1]) <= r
    return bool(inside.any()) or any(_winding(ring, q) != 0 for q in pts)


def ring_centroid(ring, ft=np.float64):
    """The polygon area centroid, relative coordinates against the first vertex; the vertex mean for zero area."""
    v = np.asarray(ring).astype(ft)
    rel = v - v[0]
    nxt = np.roll(rel, -1, axis=0)
    cross = rel[:, 0] * nxt[:, 1] - nxt[:, 0] * rel[:, 1]
    area = cross.sum()
    if area == 0.0:
        return v[0] + rel.sum(0) / ft(len(v))
    return v[0] + ((rel + nxt) * cross[:, None]).sum(0) / (ft(3.0) * area)


def quad_centroid(b, ft=np.float64):
    """pdm_collision_ref.centroid's formula (the device's for a box) in ``ft``."""
    b = np.asarray(b).astype(ft)
    u, v, w = b[1] - b[0], b[2] - b[0], b[3] - b[0]
    a1, a2 = u[0] * v[1] - v[0] * u[1], v[0] * w[1] - w[0] * v[1]
    a = a1 + a2
    if a == 0.0:
        return b[0] + ((u + v) + w) / ft(4.0)
    return b[0] + (a1 * (u + v) + a2 * (v + w)) / (ft(3.0) * a)


def fan_centroid(ring):
    """Independent of ring_centroid: the area-weighted mean of the triangle fan's centroids about the vertex mean."""
    v = np.asarray(ring, dtype=np.float64)
    o = v.mean(0)
    a, b = v - o, np.roll(v, -1, axis=0) - o
    w = 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
    return o + ((a + b) / 3.0 * w[:, None]).sum(0) / w.sum()


# ---- the distance

def ego_quad(state, ap, ft=np.float64):
    """(4, 2): front-left, rear-left, rear-right, front-right of the pose (x, y, h): pdm_area_ref.coords' formulas."""
    x, y, h = (ft(v) for v in state[:3])
    c, s = np.cos(h), np.sin(h)
    half_pi = ft(np.pi / 2.0)
    cq, sq = np.cos(h + half_pi), np.sin(h + half_pi)
    cx, cy = x + ft(ap["rear_axle_to_center"]) * c, y + ft(ap["rear_axle_to_center"]) * s
    hl, hw = ft(ap["half_length"]), ft(ap["half_width"])
    out = [(cx + ((lat * cq) + (lon * c)), cy + ((lat * sq) + (lon * s)))
           for lon, lat in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw))]
    return np.array(out, dtype=ft)


def rings_intersect(quad, ring):
    """Closed intersection of the convex quad with a simple ring (float64)."""
    quad, ring = np.asarray(quad, dtype=np.float64), np.asarray(ring, dtype=np.float64)
    o = quad[0]
    q, g = quad - o, ring - o
    if len(g) == 4:
        return bool(R.quads_touch(q, g))
    edges = np.stack([g, np.roll(g, -1, axis=0)], axis=1)
    return bool(R.segment_touches(edges, q[None]).any()) or bool(A.contains([g], 0.0, 0.0))


def distance(quad, ring, ft=np.float64):
    """ego_polygon.distance(object): 0 where they intersect, else the least point-to-segment distance between the two
    boundaries, on coordinates relative to the quad's first corner."""
    if rings_intersect(quad, ring):
        return ft(0.0)
    o = np.asarray(quad).astype(ft)[0]
    q, g = np.asarray(quad).astype(ft) - o, np.asarray(ring).astype(ft) - o
    qn, gn = np.roll(q, -1, axis=0), np.roll(g, -1, axis=0)
    best = ft(np.inf)
    for p in q:
        best = min(best, _point_segment(p[0], p[1], g[:, 0], g[:, 1], gn[:, 0], gn[:, 1]).min())
    for p in g:
        best = min(best, _point_segment(p[0], p[1], q[:, 0], q[:, 1], qn[:, 0], qn[:, 1]).min())
    return np.sqrt(best)


def sampled_distance(quad, ring, per_metre=400):
    """Independent of distance(): brute-force samples of both boundaries (0 is never returned: intersecting pairs are
    the other predicate's business). An upper bound that is at most 1 / per_metre above the distance."""
    def rim(v):
        out = []
        for a, b in zip(v, np.roll(v, -1, axis=0)):
            m = max(2, int(np.hypot(*(b - a)) * per_metre) + 2)
            out.append(a + np.linspace(0.0, 1.0, m)[:, None] * (b - a))
        return np.concatenate(out)
    o = np.asarray(quad, dtype=np.float64)[0]
    a, b = rim(np.asarray(quad, dtype=np.float64) - o), rim(np.asarray(ring, dtype=np.float64) - o)
    best = np.inf
    for at in range(0, len(a), 256):
        best = min(best, float(np.hypot(a[at:at + 256, None, 0] - b[None, :, 0],
                                        a[at:at + 256, None, 1] - b[None, :, 1]).min()))
    return best


# ---- the restatement

def propagate(x, v, lead, target, p, ft=np.float64):
    """BatchIDMPolicy.propagate for one proposal: (x, v) and the leader row (progress, velocity, rear length)."""
    min_gap, headway = ft(p["min_gap_to_lead_agent"]), ft(p["headway_time"])
    accel, decel, dt = ft(p["accel_max"]), ft(p["decel_max"]), ft(p["dt"])
    x_lead, v_lead, l_r = lead
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s_star = min_gap + v * headway + (v * (v - v_lead)) / (2 * np.sqrt(accel * decel))
        s_alpha = np.maximum(x_lead - x - l_r, min_gap)
        v_dot = accel * (1 - (v / ft(target)) ** p["acceleration_exponent"] - (s_star / s_alpha) ** 2)
        clipped = np.clip(v_dot, -decel, accel)
        return x + dt * v, v + dt * clipped, v_dot


def scene_objects(tracks, rings, collided=()):
    """The packed order: the tracks that are no red light and were not hit before, then the rings."""
    return [tr for tr in tracks if R.RED_LIGHT not in tr["token"] and tr["token"] not in collided], list(rings)


def generate(paths, tracks, rings, ego_state, targets, p=None, ap=None, ft=np.float64, collided=()):
    """One scene. paths: path_of() dicts; tracks: pdm_collision_ref.track dicts (``speed`` None for a non-agent);
    rings: (n, 2) stop polygons; ego_state (11); targets (L). Returns dict(proposals (P L, 41, 3), idm (P L, 41, 2),
    lead (P L, 41, 3), lead_index (P L, 41), fallback (P), and the margins: corridor (bool: every membership steady),
    ahead (least |centroid progress - ego progress|), argmin (least gap between the two smallest distances), clip (least
    distance of an acceleration to a clip bound), clipped (how many accelerations were clipped))."""
    p, ap = p or IDM_DEFAULTS, ap or A.DEFAULTS
    tracks, rings = scene_objects(tracks, rings, collided)
    num_l, num_k = len(targets), len(tracks)
    n = len(paths) * num_l
    out = dict(proposals=np.zeros((n, T, 3), dtype=ft), idm=np.zeros((n, T, 2), dtype=ft),
               lead=np.zeros((n, T, 3), dtype=ft), lead_index=np.full((n, T), FREE, dtype=np.int32),
               fallback=np.zeros(len(paths), dtype=bool), corridor=True, ahead=np.inf, argmin=np.inf, clip=np.inf,
               clipped=0, tested=0)
    r = ap["half_width"]
    rate = p["leading_agent_update_rate"]
    max_target = float(np.max(targets))
    for pi, path in enumerate(paths):
        rows = range(pi * num_l, (pi + 1) * num_l)
        line = path["xyh"][:, :2]
        ego_progress = project(line, ego_state[0], ego_state[1], ft)
        points, out["fallback"][pi] = corridor_points(path, float(ego_progress), max_target, p)
        for n_ in rows:
            out["idm"][n_, 0] = ego_progress, ft(ego_state[R.VX])
            out["proposals"][n_, 0] = interpolate(path, [ego_progress], ft)[0]
        met_static = []
        for ring in rings:
            met, steady = meets_corridor(ring, points, r)
            out["corridor"] &= steady
            out["tested"] += 1
            met_static.append((met, project(line, *ring_centroid(ring, ft), ft) if met else None))
        for t in range(1, T):
            if t % rate:
                for n_ in rows:
                    out["lead"][n_, t], out["lead_index"][n_, t] = out["lead"][n_, t - 1], out["lead_index"][n_, t - 1]
            else:
                ahead = []                                         # (packed index, ring, progress of the centroid)
                for j, tr in enumerate(tracks):
                    if not tr["valid"][t]:
                        continue
                    met, steady = meets_corridor(tr["boxes"][t], points, r)
                    out["corridor"] &= steady
                    out["tested"] += 1
                    if met:
                        c = quad_centroid(tr["boxes"][t], ft)
                        ahead.append((j, tr["boxes"][t], project(line, c[0], c[1], ft)))
                ahead += [(num_k + i, ring, pr) for i, (ring, (met, pr)) in enumerate(zip(rings, met_static)) if met]
                carry = np.zeros(3, dtype=ft)                      # the reference's one scratch row, never cleared
                for n_ in rows:
                    x_prev = out["idm"][n_, t - 1, 0]
                    for _, _, pr in ahead:
                        out["ahead"] = min(out["ahead"], abs(float(pr - x_prev)))
                    front = [(j, ring) for j, ring, pr in ahead if pr > x_prev]
                    if front:
                        quad = ego_quad(out["proposals"][n_, t - 1], ap, ft)
                        dist = [distance(quad, ring, ft) for _, ring in front]
                        k = int(np.argmin(dist))
                        if len(dist) > 1:
                            two = np.sort(np.asarray(dist, dtype=np.float64))[:2]
                            out["argmin"] = min(out["argmin"], float(two[1] - two[0]))
                        carry[0] = x_prev + dist[k]
                        j = front[k][0]
                        if j < num_k:
                            h_ego = out["proposals"][n_, t - 1, 2]
                            rel = ft(tracks[j]["heading"]) - h_ego
                            rel = np.arctan2(np.sin(rel), np.cos(rel))
                            carry[1] = np.cos(rel) * ft(tracks[j]["speed"] or 0.0)
                        out["lead_index"][n_, t] = j
                    else:
                        carry[0] = ft(path["progress"][-1])
                        carry[2] = ft(ap["half_length"])           # vehicle length / 2
                    out["lead"][n_, t] = carry
            for li, n_ in enumerate(rows):
                x, v, v_dot = propagate(out["idm"][n_, t - 1, 0], out["idm"][n_, t - 1, 1], out["lead"][n_, t],
                                        targets[li], p, ft)
                out["idm"][n_, t] = x, v
                lo, hi = -p["decel_max"], p["accel_max"]
                if np.isfinite(v_dot):
                    out["clipped"] += int(v_dot < lo or v_dot > hi)
                    out["clip"] = min(out["clip"], abs(float(v_dot) - lo), abs(float(v_dot) - hi))
            out["proposals"][list(rows), t] = interpolate(path, out["idm"][list(rows), t, 0], ft)
    return out


def generate_scenes(scenes, p=None, ap=None, ft=np.float64):
    """A list of scene dicts (paths, tracks, rings, ego, targets, collided) -> the results stacked scene-major."""
    parts = [generate(s["paths"], s["tracks"], s["rings"], s["ego"], s["targets"], p, ap, ft, s.get("collided", ()))
             for s in scenes]
    out = {k: np.concatenate([q[k] for q in parts]) for k in ("proposals", "idm", "lead", "lead_index")}
    out["corridor"] = all(q["corridor"] for q in parts)
    for k in ("ahead", "argmin", "clip"):
        out[k] = min(q[k] for q in parts)
    return out


# ---- the bars (derived in test_proposals.py's docstring)

KEYS = ("proposals", "idm", "lead")


def floors(scenes, ap=None):
    """The derived floor of every continuous output, for a list of scenes."""
    ap = ap or A.DEFAULTS
    big = max(max(float(np.abs(q["xyh"][:, :2]).max()) for s in scenes for q in s["paths"]),
              max(float(np.abs(np.asarray(s["ego"][:2])).max()) for s in scenes))
    length = max(float(q["progress"][-1]) for s in scenes for q in s["paths"])
    verts = max(len(q["progress"]) for s in scenes for q in s["paths"])
    eps = 2.0 ** -52
    # projection: two differences at the coordinate's magnitude, the parameter's products, one rounding per summed
    # segment; the distance: corners (two roundings at the magnitude, sin / cos on the lever arms) and the differences
    progress = 4.0 * np.spacing(big) + 8.0 * eps * length + verts * np.spacing(length) + 16.0 * eps * ap["half_length"] * 2
    # interpolation: slope * dx + y_lo at the coordinate's magnitude (three roundings) plus the progress error carried
    # through a slope of at most 1; heading: sin, cos, arctan2 at 1 ulp each of pi plus the progress error over the
    # shortest segment (not known here: the longdouble term carries it)
    return dict(idm=progress, lead=progress, proposals=progress + 3.0 * np.spacing(big) + 8.0 * eps * np.pi)


def bars(scenes, ref64=None, p=None, ap=None):
    """max(floor, 16 x |float64 - longdouble| of the restatement) per output; also the measured longdouble gaps."""
    ref64 = ref64 or generate_scenes(scenes, p, ap)
    wide = generate_scenes(scenes, p, ap, ft=np.longdouble)
    assert np.array_equal(wide["lead_index"], ref64["lead_index"])
    fl = floors(scenes, ap)
    gaps = {k: float(np.abs(ref64[k].astype(np.longdouble) - wide[k]).max()) for k in KEYS}
    return {k: max(fl[k], 16.0 * gaps[k]) for k in KEYS}, gaps


def compare(tag, got, ref, bar):
    """Prints the largest differences, then asserts: lead_index equal, the continuous outputs within their bars."""
    worst = {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k].astype(np.float64)).max()) for k in KEYS}
    same = np.array_equal(np.asarray(got["lead_index"]), ref["lead_index"])
    print(f"proposals {tag}: lead_index equal {same}; " + ", ".join(f"{k} {worst[k]:.3e} (bar {bar[k]:.3e})" for k in KEYS))
    assert same, tag
    for k in KEYS:
        assert worst[k] <= bar[k], (tag, k, worst[k], bar[k])
    return worst


# ---- seeded inputs

def heading_of(xy):
    d = np.diff(xy, axis=0)
    h = np.arctan2(d[:, 1], d[:, 0])
    return np.append(h, h[-1])


def seeded_scene(seed, pose=(0.0, 0.0, 0.0), speed_limit=12.0, offsets=(-1.0, 1.0), t_obs=R.T_OBS, speed=None,
                 light_at=None):
    """The seeded centerline of pdm_collision_ref around ``pose`` with two lateral offsets, the five default policies
    at ``speed_limit``, seeded tracks along it (a slower vehicle ahead in the corridor, a vehicle that cuts in late, a
    stationary object beside the corridor, a pedestrian crossing it, a token hit before), and one red-light ring
    across the path ahead."""
    rng = np.random.default_rng(seed)
    xy = R.seeded_centerline(seed, pose)
    base = np.concatenate([xy, heading_of(xy)[:, None]], axis=1)
    raw = [base] + [parallel_path(base, o) for o in offsets]
    paths = [path_of(q) for q in raw]
    ego = np.zeros(11)
    at = float(rng.uniform(14.0, 18.0))                           # arc length of the start along the centerline
    ego[:3] = interpolate(paths[0], [at])[0]
    ego[1] += float(rng.uniform(-0.2, 0.2))
    ego[R.VX] = float(rng.uniform(3.0, 9.0)) if speed is None else speed
    times = np.arange(t_obs) * 0.1

    def along(s, lat=0.0):
        q = interpolate(paths[0], np.atleast_1d(s))
        return (q[:, 0] - lat * np.sin(q[:, 2]), q[:, 1] + lat * np.cos(q[:, 2]), q[:, 2])

    tracks = []
    s = at + rng.uniform(22.0, 30.0) + rng.uniform(1.0, 3.0) * times
    x, y, h = along(s, rng.uniform(-0.3, 0.3))
    tracks.append(R.track(f"lead_{seed}", x, y, float(h[0]), 4.6, 1.9, "VEHICLE", float((s[1] - s[0]) * 10)))
    cut = int(rng.integers(9, 20))
    s2 = at + rng.uniform(10.0, 14.0) + 2.0 * times
    x, y, h = along(s2, np.where(np.arange(t_obs) < cut, 4.5, rng.uniform(-0.2, 0.2)))
    tracks.append(R.track(f"cut_{seed}", x, y, float(h[0]), 4.4, 1.8, "VEHICLE", 2.0))
    x, y, h = along(at + rng.uniform(15.0, 25.0), rng.choice([-1.0, 1.0]) * rng.uniform(4.0, 5.0))
    tracks.append(R.track(f"cone_{seed}", x[0], y[0], float(h[0]), 0.5, 0.5, "TRAFFIC_CONE", 0.0))
    s3 = at + rng.uniform(30.0, 40.0)
    x, y, h = along(s3, -6.0 + 1.3 * times)
    valid = np.arange(t_obs) >= 7
    tracks.append(R.track(f"ped_{seed}", x, y, float(h[0]) + np.pi / 2, 0.7, 0.7, "PEDESTRIAN", 1.3, valid))
    x, y, h = along(at + 6.0, 0.3)
    tracks.append(R.track(f"hit_before_{seed}", x[0], y[0], float(h[0]), 4.0, 1.8, "VEHICLE", 0.0))
    s4 = at + (rng.uniform(35.0, 60.0) if light_at is None else light_at)   # light_at: nearer than the vehicle ahead
    x, y, h = along(s4)
    ring = R.box(x[0], y[0], h[0], rng.uniform(3.0, 5.0), 8.0)
    return dict(paths=paths, raw_paths=raw, tracks=tracks, rings=[ring], ego=ego,
                targets=np.array(SPEED_LIMIT_FRACTIONS) * speed_limit, collided=[f"hit_before_{seed}"])


GLOBAL_POSE = (664431.37, 3997675.12, 2.3)


def golden_scenes(seed):
    """The scenes of tests/golden/pdm_proposals_s{seed}.npz, rebuilt from the seed: at the origin and at 6.6e5 / 4.0e6 m,
    two speed limits, a red light nearer than every vehicle, and a crawl whose corridor holds no vertex (the substring
    fallback)."""
    return dict(origin=seeded_scene(seed), far=seeded_scene(seed + 1, GLOBAL_POSE, speed_limit=8.0),
                light=seeded_scene(seed + 2, GLOBAL_POSE, speed_limit=12.0, light_at=17.0),
                crawl=seeded_scene(seed + 3, speed_limit=0.5, speed=0.4))


def lead_items(scene):
    """The list form pack_lead_objects takes for one scene: (tracks with a speed, rings)."""
    items = [(tr["token"], np.where(np.asarray(tr["valid"])[:, None, None], tr["boxes"], np.nan), tr["heading"],
              tr["is_agent"], tr["stopped"], tr["speed"] or 0.0) for tr in scene["tracks"]]
    return items, scene["rings"]


# ---- the hand-built cases: a straight path along +x, the vehicle 4.049 m ahead of / 1.127 m behind the rear axle and
# 1.1485 m beside it; every answer is known by construction

def straight_path(xs, y=0.0):
    xs = np.asarray(xs, dtype=np.float64)
    return path_of(np.stack([xs, np.full(xs.shape, y), np.zeros(xs.shape)], axis=-1))


def still(token, x, y, length=4.6, width=1.9, kind="VEHICLE", speed=0.0, valid=None, h=0.0):
    return R.track(token, x, y, h, length, width, kind, speed, valid)


def hand_cases():
    """[(name, scene, expected)]: ``expected`` maps (proposal, time index) -> lead_index, or names a property the
    tests check (see check_hand_case)."""
    xs = np.arange(0.0, 201.0, 10.0)
    path = straight_path(xs)
    times = np.arange(R.T_OBS)
    cases = []

    def case(name, expected, paths=(path,), tracks=(), rings=(), x=20.0, v=5.0, targets=(10.0,), y=0.0):
        ego = np.zeros(11)
        ego[0], ego[1], ego[R.VX] = x, y, v
        cases.append((name, dict(paths=list(paths), tracks=list(tracks), rings=list(rings), ego=ego,
                                 targets=np.asarray(targets, dtype=np.float64), collided=[]), expected))

    case("free_driving", dict(index={(0, 2): FREE, (0, 40): FREE},
                              lead_row=(2, (200.0, 0.0, A.DEFAULTS["half_length"]))))
    # the start projects before the first vertex: progress 0, state 0 is interpolate(1e-5)
    case("ego_before_the_first_vertex", dict(idm0=0.0, state0=(1e-5, 0.0, 0.0)), x=-3.0)
    case("ego_beyond_the_last_vertex", dict(idm0=200.0, state0=(200.0, 0.0, 0.0)), x=207.0)
    case("two_vertex_path", dict(idm0=20.0, index={(0, 2): 0}),
         paths=[straight_path([0.0, 300.0])], tracks=[still("a", 50.0, 0.0)])
    dup = straight_path([0.0, 10.0, 20.0, 30.0, 30.0, 40.0, 50.0, 60.0, 200.0])
    case("duplicated_vertex", dict(idm0=20.0, index={(0, 2): FREE}), paths=[dup])
    # behind the ego but inside the corridor: the ego stands on the vertex x = 20, the square cap reaches back to
    # 20 - 1.1485, the object spans 19 .. 20 with its centroid at 19.5
    case("object_just_behind_the_ego", dict(index={(0, 2): FREE, (0, 40): FREE}, in_corridor=(0, 2)),
         tracks=[still("behind", 19.5, 0.0, length=1.0)])
    case("object_ahead_but_beside_the_corridor", dict(index={(0, 2): FREE, (0, 40): FREE}),
         tracks=[still("beside", 45.0, 1.1485 + 0.95 + 0.1)])
    case("object_appears_at_7_seen_at_8", dict(index={(0, 6): FREE, (0, 7): FREE, (0, 8): 0, (0, 9): 0}),
         tracks=[still("late", 60.0, 0.0, valid=times >= 7)])
    case("object_leaves_the_corridor", dict(index={(0, 10): 0, (0, 11): 0, (0, 12): FREE, (0, 40): FREE}),
         tracks=[still("leaving", 60.0, np.where(times < 12, 0.0, 9.0))])
    # overlapping the ego quad at the state of step 1 with its centroid ahead of the ego's progress: distance 0
    case("overlapping_object", dict(index={(0, 2): 0}, lead_progress_is_ego=(0, 2)),
         tracks=[still("on_top", 23.5, 0.0)])
    light = A.rect(60.0, -4.0, 64.0, 4.0)
    case("red_light_nearer_than_vehicle", dict(index={(0, 2): 1, (0, 40): 1}, lead_velocity=((0, 2), 0.0)),
         tracks=[still("far", 90.0, 0.0, speed=3.0)], rings=[light])
    case("vehicle_nearer_than_red_light", dict(index={(0, 2): 0}, lead_velocity=((0, 2), 3.0), rear_length=((0, 2), 0.0)),
         tracks=[still("near", 45.0, 0.0, speed=3.0)], rings=[light])
    # the vertex-only quirk: the ego at 23 m, the corridor (23 .. 43) keeps the vertices 30 and 40 and starts at 30 - r:
    # an object that spans 27.5 .. 28.5, between the ego's bumper and the cap, is not in it
    case("corridor_starts_at_the_first_vertex_ahead", dict(index={(0, 2): FREE, (0, 40): FREE}, fallback=False),
         tracks=[still("between", 28.0, 0.0, length=1.0)], x=23.0, v=2.0, targets=(4.0,))
    # the substring fallback: a target so low that the corridor (23 .. 25.5) holds no vertex: the two interpolated ends,
    # lengthened by r to 26.65; the object spans 26 .. 28 (and overlaps the bumper at 27.049: distance 0)
    case("substring_fallback", dict(index={(0, 2): 0}, fallback=True, lead_progress_is_ego=(0, 2)),
         tracks=[still("close", 27.0, 0.0, length=2.0)], x=23.0, v=0.5, targets=(0.5,))
    case("target_below_the_start_speed", dict(decelerates=True, index={(0, 40): FREE}), v=12.0, targets=(2.0,))
    # two policies on one path and an object that appears at index 16 at x = 34.5, behind the fast proposal (36.3 m by
    # then) and ahead of the slow one (which brakes from 9 m/s and never gets past 33.5): at the even indices from 16 on
    # the fast one drives free and the slow one, AFTER it in the same scratch row, keeps its rear length 2.588
    case("carried_scratch_row", dict(carry=True), tracks=[still("late", 34.5, 0.0, length=1.0, valid=times >= 16)],
         v=9.0, targets=(14.0, 0.6))
    case("one_policy_one_path", dict(shape=(1, 41, 3)))
    return cases


def check_hand_case(name, out, expected, scene, ap=None):
    ap = ap or A.DEFAULTS
    for (n, t), want in expected.get("index", {}).items():
        assert out["lead_index"][n, t] == want, (name, n, t, out["lead_index"][n, t], want)
    if "idm0" in expected:
        assert abs(out["idm"][0, 0, 0] - expected["idm0"]) <= 1e-12, (name, out["idm"][0, 0])
    if "state0" in expected:
        assert np.abs(out["proposals"][0, 0] - np.asarray(expected["state0"])).max() <= 1e-12, (name, out["proposals"][0, 0])
    if "lead_row" in expected:
        t, row = expected["lead_row"]
        assert np.array_equal(out["lead"][0, t], np.asarray(row)), (name, out["lead"][0, t])
    if "lead_progress_is_ego" in expected:
        n, t = expected["lead_progress_is_ego"]
        assert out["lead"][n, t, 0] == out["idm"][n, t - 1, 0], name
    if "lead_velocity" in expected:
        (n, t), want = expected["lead_velocity"]
        assert abs(out["lead"][n, t, 1] - want) <= 1e-12, (name, out["lead"][n, t])
    if "rear_length" in expected:
        (n, t), want = expected["rear_length"]
        assert out["lead"][n, t, 2] == want, (name, out["lead"][n, t])
    if "in_corridor" in expected:
        t = expected["in_corridor"][1]
        tr = scene["tracks"][0]
        points, _ = corridor_points(scene["paths"][0], float(out["idm"][0, 0, 0]), float(np.max(scene["targets"])), IDM_DEFAULTS)
        assert meets_corridor(tr["boxes"][t], points, ap["half_width"]) == (True, True), name
    if "fallback" in expected and "fallback" in out:
        assert bool(out["fallback"][0]) == expected["fallback"], name
    if expected.get("decelerates"):
        dv = np.diff(out["idm"][0, :, 1])
        assert np.abs(dv[1:8] + 0.3).max() <= 1e-12, (name, dv[:8])       # clipped at -decel_max * dt
    if expected.get("carry"):
        li = out["lead_index"]
        mixed = [t for t in range(2, T, 2) if li[0, t] == FREE and li[1, t] == 0]
        assert mixed, (name, li[:, ::2])
        for t in mixed:
            assert out["lead"][1, t, 2] == ap["half_length"] and out["lead"][0, t, 2] == ap["half_length"], name
    if "shape" in expected:
        assert out["proposals"].shape == expected["shape"], name
    # rows 0 and 1 of the leader are the zero rows the reference starts with
    assert not out["lead"][:, :2].any() and (out["lead_index"][:, :2] == FREE).all(), name
