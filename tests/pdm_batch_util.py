"""CPU-only input builders for the PDM scoring chain at batch structure (tests/test_pdm_batch.py holds them to their
conditions, tests/test_pdm_batch_gpu.py runs them on the device): group sizes past one workgroup of dd_pdm_aggregate,
dd_progress past one block with ragged centerlines, more polygons than one listing pass of dd_ego_areas, ragged track
counts across the chunk of 64 of dd_collisions, many scenes, T_obs past one stride of the track boxes.

Truth is what the suite already trusts: the goldens (pdm_score_s5.npz, pdm_area_s11.npz, the simulator sets) and the
numpy restatements pdm_collision_ref (R) and pdm_area_ref (A), which the CPU suite holds to those goldens. Every
builder asserts, on the CPU and on the reference side, that its case would notice the fault it is built for; nothing
here needs a device.
"""
import numpy as np

import pdm_area_ref as A
import pdm_collision_ref as R
from test_collisions import SIM_SETS

MARGIN = 1e-7           # gaps, speeds, axle points, point-to-edge distances of the cases built here
ANGLE_MARGIN = 1e-9
KEYS = ("no_collision", "drivable_area", "driving_direction", "progress", "ttc", "collision_time_idx", "ttc_time_idx",
        "raw_progress", "score")
WAVE, BLOCK = 64, 256   # a wavefront; the workgroup of aggregate_kernel, progress_kernel and the polygon listing


def product(g, name):
    """raw * no_collision * drivable_area of a golden set: what the group's maximum is taken over."""
    return g[f"raw_progress_{name}"] * g[f"no_collision_{name}"] * g[f"drivable_area_{name}"]


# ---- 1. group sizes past one workgroup

def group_rows(g, name, per_group, seed, second_in):
    """rows (per_group): candidate i holds golden row rows[i]. The row with the largest product sits at the last index
    alone, the row with the second largest at one index inside ``second_in`` = (lo, hi) alone, every other index draws
    from the remaining rows by a seeded permutation (all of them appear: per_group > 96)."""
    p = product(g, name)
    assert np.isfinite(p).all()
    order = np.argsort(p, kind="stable")
    top, second = int(order[-1]), int(order[-2])
    rest = order[:-2][np.random.default_rng(seed).permutation(len(p) - 2)]
    lo, hi = second_in
    assert 0 <= lo < hi <= per_group - 1 and per_group - 2 >= len(rest)
    at = lo + (hi - lo) // 3
    rows = np.empty(per_group, dtype=np.int64)
    free = [i for i in range(per_group - 1) if i != at]
    rows[free] = rest[np.arange(len(free)) % len(rest)]
    rows[at], rows[-1] = second, top
    assert set(rows.tolist()) == set(range(len(p)))
    return rows


def term_of(p, multi, pmax, threshold=5.0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(pmax > threshold, p / pmax, np.where(multi == 0.0, 0.0, 1.0))


def group_case(g, names, per_group, seed, second_in):
    """(states (G, per_group, 41, 11), rows (G, per_group), scenes, figures): one scene per name. ``figures`` says how
    the construction bites: per scene the share of candidates whose progress term moves by more than the term's bar
    when the maximum is taken over the indices below ``second_in[1]`` (cut_hi: without the last index) or below
    ``second_in[0]`` (cut_lo: without the second largest too); over all candidates and over those with a non-zero
    product (a zero product gives a term of 0 under every maximum)."""
    rows = np.stack([group_rows(g, n, per_group, seed + k, second_in) for k, n in enumerate(names)])
    states = np.stack([g[f"states_{n}"][rows[k]] for k, n in enumerate(names)])
    figures = []
    for k, n in enumerate(names):
        p = product(g, n)[rows[k]]
        multi = (g[f"no_collision_{n}"] * g[f"drivable_area_{n}"])[rows[k]]
        line = g[f"scene_{n}"][6]
        bar = R.score_bars(dict(pmax=np.full(p.shape, p.max())), R.raw_progress_bar(g[f"states_{n}"], line))[0]
        true = term_of(p, multi, p.max())
        fig = dict(pmax=float(p.max()))
        for tag, upto in (("cut_hi", second_in[1]), ("cut_lo", second_in[0])):
            moved = np.abs(term_of(p, multi, p[:upto].max()) - true) > bar
            fig[tag] = float(moved.mean())
            fig[tag + "_of_nonzero"] = float(moved[p != 0.0].mean()) if (p != 0.0).any() else 0.0
        figures.append(fig)
    pmax = [f["pmax"] for f in figures]
    assert len(set(pmax)) == len(pmax), pmax          # the scenes' maxima are pairwise distinct
    return states, rows, [g[f"scene_{n}"] for n in names], figures


# ---- 2. dd_pdm_aggregate on its own

AGG_GROUPS = (1, 63, 64, 65, 192, 193, 256, 257, 513)
AGG_SCENES = 6
# The six reference values by role, and the scene each goes to. Only "above" and "between" can move a term of an
# ordinary scene (below every product, 0, 5.0 and NaN all leave p / p = 1 above the threshold and the multiplier's
# branch below it), and the scene whose multipliers are all 0 never moves: so the two sit at scenes 1 and 3, where each
# neighbour's value in place of a scene's own moves more than half the terms of four scenes in both directions
# (aggregate_conditions asserts it), and "between" sits high among the products.
AGG_REFERENCE = dict(below=-1.0, above=100.0, between=50.0, threshold=5.0, zero=0.0, nan=float("nan"))
AGG_REFERENCE_ORDER = ("zero", "above", "nan", "between", "threshold", "below")


def third_role_index(per_group):
    """An index held by wavefront 2 or 3 of aggregate_kernel's workgroup (i % 256 >= 128), the middle one of those
    the group has; None below 129 candidates."""
    held = [i for i in range(per_group) if i % BLOCK >= 2 * WAVE]
    return held[len(held) // 2] if held else None


def aggregate_case(per_group, seed):
    """Synthetic sub-scores of six scenes drawn from the values the stages can produce (the comfort bytes are 0 / 1:
    include/ddmi.h takes them "as dd_comfort writes" them). Roles: 0 the maximum at index 0; 1 at the last index; 2
    in wavefront 2 or 3 only (where per_group reaches them); 3 every product <= 5.0 with one exactly 5.0; 4 a NaN
    raw progress at the last index; 5 every multiplier 0."""
    rng = np.random.default_rng(seed)
    shape = (AGG_SCENES, per_group)
    c = dict(no_collision=rng.choice([0.0, 0.5, 1.0], shape, p=[0.1, 0.2, 0.7]),
             drivable_area=rng.choice([0.0, 1.0], shape, p=[0.1, 0.9]),
             driving_direction=rng.choice([0.0, 0.5, 1.0], shape), ttc=rng.choice([0.0, 1.0], shape),
             comfort=(rng.uniform(size=shape + (6,)) < 0.9).astype(np.uint8),
             raw_progress=rng.uniform(0.0, 60.0, shape))

    def put_max(scene, at):
        c["no_collision"][scene, at] = c["drivable_area"][scene, at] = 1.0
        c["raw_progress"][scene, at] = 60.0 + rng.uniform(0.5, 1.0)

    put_max(0, 0)
    put_max(1, per_group - 1)
    third = third_role_index(per_group)
    if third is not None:
        put_max(2, third)
    c["raw_progress"][3] = rng.uniform(0.0, 4.9, per_group)
    at5 = per_group // 2
    c["no_collision"][3, at5] = c["drivable_area"][3, at5] = 1.0
    c["raw_progress"][3, at5] = 5.0
    c["raw_progress"][4, -1] = np.nan
    zero = rng.uniform(size=per_group) < 0.5
    c["no_collision"][5, zero] = 0.0
    c["drivable_area"][5, ~zero] = 0.0
    c["reference"] = np.array([AGG_REFERENCE[k] for k in AGG_REFERENCE_ORDER])
    return c


def aggregate_ref(c, reference=None):
    """R.aggregate per scene -> dict(score, progress, pmax) as (G, per_group) arrays."""
    parts = [R.aggregate(c["no_collision"][s], c["drivable_area"][s], c["driving_direction"][s], c["raw_progress"][s],
                         c["ttc"][s], c["comfort"][s].astype(bool).all(-1),
                         reference=None if reference is None else reference[s]) for s in range(AGG_SCENES)]
    return dict(score=np.stack([q[0] for q in parts]), progress=np.stack([q[1] for q in parts]),
                pmax=np.stack([q[2] for q in parts]))


def aggregate_conditions(c):
    """Assert that the roles are realised and that a neighbour's reference value would show. Returns the figures."""
    per_group = c["raw_progress"].shape[1]
    multi = c["no_collision"] * c["drivable_area"]
    with np.errstate(invalid="ignore"):
        p = c["raw_progress"] * multi
    assert set(np.unique(c["comfort"]).tolist()) <= {0, 1}
    assert int(np.argmax(p[0])) == 0 and int(np.argmax(p[1])) == per_group - 1 and p[0].max() > 5.0 and p[1].max() > 5.0
    third = third_role_index(per_group)
    if third is not None:
        assert int(np.argmax(p[2])) == third and (third % BLOCK) // WAVE >= 2
        assert p[2, :2 * WAVE].max() != p[2].max()     # wavefronts 0 and 1 of the first step do not hold it
    assert p[3].max() == 5.0 and (p[3] == 5.0).sum() == 1
    assert np.isnan(p[4, -1]) and np.isfinite(p[4, :-1]).all()
    assert (multi[5] == 0.0).all()
    if per_group > 1:
        assert (multi[3] == 0.0).any() and (multi[3] != 0.0).any() and (c["raw_progress"][5] > 5.0).any()
    ref = c["reference"]
    assert len(set(np.nan_to_num(ref, nan=-7.0).tolist())) == AGG_SCENES
    finite = p[np.isfinite(p)]
    assert AGG_REFERENCE["below"] < finite.min() and AGG_REFERENCE["above"] > finite.max()
    assert finite.min() < AGG_REFERENCE["between"] < finite.max() or per_group == 1
    own = aggregate_ref(c, ref)["progress"]
    moved = {}
    for shift in (1, -1):
        other = aggregate_ref(c, np.roll(ref, -shift))["progress"]       # scene s reads reference[s + shift]
        share = (other != own).mean(axis=1)
        moved[shift] = int((share > 0.5).sum())
        # one candidate per scene: the NaN scene and the all-zero scene cannot move, and the roles leave three
        assert moved[shift] >= (4 if per_group > 1 else 3), (shift, share)
    return dict(moved=moved, group_vs_pair=float((aggregate_ref(c)["progress"] != own).mean()))


# ---- 3. dd_progress on its own

PROGRESS_SCENES, PROGRESS_GROUP = 7, 75
PROGRESS_AXLE = 1.5       # rear_axle_to_center of the call: with heading 0 the centers of dyadic states are exact
TIE_SCENE, ZERO_SCENE, GLOBAL_SCENE = 5, 4, 6
GLOBAL_POSE = (664431.37, 3997675.12, 2.3)


def progress_lines(seed):
    """Seven ragged centerlines: 2 vertices; 3 vertices; 24 seeded; 300; a doubled first and a doubled inner vertex
    (zero-length segments) on a dyadic grid; a hairpin on a dyadic grid; 24 seeded in the global frame."""
    rng = np.random.default_rng(seed)
    long_x = np.cumsum(rng.uniform(0.15, 0.35, 300))
    long = np.stack([long_x, 3.0 * np.sin(long_x / 9.0)], -1)
    zero = np.array([[0.0, 0.0], [0.0, 0.0], [4.0, 0.0], [9.0, 1.0], [9.0, 1.0], [14.0, 3.0], [20.0, 3.0]])
    hairpin = np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 2.0], [0.0, 2.0]])
    return [A.to_frame(np.array([[-5.0, 0.0], [40.0, 3.0]]), (10.0, 50.0, 0.4)),
            A.to_frame(np.array([[0.0, 0.0], [12.0, 1.0], [30.0, -2.0]]), (-60.0, 20.0, -1.1)),
            R.seeded_centerline(seed, (30.0, -70.0, 2.0)),
            A.to_frame(long, (-150.0, -120.0, 0.9)),
            zero + np.array([128.0, 64.0]),
            hairpin + np.array([-96.0, 160.0]),
            R.seeded_centerline(seed + 1, GLOBAL_POSE)]


def along(line, s, lateral):
    """The point at arc length ``s`` of the polyline (extended past both ends), ``lateral`` metres to its left."""
    seg = np.diff(line, axis=0)
    length = np.linalg.norm(seg, axis=1)
    keep = length > 0
    start, seg, length = line[:-1][keep], seg[keep], length[keep]
    cum = np.concatenate([[0.0], np.cumsum(length)])
    i = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, len(seg) - 1)
    u = seg[i] / length[i, None]
    return start[i] + (s - cum[i])[:, None] * u + lateral[:, None] * np.stack([-u[:, 1], u[:, 0]], -1)


def segments(line, x, y):
    """Per segment the squared distance and the arc length of the nearest point, in R.project's own arithmetic."""
    d2, arc, passed = [], [], 0.0
    for a, b in zip(line[:-1], line[1:]):
        dx, dy = b[0] - a[0], b[1] - a[1]
        len2 = dx * dx + dy * dy
        length = np.sqrt(len2)
        wx, wy = x - a[0], y - a[1]
        s = (wx * dx + wy * dy) / len2 if len2 > 0.0 else 0.0
        s = min(max(s, 0.0), 1.0)
        ex, ey = wx - s * dx, wy - s * dy
        d2.append(ex * ex + ey * ey), arc.append(passed + s * length)
        passed += length
    return np.array(d2), np.array(arc)


def is_tie(line, x, y, near=1e-3, apart=1e-2):
    """Another stretch of the line (its arc length ``apart`` away) comes within ``near`` metres of the nearest one."""
    d2, arc = segments(line, x, y)
    b = int(np.argmin(d2))
    return bool(((np.abs(arc - arc[b]) > apart) & (np.sqrt(d2) - np.sqrt(d2[b]) < near)).any())


def progress_case(seed):
    """dict(states (7, 75, 41, 11) with states 0 and 40 laid around each scene's line and zeros between, lines, centers
    (7, 75, 2, 2), exact (7, 75): the candidates whose result must be bit-equal, ties (7, 75))."""
    rng = np.random.default_rng(seed + 7)
    lines = progress_lines(seed)
    n, r = PROGRESS_GROUP, PROGRESS_AXLE
    states = np.zeros((PROGRESS_SCENES, n, A.T, 11))
    for g, line in enumerate(lines):
        total = float(np.linalg.norm(np.diff(line, axis=0), axis=1).sum())
        s0 = rng.uniform(-0.1 * total, 0.8 * total, n)
        step = np.where(rng.uniform(size=n) < 0.85, rng.uniform(3.0, 0.5 * total, n), -rng.uniform(1.0, 10.0, n))
        s1 = s0 + step
        s0[1:4], s1[1:4] = [-6.0, -3.0, 0.3 * total], [0.4 * total, total + 5.0, total + 8.0]   # before / past the ends
        centers = np.stack([along(line, s0, rng.uniform(-4.0, 4.0, n)), along(line, s1, rng.uniform(-4.0, 4.0, n))], 1)
        heading = rng.uniform(-3.1, 3.1, (n, 2))
        if g in (TIE_SCENE, ZERO_SCENE):      # dyadic centers, heading 0: the device's centers are numpy's
            centers = np.round(centers * 4.0) / 4.0
            heading[:] = 0.0
        if g == TIE_SCENE:                    # on the hairpin's middle line y = 1: equidistant from both legs
            o = lines[TIE_SCENE][0]
            k = n // 2
            centers[4:k, 0, 0] = o[0] + 0.25 * rng.integers(1, 9, k - 4)
            centers[4:k, 1, 0] = o[0] + 0.25 * rng.integers(14, 27, k - 4)
            centers[4:k, :, 1] = o[1] + 1.0
        if g == ZERO_SCENE:                   # nearest to the doubled vertices themselves
            o = lines[ZERO_SCENE]
            centers[4, 0], centers[4, 1] = o[0] + [-1.0, 0.5], o[3] + [0.25, -1.0]
            centers[5, 0], centers[5, 1] = o[0] + [-2.0, -2.0], o[4] + [0.5, -2.0]
        if g > 0:                             # the first candidate starts 0.5 m past the previous scene's line end
            prev = lines[g - 1]
            u = (prev[-1] - prev[-2]) / np.linalg.norm(prev[-1] - prev[-2])
            centers[0, 0] = prev[-1] + 0.5 * u
            if g in (TIE_SCENE, ZERO_SCENE):
                centers[0, 0] = np.round(centers[0, 0] * 4.0) / 4.0
        for e, t in enumerate((0, A.T - 1)):
            states[g, :, t, A.X] = centers[:, e, 0] - r * np.cos(heading[:, e])
            states[g, :, t, A.Y] = centers[:, e, 1] - r * np.sin(heading[:, e])
            states[g, :, t, A.HEADING] = heading[:, e]
    ap = A.params(rear_axle_to_center=r)
    centers = np.stack([A.coords(states[g], ap)[:, [0, A.T - 1], A.CENTER] for g in range(PROGRESS_SCENES)])
    ties = np.array([[is_tie(lines[g], *centers[g, i, 0]) or is_tie(lines[g], *centers[g, i, 1]) for i in range(n)]
                     for g in range(PROGRESS_SCENES)])
    exact = np.zeros((PROGRESS_SCENES, n), dtype=bool)
    exact[[TIE_SCENE, ZERO_SCENE]] = True
    return dict(states=states, lines=lines, centers=centers, ties=ties, exact=exact, area_params=ap)


def progress_conditions(c):
    """Assert the conditions of the progress case on the reference side. Returns the figures."""
    lines, states, centers, ap = c["lines"], c["states"], c["centers"], c["area_params"]
    assert [len(line) for line in lines] == [2, 3, 24, 300, 7, 4, 24]
    assert np.abs(lines[GLOBAL_SCENE][:, 0]).min() > 6.6e5 and np.abs(lines[GLOBAL_SCENE][:, 1]).min() > 3.9e6
    assert (np.linalg.norm(np.diff(lines[ZERO_SCENE], axis=0), axis=1) == 0.0).sum() == 2
    for g in (TIE_SCENE, ZERO_SCENE):         # dyadic lines and centers, exact on both sides
        assert (lines[g] * 4.0 == np.round(lines[g] * 4.0)).all()
        assert (centers[g] * 4.0 == np.round(centers[g] * 4.0)).all()
        assert (states[g, ..., A.HEADING] == 0.0).all()
    own = np.stack([R.raw_progress(states[g], lines[g], ap) for g in range(PROGRESS_SCENES)])
    # the hairpin's ties: the two legs at the same squared distance as floats, the first wins, the other would show
    tied = 0
    hair = lines[TIE_SCENE]
    for i in range(PROGRESS_GROUP):
        both = [segments(hair, *centers[TIE_SCENE, i, e]) for e in range(2)]
        if all(d2[0] == d2[2] and d2[0] < d2[1] for d2, _ in both):
            tied += 1
            assert own[TIE_SCENE, i] == both[1][1][0] - both[0][1][0] > 1.0      # the first leg's arc lengths
            assert abs((both[1][1][2] - both[0][1][2]) - own[TIE_SCENE, i]) > 1.0   # the last leg's would differ
    assert tied >= 25, tied
    # the doubled vertices: a center nearest to each
    for e, v in ((0, 0), (1, 3)):
        d2, _ = segments(lines[ZERO_SCENE], *centers[ZERO_SCENE, 4, e])
        assert d2[v] == d2.min() and d2[v + 1] == d2.min()
    # clamping: before the start and past the end of the 3-vertex line
    total = float(np.linalg.norm(np.diff(lines[1], axis=0), axis=1).sum())
    first = R.project(lines[1], centers[1, :, 0, 0], centers[1, :, 0, 1])
    last = R.project(lines[1], centers[1, :, 1, 0], centers[1, :, 1, 1])
    assert (first[1:3] == 0.0).all() and (np.abs(last[2:4] - total) < 1e-12).all()
    assert (own == 0.0).sum() >= PROGRESS_SCENES and (own > 3.0).mean() > 0.6
    wrong = {}
    for shift in (1, -1):
        moved = [np.abs(R.raw_progress(states[g], lines[(g + shift) % PROGRESS_SCENES], ap) - own[g]) > 1.0
                 for g in range(PROGRESS_SCENES)]
        wrong[shift] = [float(m.mean()) for m in moved]
        assert min(wrong[shift]) > 0.5, wrong
    # the first candidate of scene g projects onto scene g - 1's line end, nowhere near its own line
    for g in range(1, PROGRESS_SCENES):
        d2_own = segments(lines[g], *centers[g, 0, 0])[0].min()
        d2_prev = segments(lines[g - 1], *centers[g, 0, 0])[0].min()
        assert d2_prev < 0.6 ** 2 < 10.0 ** 2 < d2_own, (g, d2_prev, d2_own)
    non_tie = ~c["ties"]
    assert non_tie.mean() > 0.7 and non_tie[TIE_SCENE].sum() >= 10
    return dict(own=own, tied=tied, wrong_scene=wrong, non_tie=non_tie)


def independent_progress(c, g):
    """Raw progress of scene g's candidates from the dense sampling of the line, and the bound of its error."""
    cen = c["centers"][g]
    a, bound_a = R.independent_project(c["lines"][g], cen[:, 0, 0], cen[:, 0, 1])
    b, bound_b = R.independent_project(c["lines"][g], cen[:, 1, 0], cen[:, 1, 1])
    return np.maximum(b - a, 0.0), bound_a + bound_b


# ---- 4. more polygons than one listing pass

AREA_POLYGONS = (600, 3, 0)
AREA_GROUP = 8
AREA_ROWS = (0, 9, 18, 27, 36, 45, 54, 63)        # of the synthetic golden states, scene 0
AREA_AT = (0, 63, 64, 255, 256, 511, 512)         # list indices of the seeded map's first items; the rest come last
FILLER_LAYERS = ("LANE", "LANE_CONNECTOR", "ROADBLOCK", "DRIVABLE_AREA", "CARPARK_AREA")


def area_case(g, seed):
    """dict(states (3, 8, 41, 11), maps: scenes of 600, 3 and 0 polygons, tracks, collided, lines). Scene 0: the
    seeded map's items at list indices AREA_AT and at the end, between them fillers in a seeded order - half beyond
    300 m, half 3 m squares of mixed layers laid on points of the first workgroup's candidates."""
    rng = np.random.default_rng(seed)
    states = np.stack([g["states_synth"][list(AREA_ROWS)], g["states_moving"][[3, 17, 29, 40, 58, 71, 83, 91]],
                       g["states_moving"][[5, 11, 23, 37, 44, 62, 77, 95]]])
    items = list(g["scene_synth"][0])
    pts = A.coords(states[0, :4]).reshape(-1, 2)
    fillers = AREA_POLYGONS[0] - len(items)
    near = fillers // 2
    out = []
    for i in range(fillers):
        if i < near:
            c = pts[rng.integers(len(pts))] + rng.uniform(-1.4, 1.4, 2)
            layer = "INTERSECTION" if i < 2 else FILLER_LAYERS[int(rng.integers(len(FILLER_LAYERS)))]
            ring = A.to_frame(A.rect(-1.5, -1.5, 1.5, 1.5), (c[0], c[1], rng.uniform(-3.0, 3.0)))
            out.append(([ring], layer, bool(rng.integers(2)) and layer in A.LANE_LAYERS))
        else:
            ang, rad = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(300.0, 900.0)
            pose = (rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3.0, 3.0))
            ring = A.to_frame(A.rect(-4.0, -2.0, 4.0, 2.0), pose)
            out.append(([ring], FILLER_LAYERS[int(rng.integers(len(FILLER_LAYERS)))], bool(rng.integers(2))))
    out = [out[i] for i in rng.permutation(fillers)]
    head, tail = items[:len(AREA_AT)], items[len(AREA_AT):]
    scene0 = []
    for at, it in zip(AREA_AT, head):
        while len(scene0) < at:
            scene0.append(out.pop())
        scene0.append(it)
    scene0 += out + tail
    maps = [scene0, list(g["scene_moving"][0][:3]), []]
    tracks = [g["scene_synth"][4], g["scene_moving"][4], g["scene_moving"][4]]
    collided = [g["scene_synth"][5], g["scene_moving"][5], g["scene_moving"][5]]
    lines = [g["scene_synth"][6], g["scene_moving"][6], g["scene_moving"][6]]
    return dict(states=states, maps=maps, tracks=tracks, collided=collided, lines=lines, seeded=items)


def workgroup_keeps(states, items, waves=4):
    """Per workgroup of ``waves`` consecutive candidates (five points, 41 states) the mask of the polygons whose closed
    bounding box meets the workgroup's: what ego_areas_kernel lists."""
    lo = np.array([np.min([r.min(0) for r in rings], 0) for rings, _, _ in items])
    hi = np.array([np.max([r.max(0) for r in rings], 0) for rings, _, _ in items])
    keeps = []
    for w in range(0, states.shape[0], waves):
        p = A.coords(states[w:w + waves]).reshape(-1, 2)
        b0, b1 = p.min(0), p.max(0)
        keeps.append((b0[0] <= hi[:, 0]) & (b1[0] >= lo[:, 0]) & (b0[1] <= hi[:, 1]) & (b1[1] >= lo[:, 1]))
    return np.array(keeps)


def area_margin(maps, grouped, p=None):
    """The smallest distance of any point to any edge of its scene's map, and of any finite m to a threshold."""
    p = p or A.DEFAULTS
    edge = min([A.edge_distance(items, pts) for items, pts in zip(maps, grouped["coords"])] + [np.inf])
    f = grouped["m"][np.isfinite(grouped["m"])]
    bounds = np.array([p["driving_direction_compliance_threshold"], p["driving_direction_violation_threshold"]])
    return edge, float(np.abs(f[:, None] - bounds).min()) if f.size else np.inf


def area_conditions(c):
    maps, states = c["maps"], c["states"]
    assert tuple(len(m) for m in maps) == AREA_POLYGONS
    last = len(maps[0]) - (len(c["seeded"]) - len(AREA_AT))
    for at, it in zip(AREA_AT + tuple(range(last, len(maps[0]))), c["seeded"]):
        assert maps[0][at] is it
    assert sum(it[1] == "INTERSECTION" for it in maps[0]) == 3
    assert {it[1] for it in maps[0]} == set(A.LANE_LAYERS + A.DRIVABLE_LAYERS)
    keeps = workgroup_keeps(states[0], maps[0])
    per_pass = np.array([[k[b:b + BLOCK].sum() for b in range(0, len(k), BLOCK)] for k in keeps])
    assert keeps.sum(1).max() >= 257 and per_pass.max() > WAVE and per_pass.shape[1] == 3
    waves = np.array([[k[b:b + WAVE].any() for b in range(0, len(k), WAVE)] for k in keeps])
    assert waves[int(np.argmax(keeps.sum(1)))].all(), waves     # every wavefront of every pass lists something
    grouped = A.ego_areas_grouped(states, maps)
    edge, m = area_margin(maps, grouped)
    assert edge >= MARGIN and m >= MARGIN, (edge, m)
    # the fillers do change flags: the seeded map alone answers differently
    plain = A.ego_areas(states[0], c["seeded"])
    changed = (plain["areas"] != grouped["areas"][0]).mean(axis=(0, 1))
    assert (changed > 0.01).all(), changed
    # and a polygon past the first pass decides one: the list cut at 256 answers differently
    cut = A.ego_areas(states[0], maps[0][:BLOCK])
    assert (cut["areas"] != grouped["areas"][0]).any() and (A.ego_areas(states[0], maps[0][:2 * BLOCK])["areas"]
                                                            != grouped["areas"][0]).any()
    return dict(kept=keeps.sum(1).tolist(), per_pass=per_pass.tolist(), edge=edge, m=m, changed=changed.tolist(),
                grouped=grouped)


# ---- the restatement of the whole chain over scenes, with its margins

def restated(states, maps, tracks, lines, collided, **kw):
    """R.pdm_score per scene over (G, n, 41, 11) host states, the scenes flattened; the margins of the cases."""
    parts = [R.pdm_score(states[g], maps[g], tracks[g], lines[g], collided=collided[g], **kw) for g in range(len(maps))]
    ref = {k: np.concatenate([q[k] for q in parts]) for k in KEYS + ("comfort", "pmax")}
    ref["comfortable"] = ref["comfort"].all(-1).astype(np.float64)
    margins = {k: min(q[k] for q in parts) for k in ("gap_margin", "speed_margin", "angle_margin")}
    margins["axle_margin"] = min([A.edge_distance([it for it in maps[g] if it[1] == "INTERSECTION"], q["axle_points"])
                                  for g, q in enumerate(parts) if len(q["axle_points"])] + [np.inf])
    margins["edge_margin"] = min([A.edge_distance(maps[g], A.coords(states[g])) for g in range(len(maps))] + [np.inf])
    return ref, margins, parts


def hold_margins(tag, m):
    print(f"pdm batch {tag}: margins {m}")
    assert m["gap_margin"] >= MARGIN and m["speed_margin"] >= MARGIN and m["axle_margin"] >= MARGIN
    assert m["edge_margin"] >= MARGIN and m["angle_margin"] >= ANGLE_MARGIN


# ---- 5. many ragged scenes through the chain

def hand_batch():
    """Every hand case of R.hand_cases() but pair_reference, each padded to three candidates by repeating candidate 0
    (the group's maximum stays), as the scenes of one call."""
    cases = [c for c in R.hand_cases() if c[0] != "pair_reference"]
    states = []
    for _, c, _ in cases:
        s = c["states"]
        states.append(np.concatenate([s] + [s[:1]] * (3 - len(s))))
    return cases, np.stack(states)


TRACK_COUNTS = (0, 1, 9, 63, 64, 65, 129, 9, 0, 9, 130, 9)   # packed tracks per scene: what dd_collisions walks
NEAR_AT = (0, 63, 64, 65, 127, 128)                          # and the last
RAGGED_GROUP = 5
RAGGED_SEED = 131
FAR = 10.0


def near_positions(count, near):
    """The packed list positions of ``near`` seeded tracks among ``count``: NEAR_AT where the count reaches them, the
    last position, and the rest spread evenly over what is free."""
    if count <= near:
        return list(range(count))
    want = sorted({p for p in NEAR_AT if p < count - 1} | {count - 1})[:near]
    free = [p for p in range(count) if p not in want]
    extra = [free[int(i)] for i in np.linspace(0, len(free) - 1, near - len(want))] if near > len(want) else []
    out = sorted(set(want) | set(extra))
    assert len(out) == near
    return out


def ego_box(states):
    """The box of every ego quad of (n, 41, 11) states, the shifted TTC quads included."""
    corners, _, shifted = R.ego_quads(states)
    pts = np.concatenate([corners.reshape(-1, 2), shifted.reshape(-1, 2)])
    pts = pts[np.isfinite(pts).all(-1)]
    return pts.min(0), pts.max(0)


def far_tracks(states, count, tag, t_obs=R.T_OBS):
    """``count`` tracks whose boxes over all times stay FAR metres and more from every ego quad's box."""
    lo, hi = ego_box(states)
    out = []
    for i in range(count):
        side = i % 4
        off = FAR + 8.0 + 5.0 * (i // 4)
        cx, cy = [(hi[0] + off, lo[1]), (lo[0] - off, hi[1]), (lo[0], hi[1] + off), (hi[0], lo[1] - off)][side]
        speed = 0.0 if i % 3 else 1.0      # every third one moves, away from the ego's box
        away = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)][side]
        d = np.arange(t_obs) * 0.1 * speed
        kind = ("VEHICLE", "PEDESTRIAN", "TRAFFIC_CONE", "BICYCLE")[i % 4]
        out.append(R.track(f"far_{tag}_{i}", cx + d * away[0], cy + d * away[1], 0.3 * i, 4.0, 2.0, kind, speed,
                           t_obs=t_obs))
    return out


def box_distance(tr, lo, hi):
    b = tr["boxes"][np.asarray(tr["valid"], dtype=bool)].reshape(-1, 2)
    return float(max(lo[0] - b[:, 0].max(), b[:, 0].min() - hi[0], lo[1] - b[:, 1].max(), b[:, 1].min() - hi[1]))


def ragged_case(g, seed=RAGGED_SEED):
    """Twelve scenes x five candidates: golden rows of the three simulator sets, each scene from R.seeded_scene(seed +
    scene, ...) around its own rows with a centerline of its own length, the packed track counts TRACK_COUNTS made up
    by far tracks around the seeded ones; the red-light and the previously collided token ride along uncounted.
    Returns dict(states, maps, tracks (all), near (the seeded tracks that count), collided, lines)."""
    c = dict(states=[], maps=[], tracks=[], near=[], collided=[], lines=[], positions=[])
    for s, count in enumerate(TRACK_COUNTS):
        rows = (np.arange(RAGGED_GROUP) * 19 + 7 * s) % 96
        states = g[f"states_{SIM_SETS[s % 3]}"][rows]
        items, _, _, _, tracks, collided, _ = R.seeded_scene(seed + s, states, lanes=3 - s % 2)
        near = R.drop_tokens(tracks, collided)
        dropped = [tr for tr in tracks if not any(tr is q for q in near)]
        near = near[:count]
        at = near_positions(count, len(near))
        far = far_tracks(states, count - len(near), s)
        packed = []
        for p in range(count):
            packed.append(near[at.index(p)] if p in at else far.pop())
        if count >= 9:       # never packed: in front and in the middle of the list
            packed = dropped[:1] + packed[:count // 2] + dropped[1:] + packed[count // 2:]
        else:
            collided = []
        c["states"].append(states), c["maps"].append(items), c["tracks"].append(packed), c["near"].append(near)
        c["collided"].append(collided), c["positions"].append(at)
        c["lines"].append(R.seeded_centerline(seed + s, tuple(states[0, 0, :3]), vertices=18 + 3 * s))
    c["states"] = np.stack(c["states"])
    return c


def ragged_conditions(c):
    """Assert the conditions of the ragged case on the reference side. Returns (reference, figures)."""
    G = len(TRACK_COUNTS)
    for s in range(G):
        kept = R.drop_tokens(c["tracks"][s], c["collided"][s])
        assert len(kept) == TRACK_COUNTS[s], (s, len(kept))
        assert [i for i, tr in enumerate(kept) if any(tr is q for q in c["near"][s])] == c["positions"][s]
        lo, hi = ego_box(c["states"][s])
        for tr in kept:
            if tr["token"].startswith("far_"):
                assert box_distance(tr, lo, hi) >= FAR, (s, tr["token"])
    assert c["positions"][10] == [0, 63, 64, 65, 127, 128, 129] and c["positions"][6][-1] == 128
    assert c["positions"][5][-2:] == [63, 64] and c["positions"][4][-1] == 63 and c["positions"][3][-1] == 62
    assert len({len(m) for m in c["maps"]}) > 1 and len({len(line) for line in c["lines"]}) == G
    ref, margins, parts = restated(c["states"], c["maps"], c["near"], c["lines"], [[]] * G)
    hold_margins("ragged scenes", margins)
    changed = 0
    for s in range(G):
        o = (s + 1) % G
        other = R.pdm_score(c["states"][s], c["maps"][o], c["near"][o], c["lines"][o])
        changed += any(not np.array_equal(other[k], parts[s][k], equal_nan=True) for k in KEYS)
    discrete = 0
    for s in range(G):
        o = (s + 1) % G
        other = R.pdm_score(c["states"][s], c["maps"][s], c["near"][o], c["lines"][s])
        discrete += any(not np.array_equal(other[k], parts[s][k]) for k in ("no_collision", "ttc", "collision_time_idx",
                                                                             "ttc_time_idx"))
    hit = sum(bool((q["no_collision"] != 1.0).any()) for q in parts)
    close = sum(bool((q["ttc"] != 1.0).any()) for q in parts)
    assert changed >= 9 and hit >= 3 and close >= 3, (changed, hit, close)
    return ref, dict(changed=changed, changed_by_tracks_alone=discrete, hit=hit, close=close, margins=margins)


MANY_SCENES = 257
MANY_CYCLE = (0, 1, 2, 4, 5)      # scenes of the ragged case: 0, 1, 9, 64 and 65 packed tracks


def many_case(c):
    """257 scenes x 1 candidate: candidate 0 of five scenes of the ragged case in a cycle."""
    pick = [MANY_CYCLE[s % len(MANY_CYCLE)] for s in range(MANY_SCENES)]
    return pick, dict(states=np.stack([c["states"][s][:1] for s in pick]), maps=[c["maps"][s] for s in pick],
                      tracks=[c["tracks"][s] for s in pick], collided=[c["collided"][s] for s in pick],
                      lines=[c["lines"][s] for s in pick])


LONG_T_OBS = 70


def long_case(g, rows=24):
    """The moving scene's tracks over 70 times: the same boxes up to time 50, then a box on top of the ego."""
    states = g["states_moving"][:rows]
    seed = int(g["seed"])
    items, _, _, _, tracks, collided, line = g["scene_moving"]
    longer, _ = R.seeded_tracks(seed, g["states_moving"], t_obs=LONG_T_OBS)
    x, y, h = states[0, 20, :3]
    on_top = R.box(x + 1.5 * np.cos(h), y + 1.5 * np.sin(h), h, 6.0, 3.0)
    for a, b in zip(tracks, longer):
        assert a["token"] == b["token"] and np.array_equal(a["boxes"], b["boxes"][:R.T_OBS])
        assert np.array_equal(a["valid"], b["valid"][:R.T_OBS]) and a["heading"] == b["heading"]
        b["boxes"][R.T_OBS:] = on_top
        b["valid"][R.T_OBS:] = True
    # the box does meet the ego: as map 20 it would be a hit
    assert R.quads_touch(R.ego_quads(states[:1])[0][0, 20], on_top)
    return dict(states=states, maps=[items], lines=[line], collided=[collided], tracks=[tracks], longer=[longer])
