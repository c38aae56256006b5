"""The numpy restatement of the rest of the PDM score (tests/pdm_collision_ref.py: no-at-fault collision, TTC,
progress, aggregation) against the golden written by the reference's own PDMScorer
(tests/golden/make_collision_golden.py), the hand-built quirk cases whose answers are known by construction, the three
packers and the argument checks of dd_collisions, dd_progress and dd_pdm_aggregate, on the CPU.

Sets: the simulated states of the three pdm_sim_s3_* goldens on seeded maps, tracks and centerlines (the global one at
6.6e5 / 4.0e6 m), 96 synthetic state arrays, one row with a NaN pose, 24 rows of the moving set under non-default
parameters, the moving set as pairs with its candidate 0. Scenes are rebuilt from the golden's seed. No candidate is
excluded.

Bars (derived, not tuned; printed before every assert):
  no_collision, ttc, drivable_area, driving_direction, the comfort term and both time indices are EQUAL: the generator
  keeps every separating-axis gap and every rear-axle point 1e-6 m, every speed 1e-6 m/s, every used angle 1e-9 rad
  and every comfort signal 1e-5 from what decides it, far above any correct float64 evaluation's rounding (1e-9 m at
  4e6 m).
  raw progress: pdm_collision_ref.raw_progress_bar - per projection four roundings at the largest coordinate (the
  center's two, the segment ends' one each), 16 ulp of the lever arm for sin / cos, 8 ulp of the path length for the
  parameter's products and one rounding per summed segment at the path length; twice, for the two projections. At
  4e6 m with a 24-vertex, 110 m line: 2 (4 x 4.7e-10 + 5e-15 + 2e-13 + 24 x 1.4e-14) = 3.7e-9 m.
  progress term: 2 raw_bar / pmax where it is a quotient, plus 4 ulp of 1; score: that times w_progress / sum(w), plus
  4 ulp of 1.
  At most half of the continuous values may differ from the reference's at all.
Measured here: the restatement reproduces the reference bit for bit (the same numpy on the same host).
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import pdm_area_ref as A
import pdm_collision_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIM_SETS = ("moving", "standing", "global")
ALT_ROWS = 24
NAN_ROW, NAN_AT = 5, 17
EQUAL_KEYS = ("no_collision", "ttc", "drivable_area", "driving_direction", "collision_time_idx", "ttc_time_idx")


def load():
    """The score golden with, per set, the states under states_{name} and the scene rebuilt from the seed under
    scene_{name} (pdm_collision_ref.seeded_scene: items, tokens, route ids, checks, tracks, collided, line)."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "pdm_score_s*.npz")))
    assert len(files) == 1, files
    with np.load(files[0]) as g:
        rec = {k: g[k] for k in g.files}
    seed = int(rec["seed"])
    for k, name in enumerate(SIM_SETS):
        with np.load(os.path.join(GOLDEN, f"pdm_sim_s3_{name}.npz")) as g:
            rec[f"states_{name}"] = g["states"]
        rec[f"scene_{name}"] = R.seeded_scene(seed + k, rec[f"states_{name}"], lanes=3 if k != 1 else 2)
    synth = R.with_velocity(A.synthetic_states(seed))
    rec["states_synth"] = synth
    rec["states_nan"] = synth[NAN_ROW:NAN_ROW + 1].copy()
    rec["states_nan"][0, NAN_AT, A.X] = np.nan
    rec["states_alt"] = rec["states_moving"][:ALT_ROWS]
    rec["scene_synth"] = rec["scene_nan"] = R.seeded_scene(seed + 3, synth)
    rec["area_params_alt"] = A.params(**A.ALT)
    rec["score_params_alt"] = R.score_params(**dict(zip(rec["alt_names"].tolist(), rec["alt_values"].tolist())))
    rec["scene_alt"] = R.seeded_scene(seed, rec["states_moving"], dt=rec["area_params_alt"]["dt"])
    rec["path"] = files[0]
    return rec


@pytest.fixture(scope="module")
def golden():
    return load()


def params_of(g, name):
    return (g["area_params_alt"], g["score_params_alt"]) if name == "alt" else (A.params(), R.score_params())


def restate(g, name, rows=slice(None), reference=None):
    items, _, _, _, tracks, collided, line = g[f"scene_{name}"]
    ap, sp = params_of(g, name)
    return R.pdm_score(g[f"states_{name}"][rows], items, tracks, line, ap, sp, reference=reference, collided=collided)


def golden_ref(g, name):
    ref = {k: g[f"{k}_{name}"] for k in EQUAL_KEYS + ("comfortable", "raw_progress", "progress", "score")}
    with np.errstate(invalid="ignore"):
        ref["pmax"] = np.full(ref["score"].shape, np.max(ref["raw_progress"] * ref["no_collision"] * ref["drivable_area"]))
    return ref


def compare_to(tag, got, ref, raw_bar, sp=None):
    """Print every figure, then return them. ``got`` / ``ref``: dicts over the same candidates; ``got`` carries
    ``comfort`` (N, 6) flags or ``comfortable``; ``ref`` carries ``pmax`` for the bars."""
    comfortable = got["comfortable"] if "comfortable" in got else got["comfort"].all(-1).astype(np.float64)
    wrong = {k: int((got[k] != ref[k]).sum()) for k in EQUAL_KEYS}
    wrong["comfortable"] = int((comfortable != ref["comfortable"]).sum())
    term_bar, score_bar = R.score_bars(ref, raw_bar, sp)
    fig = dict(wrong=wrong, nan_ok=True, over=-np.inf, share=0.0)
    text = []
    with np.errstate(invalid="ignore"):
        for k, bar in (("raw_progress", raw_bar), ("progress", term_bar), ("score", score_bar)):
            a, b = np.asarray(got[k]), ref[k]
            fig["nan_ok"] &= np.array_equal(np.isnan(a), np.isnan(b))
            diff = np.nan_to_num(np.abs(a - b), nan=0.0)
            fig["over"] = max(fig["over"], float((diff - bar).max()))
            share = float(((a != b) & ~np.isnan(b)).mean())
            fig["share"] = max(fig["share"], share)
            text.append(f"{k}: largest difference {diff.max():.3e} (bar {np.max(bar):.3e}), not bit-equal share "
                        f"{share:.3e}")
    print(f"pdm score {tag}: wrong {wrong}; no_collision {np.unique(got['no_collision']).tolist()}, ttc "
          f"{np.unique(got['ttc']).tolist()}; " + "; ".join(text))
    return fig


def hold(fig):
    assert not any(fig["wrong"].values()), fig["wrong"]
    assert fig["nan_ok"]
    assert fig["over"] <= 0.0
    assert fig["share"] <= 0.5


def bar_of(g, name):
    return R.raw_progress_bar(g[f"states_{name}"], g[f"scene_{name}"][6], params_of(g, name)[0])


def test_golden_covers_what_it_should(golden):
    g = golden
    assert os.path.getsize(g["path"]) < 1 << 20
    for k in ("gap", "speed", "axle", "tie", "pmax"):
        assert float(g[f"{k}_margin"]) >= 1e-6, k
    assert float(g["angle_margin"]) >= 1e-9 and float(g["comfort_margin"]) >= 1e-5
    names = SIM_SETS + ("synth",)
    assert set(np.concatenate([g[f"no_collision_{n}"] for n in names]).tolist()) == {0.0, 0.5, 1.0}
    assert set(np.concatenate([g[f"ttc_{n}"] for n in names]).tolist()) == {0.0, 1.0}
    assert (sum(g[f"first_types_{n}"] for n in names) > 0).all()          # all five types decide a first hit
    pmax = [float(np.max(g[f"raw_progress_{n}"] * g[f"no_collision_{n}"] * g[f"drivable_area_{n}"]))
            for n in names + ("alt",)]
    thresholds = [5.0] * len(names) + [g["score_params_alt"]["progress_distance_threshold"]]
    assert {p > t for p, t in zip(pmax, thresholds)} == {True, False}     # both progress branches
    assert (g["score_pair"] != g["score_moving"]).any()                  # group and pair normalisation differ
    assert np.abs(g["states_global"][..., 0]).min() > 6.6e5 and np.isnan(g["states_nan"]).sum() == 1
    tokens = [tr["token"] for tr in g["scene_moving"][4]]
    assert any(R.RED_LIGHT in t for t in tokens) and set(g["scene_moving"][5]) <= set(tokens)
    assert any(not tr["valid"].all() for tr in g["scene_moving"][4])
    assert any(not tr["is_agent"] for tr in g["scene_moving"][4])


@pytest.mark.parametrize("name", SIM_SETS + ("synth", "nan", "alt"))
def test_restatement_matches_the_reference(golden, name):
    g = golden
    got = restate(g, name)
    ref = golden_ref(g, name)
    fig = compare_to(f"restatement vs reference [{name}]", got, ref, bar_of(g, name), params_of(g, name)[1])
    hold(fig)
    if name != "nan":   # the deciding first hits are recorded, and the restatement's own margins are the generator's
        assert np.array_equal(np.bincount(got["types"][got["types"] >= 0], minlength=5)[:5], g[f"first_types_{name}"])
        assert got["gap_margin"] >= 1e-6 and got["speed_margin"] >= 1e-6 and got["angle_margin"] >= 1e-9


def test_pair_normalisation_matches_the_reference(golden):
    """Each candidate of the moving set scored as the pair [candidate 0, candidate]: the reference's values against the
    restatement's per-candidate rule with candidate 0's raw * multi as the reference value."""
    g = golden
    got = restate(g, "moving", reference=float(g["pair_reference"]))
    with np.errstate(invalid="ignore"):
        pmax = np.maximum(float(g["pair_reference"]), g["raw_progress_moving"] * g["no_collision_moving"]
                          * g["drivable_area_moving"])
    ref = dict(golden_ref(g, "moving"), score=g["score_pair"], progress=g["progress_pair"], pmax=pmax)
    hold(compare_to("pairs vs reference [moving]", got, ref, bar_of(g, "moving")))


def check_hand_case(name, out, expected):
    for k, v in expected.items():
        got = out[k][0] if np.ndim(v) == 0 or k in ("types", "ttc_hits") else out[k]
        if k in ("raw_progress", "progress"):
            assert np.allclose(got, v, rtol=0, atol=1e-12, equal_nan=True), (name, k, got, v)
        else:
            assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(v, dtype=np.float64)), (name, k, got, v)


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, c, expected = case
    out = R.pdm_score(c["states"], c["items"], c["tracks"], c["line"], reference=c["reference"], collided=c["collided"])
    assert out["gap_margin"] >= 1e-3 and out["angle_margin"] >= 1e-3, (out["gap_margin"], out["angle_margin"])
    check_hand_case(name, out, expected)


def test_primitives_against_independent_predicates():
    """Random quad pairs and bumper segments at map coordinates: the separating-axis test against vertex containment
    plus edge crossings; the centroid against the corner mean; the projection against dense sampling."""
    rng = np.random.default_rng(3)
    origin = np.array([664431.37, 3997675.12])
    a = origin + R.box(rng.uniform(-3, 3, 400), rng.uniform(-3, 3, 400), rng.uniform(-4, 4, 400), 5.176, 2.297)
    b = origin + R.box(rng.uniform(-3, 3, 400), rng.uniform(-3, 3, 400), rng.uniform(-4, 4, 400),
                       rng.uniform(0.5, 5.0, 400), rng.uniform(0.5, 2.2, 400))
    touch, margin = R.quads_touch(a, b), np.abs(R.gap(a, b))
    seg = a[:, [0, 3]]
    seg_touch, seg_margin = R.segment_touches(seg, b), np.abs(R.gap(seg, b))
    assert 50 < touch.sum() < 350 and 20 < seg_touch.sum() < 380
    for i in range(400):
        if margin[i] > 1e-6:
            assert bool(touch[i]) == R.independent_touch(a[i], b[i]), i
        if seg_margin[i] > 1e-6:
            assert bool(seg_touch[i]) == R.independent_touch(seg[i], b[i]), i
    assert np.abs(R.centroid(b) - b.mean(-2)).max() < 1e-8
    # closed: sharing an edge or a corner counts; a non-finite corner intersects nothing
    sq = A.rect(0, 0, 1, 1)
    assert R.quads_touch(sq, sq + [1.0, 0.0]) and R.quads_touch(sq, sq + [1.0, 1.0]) and not R.quads_touch(sq, sq + [1.5, 0])
    assert R.segment_touches(np.array([[1.0, -1.0], [1.0, 2.0]]), sq)       # along the edge x = 1
    assert not R.segment_touches(np.array([[1.25, -1.0], [1.25, 2.0]]), sq)
    bad = sq.copy()
    bad[2, 0] = np.nan
    assert not R.quads_touch(bad, sq) and not R.quads_touch(sq + [0.5, 0.5], bad)
    line = R.seeded_centerline(4, (664431.37, 3997675.12, 0.7))
    pts = line[rng.integers(0, len(line), 50)] + rng.uniform(-6, 6, (50, 2))
    got = R.project(line, pts[:, 0], pts[:, 1])
    for p, s in zip(pts, got):
        want, bound = R.independent_project(line, p[0], p[1])
        assert abs(s - want) <= bound
    # the first segment on a tie: a point equidistant from both legs of a right angle
    corner = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0]])
    assert R.project(corner, np.array(8.0), np.array(2.0)) == 8.0
    assert np.isnan(R.project(corner, np.array(np.nan), np.array(2.0)))


# ---- the packers

def test_observation_packer(golden):
    from diffusiondrive_amd import simulate as S
    g = golden
    tracks, collided = g["scene_moving"][4], g["scene_moving"][5]
    kept = R.drop_tokens(tracks, collided)
    assert len(kept) == len(tracks) - 2
    few = kept[:3]
    packed = S.pack_observations([R.track_items(tracks), [], R.track_items(few)], "cpu", collided=[collided, [], []])
    assert [t.dtype for t in packed[:5]] == [S.torch.float64, S.torch.uint8, S.torch.float64, S.torch.uint8,
                                             S.torch.int32]
    k = len(kept)
    assert packed.scene_track_off.tolist() == [0, k, k, k + 3]
    assert tuple(packed.boxes.shape) == (k + 3, R.T_OBS, 4, 2) and tuple(packed.valid.shape) == (k + 3, R.T_OBS)
    assert packed.tokens == (tuple(tr["token"] for tr in kept), (), tuple(tr["token"] for tr in few))
    for j, tr in enumerate(kept):
        v = tr["valid"]
        assert np.array_equal(packed.valid[j].numpy().astype(bool), v)
        assert np.array_equal(packed.boxes[j].numpy()[v], tr["boxes"][v]) and np.isfinite(packed.boxes[j].numpy()).all()
        assert packed.heading[j].item() == tr["heading"]
        assert packed.flags[j].item() == (S.FLAG_STOPPED if tr["stopped"] else 0) | (S.FLAG_AGENT if tr["is_agent"] else 0)
    # the duck-typed PDMObservation gives the same arrays (its boxes carry shapely's closing vertex), a mask the same
    # as NaN rows
    duck = S.pack_observations([R.duck_observation(tracks, collided)], "cpu")
    order = [duck.tokens[0].index(t) for t in packed.tokens[0]]
    for a, b in zip(duck[:4], packed[:4]):
        assert S.torch.equal(a[order], b[:k])
    masked = S.pack_observations([[(tr["token"], (tr["boxes"], tr["valid"]), tr["heading"], tr["is_agent"],
                                    tr["stopped"]) for tr in kept]], "cpu")
    assert all(S.torch.equal(a, b[:k]) for a, b in zip(masked[:4], packed[:4]))
    empty = S.pack_observations([[], []], "cpu")
    assert tuple(empty.boxes.shape) == (0, S.MIN_OBS_TIMES, 4, 2) and empty.scene_track_off.tolist() == [0, 0, 0]


def test_observation_packer_rejections():
    from diffusiondrive_amd import simulate as S
    ok = R.track("a", 5.0, 0.0, 0.0, 4.0, 2.0, "VEHICLE", 1.0)
    item = lambda tr, **kw: tuple(kw.get(k, v) for k, v in zip(  # noqa: E731
        ("token", "boxes", "heading", "is_agent", "stopped"), R.track_items([tr])[0]))
    with pytest.raises(ValueError, match=r"boxes are \(T_obs, 4"):
        S.pack_observations([[item(ok, boxes=np.zeros((51, 3, 2)))]], "cpu")
    for bad in (np.nan, np.inf):
        b = ok["boxes"].copy()
        b[7, 2, 1] = bad
        with pytest.raises(ValueError, match="non-finite box"):
            S.pack_observations([[item(ok, boxes=b)]], "cpu")
    with pytest.raises(ValueError, match="T_obs = 49 is below 50"):
        S.pack_observations([[item(ok, boxes=ok["boxes"][:49])]], "cpu")
    with pytest.raises(ValueError, match="duplicate token 'a'"):
        S.pack_observations([[item(ok), item(ok)]], "cpu")
    with pytest.raises(ValueError, match="expected \\(token, boxes"):
        S.pack_observations([[("a", ok["boxes"])]], "cpu")
    duck = R.duck_observation([ok])
    duck._occupancy_maps[3]._geometries[0].exterior.coords = np.zeros((6, 2))
    with pytest.raises(ValueError, match="a box is 4"):
        S.pack_observations([duck], "cpu")
    duck = R.duck_observation([ok])
    duck._occupancy_maps[3].tokens = ["a", "a"]
    with pytest.raises(ValueError, match="duplicate token"):
        S.pack_observations([duck], "cpu")


def test_centerline_packer():
    import types
    from diffusiondrive_amd import simulate as S
    a, b = R.seeded_centerline(1), R.seeded_centerline(2, vertices=7)
    path = types.SimpleNamespace(_states_se2_array=np.concatenate([b, np.zeros((7, 1))], axis=1))
    packed = S.pack_centerlines([a, path], "cpu")
    assert packed.verts.dtype == S.torch.float64 and packed.scene_off.dtype == S.torch.int32
    assert packed.scene_off.tolist() == [0, 24, 31]
    assert np.array_equal(packed.verts.numpy(), np.concatenate([a, b]))
    with pytest.raises(ValueError, match="fewer than 2"):
        S.pack_centerlines([a[:1]], "cpu")
    with pytest.raises(ValueError, match="non-finite"):
        S.pack_centerlines([np.array([[0.0, 0.0], [np.nan, 1.0]])], "cpu")
    with pytest.raises(ValueError, match=r"\(L, 2\)"):
        S.pack_centerlines([np.zeros((4, 3))], "cpu")


def test_map_packer_layers(golden):
    """layers=None is today's result bit for bit; a layer list keeps those polygons alone, in order."""
    from diffusiondrive_amd import simulate as S
    from test_ego_areas import unpack
    maps = [golden["scene_synth"][0], [], golden["scene_moving"][0]]
    plain, none = S.pack_drivable_maps(maps, "cpu"), S.pack_drivable_maps(maps, "cpu", None)
    assert all(S.torch.equal(a, b) for a, b in zip(plain, none))
    only = S.pack_drivable_maps(maps, "cpu", layers=("INTERSECTION",))
    counts = [sum(it[1] == "INTERSECTION" for it in m) for m in maps]
    assert counts[0] >= 1 and only.scene_poly_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    want = [it for it in maps[0] if it[1] == "INTERSECTION"]
    for (rings, kind), (want_rings, _, _) in zip(unpack(only, 0), want):
        assert kind == S.KIND_DRIVABLE and all(np.array_equal(a, b) for a, b in zip(rings, want_rings))
    with pytest.raises(ValueError, match="unknown layer names"):
        S.pack_drivable_maps(maps, "cpu", layers=("WALKWAYS",))


# ---- the C entries on a machine without a GPU

def score_params_with(lib, **kw):
    from diffusiondrive_amd import _lib
    q = _lib.DDScoreParams()
    lib.dd_default_score_params(ctypes.byref(q))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def call_collisions(lib, ptr, n=96, per_group=96, scenes=1, num_tracks=3, num_times=51, num_polys=2, null=(),
                    stream=None, area=None, **over):
    """dd_collisions with every array at ``ptr`` but for the names in ``null``; ``area`` overrides fields of the
    default dd_area_params, ``over`` of the default dd_score_params."""
    from diffusiondrive_amd import _lib
    from test_ego_areas import area_params_with
    at = lambda name: None if name in null else ptr  # noqa: E731
    o = None if "obs" in null else _lib.DDObservations(at("boxes"), at("valid"), at("heading"), at("flags"),
                                                       at("scene_track_off"), num_tracks, num_times)
    m = None if "intersections" in null else _lib.DDDrivableMaps(at("verts"), at("ring_off"), at("poly_ring_off"),
                                                                 at("poly_kind"), at("scene_poly_off"), num_polys)
    ap = None if "area_params" in null else area_params_with(lib, **(area or {}))
    sp = None if "score_params" in null else score_params_with(lib, **over)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    rc = lib.dd_collisions(at("states"), at("areas"), n, per_group, ref(o), ref(m), scenes, ref(ap), ref(sp),
                           at("work"), at("out_no_collision"), at("out_collision_time_idx"), at("out_ttc"),
                           at("out_ttc_time_idx"), stream)
    return rc, lib.dd_last_error().decode()


def call_progress(lib, ptr, n=96, per_group=96, scenes=1, num_verts=24, null=(), stream=None, **area):
    from diffusiondrive_amd import _lib
    from test_ego_areas import area_params_with
    at = lambda name: None if name in null else ptr  # noqa: E731
    c = None if "lines" in null else _lib.DDCenterlines(at("verts"), at("scene_off"), num_verts)
    ap = None if "area_params" in null else area_params_with(lib, **area)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    rc = lib.dd_progress(at("states"), n, per_group, ref(c), scenes, ref(ap), at("out_raw_progress"), stream)
    return rc, lib.dd_last_error().decode()


def call_aggregate(lib, ptr, n=96, per_group=96, null=(), reference=None, stream=None, **over):
    at = lambda name: None if name in null else ptr  # noqa: E731
    sp = None if "score_params" in null else score_params_with(lib, **over)
    rc = lib.dd_pdm_aggregate(at("no_collision"), at("drivable_area"), at("driving_direction"), at("raw_progress"),
                              at("ttc"), at("comfort"), n, per_group, ctypes.byref(sp) if sp is not None else None,
                              reference, at("out_score"), at("out_progress"), stream)
    return rc, lib.dd_last_error().decode()


def count_cases(with_scenes=True):
    cases = [(dict(n=0), "N = 0"), (dict(n=-5), "N = -5"), (dict(per_group=0), "per_group = 0"),
             (dict(per_group=-2), "per_group = -2"), (dict(per_group=7), "not a multiple of per_group = 7")]
    if with_scenes:
        cases += [(dict(scenes=2), "G = 2"), (dict(per_group=48, scenes=1), "G = 1"), (dict(scenes=0), "G = 0")]
    return cases


def score_param_cases():
    nan, inf = float("nan"), float("inf")
    cases = []
    for field in R.SCORE_DEFAULTS:
        cases += [(dict([(field, v)]), f"dd_score_params.{field}") for v in (-1.0, nan, inf)]
    cases.append((dict(progress_weight=0.0, ttc_weight=0.0, comfortable_weight=0.0), "is zero"))
    return cases


def collisions_rejection_cases():
    """(keyword arguments of call_collisions, text dd_last_error() must carry): every rejection dd_collisions
    documents."""
    nan, inf = float("nan"), float("inf")
    cases = count_cases()
    for name in ("states", "areas", "obs", "intersections", "area_params", "score_params", "work", "out_no_collision",
                 "out_collision_time_idx", "out_ttc", "out_ttc_time_idx"):
        cases.append((dict(null=(name,)), f"{name} is null"))
    cases += [(dict(null=("scene_track_off",)), "dd_observations.scene_track_off is null"),
              (dict(null=("scene_track_off",), num_tracks=0), "dd_observations.scene_track_off is null"),
              (dict(num_tracks=-1), "dd_observations.num_tracks = -1"),
              (dict(num_times=49), "dd_observations.num_times = 49"),
              (dict(null=("scene_poly_off",)), "dd_drivable_maps.scene_poly_off is null"),
              (dict(null=("scene_poly_off",), num_polys=0), "dd_drivable_maps.scene_poly_off is null"),
              (dict(num_polys=-1), "dd_drivable_maps.num_polys = -1")]
    cases += [(dict(null=(f,)), f"dd_observations.{f} is null") for f in ("boxes", "valid", "heading", "flags")]
    cases += [(dict(null=(f,)), f"dd_drivable_maps.{f} is null") for f in ("verts", "ring_off", "poly_ring_off")]
    for field in ("half_length", "half_width", "rear_axle_to_center", "dt"):
        cases += [(dict(area=dict([(field, v)])), f"dd_area_params.{field}") for v in (0.0, -1.0, nan, inf)]
    cases += score_param_cases()
    cases.append((dict(ahead_angle=2.7), "is above behind_angle"))
    return cases


def progress_rejection_cases():
    nan, inf = float("nan"), float("inf")
    cases = count_cases()
    cases += [(dict(null=(name,)), f"{name} is null") for name in ("states", "lines", "area_params", "out_raw_progress")]
    cases += [(dict(null=("verts",)), "dd_centerlines.verts is null"),
              (dict(null=("scene_off",)), "dd_centerlines.scene_off is null"),
              (dict(num_verts=1), "dd_centerlines.num_verts = 1"),
              (dict(n=96, per_group=32, scenes=3, num_verts=5), "dd_centerlines.num_verts = 5")]
    cases += [(dict(rear_axle_to_center=v), "dd_area_params.rear_axle_to_center") for v in (0.0, -1.0, nan, inf)]
    return cases


def aggregate_rejection_cases():
    cases = count_cases(with_scenes=False)
    cases += [(dict(null=(name,)), f"{name} is null")
              for name in ("no_collision", "drivable_area", "driving_direction", "raw_progress", "ttc", "comfort",
                           "score_params", "out_score", "out_progress")]
    return cases + score_param_cases()


def test_defaults_and_rejections_need_no_device():
    """The defaults are the reference's, and every bad argument of the three entries is refused before any device call
    (the pointers are host addresses that a launch could not use; the sentinel-filled buffer stays untouched)."""
    from diffusiondrive_amd import _lib
    from diffusiondrive_amd import simulate as S
    lib = _lib.load()
    p = S.default_score_params(lib)
    assert {k: getattr(p, k) for k, _ in p._fields_} == R.SCORE_DEFAULTS
    assert lib.dd_collisions_work(0) > 0 and lib.dd_collisions_work(7) == 28
    buf = (ctypes.c_double * 16)(*([-7.0] * 16))
    ptr = ctypes.addressof(buf)
    for call, who, cases in ((call_collisions, "dd_collisions: ", collisions_rejection_cases()),
                             (call_progress, "dd_progress: ", progress_rejection_cases()),
                             (call_aggregate, "dd_pdm_aggregate: ", aggregate_rejection_cases())):
        assert len(cases) > 15
        for kw, text in cases:
            rc, msg = call(lib, ptr, **kw)
            assert rc == -1 and msg.startswith(who) and text in msg, (who, kw, rc, msg)
    assert list(buf) == [-7.0] * 16
