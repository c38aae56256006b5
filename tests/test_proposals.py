"""The numpy restatement of PDM-Closed's proposal generation (tests/pdm_proposal_ref.py) against the golden written by
the reference's own PDMGenerator (tests/golden/make_proposal_golden.py), its interpolation against real scipy, the
hand-built quirk cases whose answers are known by construction, and the two packers, on the CPU.

Bars (derived, not tuned; printed before every assert). lead_index is EQUAL: the generator keeps every corridor
membership steady under r +- 5e-3 m, every compared progress 1e-6 m apart and every argmin's runner-up 1e-6 m behind.
A continuous output's bar is the larger of
  a floor (pdm_proposal_ref.floors): progress / leader progress - the projection's two differences at the largest
  coordinate (4 spacings), its products (8 ulp of the path length), one rounding per summed segment at the path
  length, and sin / cos on the ego quad's lever arms (16 ulp of the vehicle length) through the distance on relative
  coordinates; proposals - that carried through a slope of at most 1, plus scipy's slope * dx + y_lo at the largest
  coordinate (3 spacings) and sin, cos, arctan2 of the heading (8 ulp of pi). At 4.0e6 m with a 24-vertex, 110 m path:
  4 x 4.7e-10 + 2e-13 + 24 x 1.4e-14 + 1.8e-14 = 1.9e-9 m and 3.3e-9 m; at the origin about 6e-13 m;
  and 16 times the largest difference between the restatement in float64 and in numpy.longdouble on the case at hand
  (the conditioning of the 40-step recurrence and of pow(., 10) on the reference's side; the factor covers a pow that
  rounds differently from glibc's), computed at run time. It never measures the code under test.
No share-of-values cap. Measured here: the restatement reproduces the reference to 3e-14 (the same numpy on the same
host; the leader's progress of the crawl differs in its last bits where shapely's substring is restated).
"""
import glob
import os

import numpy as np
import pytest

import pdm_area_ref as A
import pdm_collision_ref as R
import pdm_proposal_ref as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def load():
    """The golden with the scenes rebuilt from its seed under ``scenes`` and, per scene, the restatement in float64
    under ``ref`` and its bars under ``bars`` (computed once and shared)."""
    if "golden" not in _CACHE:
        files = sorted(glob.glob(os.path.join(GOLDEN, "pdm_proposals_s*.npz")))
        assert len(files) == 1, files
        with np.load(files[0]) as g:
            rec = {k: g[k] for k in g.files}
        rec["scenes"] = Q.golden_scenes(int(rec["seed"]))
        assert list(rec["scenes"]) == rec["names"].tolist()
        rec["ref"], rec["bars"], rec["gaps"] = {}, {}, {}
        for name, scene in rec["scenes"].items():
            rec["ref"][name] = Q.generate_scenes([scene])
            rec["bars"][name], rec["gaps"][name] = Q.bars([scene], rec["ref"][name])
        _CACHE["golden"] = rec
    return _CACHE["golden"]


def golden_of(g, name):
    return {k: g[f"{k}_{name}"] for k in Q.KEYS + ("lead_index",)}


@pytest.mark.parametrize("name", ("origin", "far", "light", "crawl"))
def test_restatement_reproduces_the_reference(name):
    g = load()
    ref = g["ref"][name]
    assert ref["corridor"] and ref["ahead"] >= 1e-6 and ref["argmin"] >= 1e-6, (ref["ahead"], ref["argmin"])
    print(f"proposals [{name}]: float64 against longdouble {g['gaps'][name]}")
    Q.compare(f"restatement vs reference [{name}]", ref, golden_of(g, name), g["bars"][name])


def test_golden_covers_the_branches():
    g = load()
    kinds = set()
    changes = False
    for name, scene in g["scenes"].items():
        k = len(Q.scene_objects(scene["tracks"], scene["rings"], scene["collided"])[0])
        li = g[f"lead_index_{name}"][:, 2:]
        kinds |= {"free"} if (li == Q.FREE).any() else set()
        kinds |= {"track"} if ((li >= 0) & (li < k)).any() else set()
        kinds |= {"ring"} if (li >= k).any() else set()
        changes |= bool((np.diff(li, axis=1) != 0).any())
    fallback = {bool(f) for name, scene in g["scenes"].items()
                for f in Q.generate(scene["paths"][:1], [], [], scene["ego"], scene["targets"])["fallback"]}
    assert kinds == {"free", "track", "ring"} and changes and fallback == {True, False}
    assert float(g["ahead_margin"]) >= 1e-6 and float(g["argmin_margin"]) >= 1e-6 and float(g["clip_margin"]) >= 1e-9


def test_interpolate_is_scipys_bit_for_bit():
    interp1d = pytest.importorskip("scipy.interpolate").interp1d
    g = load()
    dup = Q.straight_path([0.0, 10.0, 20.0, 30.0, 30.0, 40.0, 50.0, 60.0, 200.0])
    paths = [q for scene in g["scenes"].values() for q in scene["paths"]] + [dup]
    rng = np.random.default_rng(11)
    for path in paths:
        s, length = path["progress"], path["progress"][-1]
        d = np.concatenate([rng.uniform(-5.0, length + 5.0, 500), s, s + 1e-9, s - 1e-9, [0.0, 1e-5, length, np.nan]])
        with np.errstate(invalid="ignore", divide="ignore"):
            want = interp1d(s, path["xyh"], axis=0)(np.clip(d, 1e-5, length))
            want[..., 2] = np.arctan2(np.sin(want[..., 2]), np.cos(want[..., 2]))
        want[np.isnan(want)] = 0.0
        assert np.array_equal(Q.interpolate(path, d), want)


def test_projection_is_the_scorers():
    g = load()
    rng = np.random.default_rng(5)
    for scene in g["scenes"].values():
        line = scene["paths"][0]["xyh"][:, :2]
        pts = line[rng.integers(len(line), size=50)] + rng.normal(0.0, 4.0, (50, 2))
        for x, y in pts:
            assert Q.project(line, x, y) == float(R.project(line, x, y))


@pytest.mark.parametrize("case", Q.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, scene, expected = case
    out = Q.generate(scene["paths"], scene["tracks"], scene["rings"], scene["ego"], scene["targets"])
    assert out["corridor"], name
    Q.check_hand_case(name, out, expected, scene)


def test_the_first_step_runs_against_the_zero_row():
    """Index 1 copies row 0, which is the zero row: s_alpha = min_gap, and 5 m/s brakes at the clip bound."""
    name, scene, _ = Q.hand_cases()[0]
    out = Q.generate(scene["paths"], [], [], scene["ego"], scene["targets"])
    assert abs(out["idm"][0, 1, 1] - (5.0 - 0.3)) <= 1e-15 and out["idm"][0, 1, 0] == 20.0 + 0.1 * 5.0


def test_pack_paths():
    from diffusiondrive_amd import simulate as S
    g = load()
    scene = g["scenes"]["far"]
    packed = S.pack_paths([scene["raw_paths"]], "cpu")
    assert packed.paths_per_scene == 3 and packed.path_off.tolist() == [0, 24, 48, 72]
    assert np.array_equal(packed.progress.numpy(), np.concatenate([q["progress"] for q in scene["paths"]]))
    assert np.array_equal(packed.verts.numpy(), np.concatenate([q["xyh"] for q in scene["paths"]]))
    duck = [type("P", (), dict(_states_se2_array=q["xyh"], _progress=q["progress"]))() for q in scene["paths"]]
    again = S.pack_paths([duck], "cpu")
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(packed[:3], again[:3]))
    wrapped = np.array([[0.0, 0.0, 3.1], [-1.0, 0.0, -3.1], [-2.0, 0.1, 3.0]])
    assert np.all(np.abs(np.diff(S.pack_paths([[wrapped]], "cpu").verts.numpy()[:, 2])) < 1.0)
    ok = scene["raw_paths"][0]
    for bad, text in (([[ok[:1]]], "fewer than 2"), ([[np.where(np.arange(24)[:, None] == 3, np.nan, ok)]], "non-finite"),
                      ([[np.array([[1.0, 1.0, 0.0], [1.0, 1.0 + 1e-6, 0.0]])]], "above 1e-5"),
                      ([[ok], [ok, ok]], "the same in every scene"), ([[ok[:, :2]]], r"\(V, 3\)")):
        with pytest.raises(ValueError, match=text):
            S.pack_paths(bad, "cpu")


def test_pack_lead_objects():
    from diffusiondrive_amd import simulate as S
    g = load()
    scene = g["scenes"]["origin"]
    items, rings = Q.lead_items(scene)
    packed = S.pack_lead_objects([items], "cpu", stop_polygons=[rings], collided=[scene["collided"]])
    kept, _ = Q.scene_objects(scene["tracks"], scene["rings"], scene["collided"])
    assert packed.tokens[0][:len(kept)] == tuple(tr["token"] for tr in kept) and len(packed.tokens[0]) == len(kept) + 1
    assert packed.scene_track_off.tolist() == [0, len(kept)] and packed.ring_off.tolist() == [0, 4]
    assert np.array_equal(packed.speed.numpy(), [tr["speed"] or 0.0 for tr in kept])
    assert np.array_equal(packed.stop_verts.numpy(), rings[0])
    # the duck-typed observation: red-light tokens in the maps are KEPT as rings, collided ones dropped
    light = R.track(f"{R.RED_LIGHT}_a", 0.0, 0.0, 0.0, 1.0, 1.0, "VEHICLE", 0.0)
    light["boxes"][:] = rings[0]
    duck = R.duck_observation(scene["tracks"] + [light], scene["collided"])
    del duck.unique_objects[light["token"]]
    again = S.pack_lead_objects([duck], "cpu")
    for a, b in zip(packed[:8], again[:8]):
        assert np.array_equal(a.numpy(), b.numpy())
    with pytest.raises(ValueError, match="below 41"):
        S.pack_lead_objects([[(t, b[:40], h, a, s, v) for t, b, h, a, s, v in items]], "cpu")
    with pytest.raises(ValueError, match="fewer than 3"):
        S.pack_lead_objects([items], "cpu", stop_polygons=[[rings[0][:2]]])
    with pytest.raises(ValueError, match="non-finite vertex"):
        S.pack_lead_objects([items], "cpu", stop_polygons=[[rings[0] * np.nan]])
    with pytest.raises(ValueError, match="speed"):
        S.pack_lead_objects([[it[:5] for it in items]], "cpu")
    with pytest.raises(ValueError, match="duplicate token"):
        S.pack_lead_objects([items + items[:1]], "cpu")
