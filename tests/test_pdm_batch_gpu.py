"""The PDM scoring chain on the GPU at batch structure: groups past one workgroup of dd_pdm_aggregate, dd_progress past
one block over ragged centerlines, more polygons than one listing pass of dd_ego_areas, ragged track counts across the
chunk of 64 of dd_collisions, 257 scenes, 70 observation times. The inputs and the conditions that make each case
bite are tests/pdm_batch_util.py's, held on the CPU by tests/test_pdm_batch.py.

Truth is what the suite already trusts: the goldens and the numpy restatements pdm_collision_ref / pdm_area_ref.
Bars (the project's own; every case prints its figures before asserting):
  no_collision, ttc, drivable_area, driving_direction, the comfort flags, the area flags, both time indices: EQUAL;
  the cases' own margins are printed and asserted (1e-7 for gaps, speeds, axle points and points to edges, 1e-9 rad).
  raw progress: pdm_collision_ref.raw_progress_bar; progress term and score: pdm_collision_ref.score_bars (with a raw
  bar of 0 where dd_pdm_aggregate is fed the reference's own inputs: the term's and the score's 4 ulp remain).
  share cap: at most half of the continuous values may differ from the reference's at all.
  BIT-EQUAL, no tolerance, wherever a relation follows from the kernels' design (deterministic, no atomics, one
  candidate per wavefront or thread, culls that are conservative by construction): a candidate in a larger group
  against the same row in a group of 96, a scene in a batch against the scene alone, the batch reversed, a cull
  off against on, 70 observation times against 51.
Measured on an MI355X: DESIGN.md sections 16 and 17.
"""
import os

import numpy as np
import pytest
import torch

import pdm_area_ref as A
import pdm_batch_util as U
import pdm_collision_ref as R
from test_collisions import bar_of, check_hand_case, compare_to, golden_ref, hold, load
from test_collisions_gpu import dev, run_twice
from test_ego_areas import compare_to as compare_areas, hold as hold_areas
from test_ego_areas_gpu import flat, run_twice as areas_twice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load()


@pytest.fixture(scope="module")
def ragged(golden):
    return U.ragged_case(golden)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.int64), b.view(np.int64)
    return a.shape == b.shape and bool((a == b).all())


def largest_difference(a, b):
    with np.errstate(invalid="ignore"):
        return float(np.nan_to_num(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))).max())


def hold_bit_equal(tag, got, want, take=None):
    """Every output of ``got`` against ``want`` (rows ``take`` of it): printed, then held with no tolerance."""
    worst = 0.0
    for k in want:
        w = want[k] if take is None else want[k][take]
        worst = max(worst, largest_difference(got[k], w))
    print(f"pdm batch {tag}: largest difference over {len(want)} outputs {worst:.3e}")
    for k in want:
        assert same_bits(got[k], want[k] if take is None else want[k][take]), (tag, k)


def scene_of(scene):
    items, _, _, _, tracks, collided, line = scene
    return [items], [tracks], [line], [collided]


# ---- 1. group sizes past one workgroup

def test_group_of_600_against_the_same_rows_in_a_group_of_96(gpu, golden):
    """One scene, per_group = 600: three stride steps of aggregate_kernel, the maximum in the third (index 599,
    wavefront 1), the second largest in the second; 150 workgroups of the per-candidate kernels. Candidate i is bit-
    equal to golden row rows[i] of the per_group = 96 run, which is at the golden's values."""
    g = golden
    states, rows, scenes, _ = U.group_case(g, ("moving",), 600, 3, (256, 512))
    maps, tracks, lines, collided = scene_of(scenes[0])
    base = run_twice(dev(g["states_moving"][None]), maps, tracks, lines, collided)
    hold(compare_to("group of 96 vs reference [moving]", base, golden_ref(g, "moving"), bar_of(g, "moving")))
    got = run_twice(dev(states), maps, tracks, lines, collided)
    hold_bit_equal("group of 600 vs rows of the group of 96", got, base, rows[0])
    ref = {k: v[rows[0]] for k, v in golden_ref(g, "moving").items()}
    hold(compare_to("group of 600 vs reference [moving]", got, ref, bar_of(g, "moving")))


def test_three_scenes_of_257_against_each_scene_alone(gpu, golden):
    """G = 3, per_group = 257 (65 workgroups a scene, the last with three spare wavefronts; the second stride step of
    aggregate_kernel holds one candidate: the maximum): each scene bit-equal to itself alone at 96, row for row."""
    g = golden
    names = ("moving", "standing", "global")
    states, rows, scenes, _ = U.group_case(g, names, 257, 3, (64, 256))
    args = [[s[i] for s in scenes] for i in (0, 4, 6, 5)]
    got = run_twice(dev(states), *args)
    for k, name in enumerate(names):
        base = run_twice(dev(g[f"states_{name}"][None]), *scene_of(scenes[k]))
        hold(compare_to(f"group of 96 vs reference [{name}]", base, golden_ref(g, name), bar_of(g, name)))
        part = {key: v[k * 257:(k + 1) * 257] for key, v in got.items()}
        hold_bit_equal(f"scene {k} of 3 x 257 [{name}] vs alone at 96", part, base, rows[k])


# ---- 2. dd_pdm_aggregate on its own

@pytest.mark.parametrize("per_group", U.AGG_GROUPS)
def test_aggregate_alone(gpu, per_group):
    """Six scenes of synthetic sub-scores (the maximum at index 0, at the last index, in wavefront 2 or 3 only, at the
    5.0 threshold exactly, a NaN, every multiplier 0) against R.aggregate per scene, without and with a per-scene
    progress_reference (below, above, between, 5.0, 0, NaN). The inputs are the reference's own: 4 ulp remain."""
    from diffusiondrive_amd import simulate as S
    c = U.aggregate_case(per_group, 100 + per_group)
    names = ("no_collision", "drivable_area", "driving_direction", "raw_progress", "ttc")
    ins = [dev(c[k]) for k in names] + [dev(c["comfort"])]
    for tag, reference in (("group", None), ("pairs", c["reference"])):
        kw = dict(progress_reference=None if reference is None else dev(reference))
        score, term = S.aggregate(*ins, **kw)
        again = S.aggregate(*ins, **kw)
        torch.cuda.synchronize()
        assert score.shape == term.shape == (U.AGG_SCENES, per_group)
        got = dict(score=score.cpu().numpy(), progress=term.cpu().numpy())
        assert same_bits(got["score"], again[0].cpu().numpy()) and same_bits(got["progress"], again[1].cpu().numpy())
        ref = U.aggregate_ref(c, reference)
        term_bar, score_bar = R.score_bars(ref, 0.0)
        equal = total = 0
        for k, bar in (("progress", term_bar), ("score", score_bar)):
            assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (tag, k)
            with np.errstate(invalid="ignore"):
                diff = np.nan_to_num(np.abs(got[k] - ref[k]))
            equal += int(((got[k] == ref[k]) | np.isnan(ref[k])).sum())
            total += got[k].size
            print(f"pdm batch aggregate alone, per_group {per_group}, {tag}: {k} largest difference {diff.max():.3e} "
                  f"(bar {np.max(bar):.3e})")
            assert (diff <= bar).all(), (tag, k, float(diff.max()))
        print(f"pdm batch aggregate alone, per_group {per_group}, {tag}: {equal} of {total} values bit-equal")
        assert total - equal <= total // 2


# ---- 3. dd_progress on its own

def test_progress_alone(gpu, golden):
    """G = 7 x 75 = 525 candidates: three blocks of progress_kernel with scene boundaries inside them, ragged
    centerlines of 2, 3, 24, 300, 7 (two zero-length segments), 4 (a hairpin with exact ties) and 24 (global frame)
    vertices, the first candidate of every scene at the previous scene's line end."""
    from diffusiondrive_amd import simulate as S
    c = U.progress_case(int(golden["seed"]))
    ap = c["area_params"]
    states = dev(c["states"])
    raw = S.progress(states, c["lines"], area_params=dict(rear_axle_to_center=U.PROGRESS_AXLE))
    again = S.progress(states, c["lines"], area_params=dict(rear_axle_to_center=U.PROGRESS_AXLE))
    torch.cuda.synchronize()
    got = raw.cpu().numpy()
    assert got.shape == (U.PROGRESS_SCENES, U.PROGRESS_GROUP) and same_bits(got, again.cpu().numpy())
    want = np.stack([R.raw_progress(c["states"][g], c["lines"][g], ap) for g in range(U.PROGRESS_SCENES)])
    bars = np.array([R.raw_progress_bar(c["states"][g], c["lines"][g], ap) for g in range(U.PROGRESS_SCENES)])
    diff = np.abs(got - want)
    share = float((got != want).mean())
    print(f"pdm batch progress alone: largest difference per scene {diff.max(1).tolist()} (bars {bars.tolist()}), not "
          f"bit-equal share {share:.3e}; on the exact scenes {diff[c['exact']].max():.3e}")
    assert np.isfinite(got).all() and (diff <= bars[:, None]).all() and share <= 0.5
    assert same_bits(got[c["exact"]], want[c["exact"]])
    worst = 0.0
    for g in range(U.PROGRESS_SCENES):
        ind, bound = U.independent_progress(c, g)
        off = np.abs(got[g] - ind)[~c["ties"][g]]
        worst = max(worst, float(off.max()) / bound)
        assert (off <= bound).all(), (g, float(off.max()), bound)
    print(f"pdm batch progress alone: {int((~c['ties']).sum())} candidates against the dense sampling, the largest "
          f"difference {worst:.3f} of its bound")


# ---- 4. more polygons than one listing pass

def test_more_polygons_than_one_listing_pass(gpu, golden):
    """Scenes of 600, 3 and 0 polygons x 8 candidates: three listing passes in scene 0, the first workgroup keeping
    303 polygons (120, 134 and 49 a pass) with every wavefront of every pass listing some. Flags and scores against
    A.ego_areas_grouped, the cull off bit-equal, then pdm_score over the same scenes against the restatement (three
    INTERSECTION polygons in scene 0, none after it)."""
    g = golden
    c = U.area_case(g, int(g["seed"]))
    grouped = A.ego_areas_grouped(c["states"], c["maps"])
    edge, m = U.area_margin(c["maps"], grouped)
    print(f"pdm batch polygons: smallest distance to an edge {edge:.3e} m, of m to a threshold {m:.3e}")
    assert edge >= U.MARGIN and m >= U.MARGIN
    states = dev(c["states"])
    got = areas_twice(states, c["maps"])
    hold_areas(compare_areas("600, 3 and 0 polygons", got, flat(grouped)))
    os.environ["DDMI_EGO_AREAS_CULL"] = "0"
    try:
        uncut = areas_twice(states, c["maps"])
    finally:
        del os.environ["DDMI_EGO_AREAS_CULL"]
    hold_bit_equal("polygons, the cull off vs on", uncut, got)
    ref, margins, _ = U.restated(c["states"], c["maps"], c["tracks"], c["lines"], c["collided"])
    U.hold_margins("polygons", margins)
    scored = run_twice(states, c["maps"], c["tracks"], c["lines"], c["collided"])
    bar = max(R.raw_progress_bar(c["states"][s], c["lines"][s]) for s in range(3))
    hold(compare_to("pdm_score over 600, 3 and 0 polygons", scored, ref, bar))
    assert same_bits(scored["drivable_area"], got["drivable_area"])


# ---- 5. many ragged scenes through the chain

def test_hand_cases_as_one_batch(gpu):
    """The 20 hand cases (all but pair_reference), three candidates each, as the scenes of one call: each scene bit-
    equal to the case alone and at its constructed answer. The TTC intersection cases sit behind scenes of other
    polygon, INTERSECTION and track counts."""
    cases, states = U.hand_batch()
    per_scene = [[c[key] for _, c, _ in cases] for key in ("items", "tracks", "line", "collided")]
    got = run_twice(dev(states), *per_scene)
    for s, (name, c, expected) in enumerate(cases):
        alone = run_twice(dev(states[s][None]), [c["items"]], [c["tracks"]], [c["line"]], [c["collided"]])
        part = {k: v[3 * s:3 * s + 3] for k, v in got.items()}
        for k in alone:
            assert same_bits(part[k], alone[k]), (name, k)
        ref = R.pdm_score(states[s], c["items"], c["tracks"], c["line"], collided=c["collided"])
        out = {k: v for k, v in part.items() if k != "comfort"}
        out["types"], out["ttc_hits"] = ref["types"], ref["ttc_hits"]     # the device does not report these
        n = c["states"].shape[0]
        check_hand_case(name, {k: v[:n] for k, v in out.items()}, dict(expected))
        for k in ("no_collision", "ttc", "collision_time_idx", "ttc_time_idx", "drivable_area"):
            assert np.array_equal(out[k], ref[k]), (name, k)
    print(f"pdm batch hand cases: {len(cases)} scenes bit-equal to the cases alone")


def ragged_args(c, order=None):
    order = range(len(c["maps"])) if order is None else order
    return (dev(c["states"][list(order)]), [c["maps"][s] for s in order], [c["tracks"][s] for s in order],
            [c["lines"][s] for s in order], [c["collided"][s] for s in order])


def test_ragged_track_counts(gpu, ragged):
    """G = 12 x 5 with 0, 1, 9, 63, 64, 65, 129, 9, 0, 9, 130 and 9 packed tracks, the seeded ones at list positions
    0, 63, 64, 65, 127, 128 and the last among far ones, against the restatement over the near tracks; the cull off
    and the scenes reversed, bit-equal."""
    c = ragged
    G = len(U.TRACK_COUNTS)
    ref, margins, _ = U.restated(c["states"], c["maps"], c["near"], c["lines"], [[]] * G)
    U.hold_margins("ragged scenes", margins)
    got = run_twice(*ragged_args(c))
    bar = max(R.raw_progress_bar(c["states"][s], c["lines"][s]) for s in range(G))
    hold(compare_to("12 ragged scenes", got, ref, bar))
    os.environ["DDMI_COLLISIONS_CULL"] = "0"
    os.environ["DDMI_EGO_AREAS_CULL"] = "0"
    try:
        uncut = run_twice(*ragged_args(c))
    finally:
        del os.environ["DDMI_COLLISIONS_CULL"], os.environ["DDMI_EGO_AREAS_CULL"]
    hold_bit_equal("ragged scenes, both culls off vs on", uncut, got)
    back = run_twice(*ragged_args(c, range(G - 1, -1, -1)))
    n = U.RAGGED_GROUP
    turned = {k: np.concatenate([v[s * n:(s + 1) * n] for s in range(G - 1, -1, -1)]) for k, v in back.items()}
    hold_bit_equal("ragged scenes reversed, turned back", turned, got)


def test_257_scenes_of_one_candidate(gpu, ragged):
    """G = 257, per_group = 1: five scenes of the ragged case (0, 1, 9, 64 and 65 tracks) in a cycle; result g is bit-
    equal to that scene's single-candidate run."""
    pick, many = U.many_case(ragged)
    got = run_twice(dev(many["states"]), many["maps"], many["tracks"], many["lines"], many["collided"])
    single = {}
    for s in U.MANY_CYCLE:
        at = pick.index(s)
        single[s] = run_twice(dev(many["states"][at][None]), [many["maps"][at]], [many["tracks"][at]],
                              [many["lines"][at]], [many["collided"][at]])
    want = {k: np.concatenate([single[s][k] for s in pick]) for k in got}
    hold_bit_equal("257 scenes x 1 vs the scenes alone", got, want)
    assert len({tuple(v[k][0] for k in U.KEYS) for v in single.values()}) == len(U.MANY_CYCLE)


def test_70_observation_times(gpu, golden):
    """T_obs = 70 (track_boxes_kernel's lanes take a second step): the moving scene's tracks, then 19 maps with a box
    on top of the ego. Nothing past map 49 is read: bit-equal to the 51-map run; only the cull boxes grow."""
    c = U.long_case(golden)
    states = dev(c["states"][None])
    base = run_twice(states, c["maps"], c["tracks"], c["lines"], c["collided"])
    got = run_twice(states, c["maps"], c["longer"], c["lines"], c["collided"])
    hold_bit_equal("70 observation times vs 51", got, base)
    assert (base["no_collision"] != 1.0).any() and (base["ttc"] != 1.0).any()
