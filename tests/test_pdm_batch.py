"""The builders of tests/pdm_batch_util.py held to their conditions, on the CPU: every case that
tests/test_pdm_batch_gpu.py runs at batch structure - a group past one workgroup, dd_progress past one block,
more polygons than one listing pass, track counts across the chunk of 64, 257 scenes, 70 observation times - must, on
the reference side, notice the fault it is built for: a maximum taken over too few indices, a neighbour scene's
reference value, line, map or tracks, a polygon or a track past a chunk that is never read. No device is needed, and
no kernel is run wrong on purpose: "would this test notice" is answered here.

One condition is held in a narrower form than it was first put. A maximum without the last stride step was to move
the progress term of 90 % of a group's candidates; the golden sets cannot give that, since 72 % of the moving set's
candidates (87 % of the standing set's) have a product raw * no_collision * drivable_area of 0 and their term is 0
under every maximum. Held instead: it moves the term of at least 90 % of the candidates with a non-zero product (it
moves all of them), and the share over all candidates is printed.
"""
import numpy as np
import pytest

import pdm_area_ref as A
import pdm_batch_util as U
import pdm_collision_ref as R
from test_collisions import load


@pytest.fixture(scope="module")
def golden():
    return load()


@pytest.fixture(scope="module")
def ragged(golden):
    return U.ragged_case(golden)


@pytest.mark.parametrize("names,per_group,second_in", [(("moving",), 600, (256, 512)),
                                                        (("moving", "standing", "global"), 257, (64, 256))])
def test_group_rows_put_the_maximum_past_the_first_steps(golden, names, per_group, second_in):
    g = golden
    states, rows, scenes, figures = U.group_case(g, names, per_group, 3, second_in)
    print(f"pdm batch groups of {per_group}: {figures}")
    assert states.shape == (len(names), per_group, 41, 11)
    last = per_group - 1
    # 599 is the third stride step of aggregate_kernel, wavefront 1; 256 the second step of a group of 257
    assert (last // U.BLOCK, last % U.BLOCK // U.WAVE) == ((2, 1) if per_group == 600 else (1, 0))
    assert -(-per_group // 4) == (150 if per_group == 600 else 65)       # workgroups per scene of the other kernels
    for k, n in enumerate(names):
        p = U.product(g, n)
        assert np.array_equal(states[k], g[f"states_{n}"][rows[k]])
        if p.max() > 0.0:
            order = np.argsort(p, kind="stable")
            assert np.flatnonzero(rows[k] == order[-1]).tolist() == [last]
            at = np.flatnonzero(rows[k] == order[-2]).tolist()
            assert len(at) == 1 and second_in[0] <= at[0] < second_in[1]
            assert p[order[-1]] > p[order[-2]] > p[order[-3]]
            f = figures[k]
            assert f["cut_hi_of_nonzero"] >= 0.9 and f["cut_lo_of_nonzero"] >= 0.9, f
            assert f["cut_hi"] > 0.1 and f["cut_lo"] > 0.1, f
            # the two cuts give different maxima: each step of the stride is needed
            assert p[rows[k][:second_in[0]]].max() < p[rows[k][:second_in[1]]].max() < p.max()


@pytest.mark.parametrize("per_group", U.AGG_GROUPS)
def test_aggregate_inputs_realise_their_roles(per_group):
    c = U.aggregate_case(per_group, 100 + per_group)
    fig = U.aggregate_conditions(c)
    print(f"pdm batch aggregate inputs, per_group {per_group}: {fig}")
    assert set(np.unique(c["no_collision"]).tolist()) <= {0.0, 0.5, 1.0}
    assert set(np.unique(c["driving_direction"]).tolist()) <= {0.0, 0.5, 1.0}
    assert set(np.unique(c["drivable_area"]).tolist()) <= {0.0, 1.0} and set(np.unique(c["ttc"]).tolist()) <= {0.0, 1.0}
    raw = c["raw_progress"][np.isfinite(c["raw_progress"])]
    assert raw.min() >= 0.0 and raw.max() <= 61.0
    group = U.aggregate_ref(c)
    assert (group["pmax"][3] == 5.0).all() and np.isnan(group["pmax"][4]).all() and (group["score"][5] == 0.0).all()
    if per_group > 1:       # both values of the second branch, and the pair rule differs from the group's
        assert set(group["progress"][3].tolist()) == {0.0, 1.0} and fig["group_vs_pair"] > 0.25


def test_progress_case_holds_its_conditions(golden):
    c = U.progress_case(int(golden["seed"]))
    fig = U.progress_conditions(c)
    print(f"pdm batch progress: {fig['tied']} exact ties on the hairpin; share moved by more than 1 m on a neighbour's "
          f"line {fig['wrong_scene']}; non-tie share per scene {fig['non_tie'].mean(1).round(2).tolist()}")
    n = U.PROGRESS_SCENES * U.PROGRESS_GROUP
    assert n == 525 and -(-n // U.BLOCK) == 3
    assert any(b % U.PROGRESS_GROUP for b in range(U.BLOCK, n, U.BLOCK))      # scene boundaries inside blocks
    # the dense sampling agrees with the restatement on the candidates it will be asked about
    for g in range(U.PROGRESS_SCENES):
        want, bound = U.independent_progress(c, g)
        assert (np.abs(fig["own"][g] - want)[fig["non_tie"][g]] <= bound).all(), g


def test_polygon_case_fills_more_than_one_listing_pass(golden):
    c = U.area_case(golden, int(golden["seed"]))
    fig = U.area_conditions(c)
    print(f"pdm batch polygons: kept per workgroup {fig['kept']}, per pass {fig['per_pass']}; smallest distance to an "
          f"edge {fig['edge']:.3e} m, of m to a threshold {fig['m']:.3e}; share of flags the fillers change "
          f"{fig['changed']}")
    ref, margins, parts = U.restated(c["states"], c["maps"], c["tracks"], c["lines"], c["collided"])
    U.hold_margins("polygons", margins)
    ix = [sum(it[1] == "INTERSECTION" for it in m) for m in c["maps"]]
    assert ix == [3, 0, 0]


def test_hand_batch_keeps_every_case(golden):
    cases, states = U.hand_batch()
    assert len(cases) == len(R.hand_cases()) - 1 and states.shape == (len(cases), 3, 41, 11)
    for s, (name, c, _) in enumerate(cases):
        n = c["states"].shape[0]
        alone = R.pdm_score(c["states"], c["items"], c["tracks"], c["line"], collided=c["collided"])
        padded = R.pdm_score(states[s], c["items"], c["tracks"], c["line"], collided=c["collided"])
        for k in U.KEYS:
            assert np.array_equal(padded[k][:n], alone[k], equal_nan=True), (name, k)
            assert np.array_equal(padded[k][n:], np.repeat(alone[k][:1], 3 - n), equal_nan=True), (name, k)
    ix = [sum(it[1] == "INTERSECTION" for it in c["items"]) for _, c, _ in cases]
    tracks = [len(c["tracks"]) for _, c, _ in cases]
    polys = [len(c["items"]) for _, c, _ in cases]
    at = [s for s, (name, _, _) in enumerate(cases) if name == "ttc_axle_in_intersection"][0]
    assert ix[at] == 1 and at > 0 and sum(ix[:at]) == 0 and len(set(polys)) > 1 and len(set(tracks)) > 2
    assert ix[at + 1] == 0 and ix[at + 2] == 1        # and the next intersection case sits behind another count


def test_ragged_scenes_hold_their_conditions(ragged):
    ref, fig = U.ragged_conditions(ragged)
    print(f"pdm batch ragged scenes: {fig}")
    assert ragged["states"].shape == (12, U.RAGGED_GROUP, 41, 11)
    assert fig["changed_by_tracks_alone"] >= 6
    assert set(ref["no_collision"].tolist()) == {0.0, 0.5, 1.0} and set(ref["ttc"].tolist()) == {0.0, 1.0}


def test_many_scenes_and_long_observations(golden, ragged):
    pick, many = U.many_case(ragged)
    assert len(pick) == U.MANY_SCENES == 257 and many["states"].shape == (257, 1, 41, 11)
    counts = [U.TRACK_COUNTS[s] for s in U.MANY_CYCLE]
    assert len(set(U.MANY_CYCLE)) == 5 and 0 in counts and len(set(counts)) == 5
    single = [R.pdm_score(ragged["states"][s][:1], ragged["maps"][s], ragged["near"][s], ragged["lines"][s])
              for s in U.MANY_CYCLE]
    assert len({tuple(float(q[k][0]) for k in U.KEYS) for q in single}) == 5     # five different answers
    c = U.long_case(golden)
    t = c["longer"][0][0]
    assert t["boxes"].shape == (U.LONG_T_OBS, 4, 2) and t["valid"][R.T_OBS:].all()
    # read as 51 maps the longer tracks are the golden's: nothing past map 49 may matter
    cut = [dict(tr, boxes=tr["boxes"][:R.T_OBS], valid=tr["valid"][:R.T_OBS]) for tr in c["longer"][0]]
    a = R.pdm_score(c["states"], c["maps"][0], cut, c["lines"][0], collided=c["collided"][0])
    b = R.pdm_score(c["states"], c["maps"][0], c["tracks"][0], c["lines"][0], collided=c["collided"][0])
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in U.KEYS)
    assert A.T + 9 <= R.T_OBS < U.WAVE < U.LONG_T_OBS      # past one stride of the track boxes' lanes
