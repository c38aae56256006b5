"""dd_collisions, dd_progress, dd_pdm_aggregate and the chained pdm_score on the GPU against the reference's PDMScorer.

The yardstick is the golden written by the reference's own pdm_scorer module (tests/golden/make_collision_golden.py)
and, where the input exists only on the device or only in this file (the chained cases, the two-scene cases, the hand
cases), the numpy restatement (tests/pdm_collision_ref.py) that test_collisions.py holds to the same golden. No
candidate is excluded.

Bars (derived in test_collisions.py's docstring, not tuned; every case prints its figures before asserting):
  no_collision, ttc, drivable_area, driving_direction, the comfort term and both time indices: EQUAL. The golden keeps
  every separating-axis gap and rear-axle point 1e-6 m, every speed 1e-6 m/s, every used angle 1e-9 rad and every
  comfort signal 1e-5 from what decides it; the cases built here print and assert their own margins (at least 1e-7).
  raw progress: pdm_collision_ref.raw_progress_bar (four roundings at the largest coordinate, sin / cos on the lever
  arm, the parameter's products, one rounding per summed segment; twice). progress term and score:
  pdm_collision_ref.score_bars (the raw bound through p / pmax and the weights, plus 4 ulp of 1).
  share cap: at most half of the continuous values may differ from the reference's at all.
Measured on an MI355X: DESIGN.md section 17.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import pdm_area_ref as A
import pdm_collision_ref as R
from test_collisions import (ALT_ROWS, SIM_SETS, bar_of, check_hand_case, compare_to, golden_ref, hold, load,
                             params_of)

pytestmark = pytest.mark.gpu

MARGIN = 1e-7
KEYS = ("no_collision", "drivable_area", "driving_direction", "progress", "ttc", "collision_time_idx", "ttc_time_idx",
        "raw_progress", "score")


@pytest.fixture(scope="module")
def golden():
    return load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def run_twice(states, maps, tracks, lines, collided=None, area=None, score=None, reference=None):
    """pdm_score twice: the two runs must be bit-equal. ``tracks``: per scene the track dicts (packed here from the
    list form). Returns numpy arrays with the leading dimensions flattened."""
    from diffusiondrive_amd import simulate as S
    obs = S.pack_observations([R.track_items(t) for t in tracks], "cuda", collided=collided)
    kw = dict(area_params=area, score_params=score,
              progress_reference=None if reference is None else dev(np.asarray(reference, dtype=np.float64)))
    a = S.pdm_score(states, maps, obs, lines, **kw)
    b = S.pdm_score(states, maps, obs, lines, **kw)
    torch.cuda.synchronize()
    lead = tuple(states.shape[:-2])
    for k in KEYS:
        assert getattr(a, k).shape == lead and getattr(a, k).dtype == torch.float64, k
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert a.comfort.shape == lead + (6,) and a.comfort.dtype == torch.bool and torch.equal(a.comfort, b.comfort)
    n = int(np.prod(lead))
    out = {k: getattr(a, k).cpu().numpy().reshape(n) for k in KEYS}
    out["comfort"] = a.comfort.cpu().numpy().reshape(n, 6)
    return out


def scene_args(scene):
    items, _, _, _, tracks, collided, line = scene
    return [items], [tracks], [line], [collided]


def restated(states, maps, tracks, lines, collided, **kw):
    """The restatement over (G, n, 41, 11) host states, the scenes flattened, with its margins printed."""
    parts = [R.pdm_score(states[g], maps[g], tracks[g], lines[g], collided=collided[g], **kw) for g in range(len(maps))]
    ref = {k: np.concatenate([q[k] for q in parts]) for k in KEYS + ("comfort", "pmax")}
    ref["comfortable"] = ref["comfort"].all(-1).astype(np.float64)
    margins = {k: min(q[k] for q in parts) for k in ("gap_margin", "speed_margin", "angle_margin")}
    axle = min([A.edge_distance([it for it in maps[g] if it[1] == "INTERSECTION"], q["axle_points"])
                for g, q in enumerate(parts) if len(q["axle_points"])] + [np.inf])
    return ref, dict(margins, axle_margin=axle)


def hold_margins(tag, m):
    print(f"pdm score {tag}: margins {m}")
    assert m["gap_margin"] >= MARGIN and m["speed_margin"] >= MARGIN and m["axle_margin"] >= MARGIN
    assert m["angle_margin"] >= 1e-9


@pytest.mark.parametrize("name", SIM_SETS + ("synth", "nan"))
def test_golden_sets_against_the_reference(gpu, golden, name):
    """The three simulator sets (the global one at 6.6e5 / 4.0e6 m), the synthetic set and the NaN row, each twice."""
    g = golden
    maps, tracks, lines, collided = scene_args(g[f"scene_{name}"])
    got = run_twice(dev(g[f"states_{name}"][None]), maps, tracks, lines, collided)
    hold(compare_to(f"device vs reference [{name}]", got, golden_ref(g, name), bar_of(g, name)))


def test_non_default_parameters(gpu, golden):
    g = golden
    ap, sp = params_of(g, "alt")
    maps, tracks, lines, collided = scene_args(g["scene_alt"])
    states = dev(g["states_alt"][None])
    got = run_twice(states, maps, tracks, lines, collided, area=ap, score=sp)
    hold(compare_to("device vs reference [alt]", got, golden_ref(g, "alt"), bar_of(g, "alt"), sp))
    plain = run_twice(states, maps, tracks, lines, collided)
    assert (plain["score"] != got["score"]).any()


def test_pair_normalisation(gpu, golden):
    """Group against pair: with candidate 0's raw * multi as progress_reference every candidate scores as the pair
    [candidate 0, candidate] does in the reference."""
    g = golden
    maps, tracks, lines, collided = scene_args(g["scene_moving"])
    states = dev(g["states_moving"][None])
    got = run_twice(states, maps, tracks, lines, collided, reference=[float(g["pair_reference"])])
    with np.errstate(invalid="ignore"):
        pmax = np.maximum(float(g["pair_reference"]), g["raw_progress_moving"] * g["no_collision_moving"]
                          * g["drivable_area_moving"])
    ref = dict(golden_ref(g, "moving"), score=g["score_pair"], progress=g["progress_pair"], pmax=pmax)
    hold(compare_to("device pairs vs reference [moving]", got, ref, bar_of(g, "moving")))
    group = run_twice(states, maps, tracks, lines, collided)
    assert (group["score"] != got["score"]).any()


def test_cull_off_gives_the_same(gpu, golden):
    """DDMI_COLLISIONS_CULL=0 (read at every call): every quad against every track, bit-equal results."""
    g = golden
    for name in ("moving", "global"):
        maps, tracks, lines, collided = scene_args(g[f"scene_{name}"])
        states = dev(g[f"states_{name}"][None])
        base = run_twice(states, maps, tracks, lines, collided)
        os.environ["DDMI_COLLISIONS_CULL"] = "0"
        try:
            uncut = run_twice(states, maps, tracks, lines, collided)
        finally:
            del os.environ["DDMI_COLLISIONS_CULL"]
        for k in base:
            assert np.array_equal(base[k], uncut[k], equal_nan=True), (name, k)


def test_one_candidate(gpu, golden):
    """N = 1 (three spare wavefronts) through the three C entries, into sentinel-filled oversize buffers."""
    from diffusiondrive_amd import _lib, simulate as S
    lib, g = gpu, golden
    row = 40
    items, _, _, _, tracks, collided, line = g["scene_moving"]
    host = g["states_moving"][row:row + 1]
    states = dev(host)
    ego = S.ego_areas(states[None], [items])
    comfort = S.comfort_metrics(states)
    obs = S.pack_observations([R.track_items(tracks)], "cuda", collided=[collided])
    ix = S.pack_drivable_maps([items], "cuda", layers=("INTERSECTION",))
    lines = S.pack_centerlines([line], "cuda")
    out = torch.full((7, 4), -7.0, dtype=torch.float64, device="cuda")
    k = int(obs.heading.numel())
    work = torch.empty(lib.dd_collisions_work(k), dtype=torch.float64, device="cuda")
    o = _lib.DDObservations(*[t.data_ptr() for t in obs[:5]], k, int(obs.boxes.shape[1]))
    m = _lib.DDDrivableMaps(*[t.data_ptr() for t in ix], int(ix.poly_kind.numel()))
    c = _lib.DDCenterlines(lines.verts.data_ptr(), lines.scene_off.data_ptr(), int(lines.verts.shape[0]))
    ap, sp = S.default_area_params(lib), S.default_score_params(lib)
    st = torch.cuda.current_stream().cuda_stream
    areas = ego.areas.contiguous().view(torch.uint8)
    rc = lib.dd_collisions(states.data_ptr(), areas.data_ptr(), 1, 1, ctypes.byref(o), ctypes.byref(m), 1,
                           ctypes.byref(ap), ctypes.byref(sp), work.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                           out[2].data_ptr(), out[3].data_ptr(), st)
    assert rc == 0, lib.dd_last_error()
    rc = lib.dd_progress(states.data_ptr(), 1, 1, ctypes.byref(c), 1, ctypes.byref(ap), out[4].data_ptr(), st)
    assert rc == 0, lib.dd_last_error()
    dac, ddc = ego.drivable_area.contiguous().view(-1), ego.driving_direction.contiguous().view(-1)
    rc = lib.dd_pdm_aggregate(out[0].data_ptr(), dac.data_ptr(), ddc.data_ptr(), out[4].data_ptr(), out[2].data_ptr(),
                              comfort.contiguous().view(torch.uint8).data_ptr(), 1, 1, ctypes.byref(sp), None,
                              out[5].data_ptr(), out[6].data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0, lib.dd_last_error()
    assert bool((out[:, 1:] == -7.0).all())
    h = out[:, 0].cpu().numpy()
    got = dict(no_collision=h[0:1], collision_time_idx=h[1:2], ttc=h[2:3], ttc_time_idx=h[3:4], raw_progress=h[4:5],
               score=h[5:6], progress=h[6:7], drivable_area=dac.cpu().numpy(), driving_direction=ddc.cpu().numpy(),
               comfort=comfort.cpu().numpy())
    ref, margins = restated(host[None], [items], [tracks], [line], [collided])
    hold(compare_to("N = 1", got, ref, R.raw_progress_bar(host, line)))
    for key in ("no_collision", "ttc", "collision_time_idx", "ttc_time_idx"):
        assert got[key][0] == g[f"{key}_moving"][row], key


def test_two_scenes_track_chunk_and_times(gpu, golden):
    """Two scenes x 5 candidates with different track counts, the scenes swapped, one scene with no tracks and no
    INTERSECTION polygon, a scene of 65 tracks (one above the chunk of 64 a wavefront culls at a time) and
    observations of 50 against 51 maps."""
    g = golden
    rows = [3, 17, 40, 58, 91]
    states = np.stack([g["states_moving"][rows], g["states_standing"][rows]])
    scenes = [g["scene_moving"], g["scene_standing"]]
    maps, lines = [s[0] for s in scenes], [s[6] for s in scenes]
    tracks, collided = [scenes[0][4], scenes[1][4][:4]], [scenes[0][5], []]
    got = run_twice(dev(states), maps, tracks, lines, collided)
    ref, margins = restated(states, maps, tracks, lines, collided)
    hold_margins("two scenes", margins)
    hold(compare_to("two scenes", got, ref, max(bar_of(g, "moving"), bar_of(g, "standing"))))
    assert (ref["no_collision"][:5] != 1.0).any() or (ref["ttc"][:5] != 1.0).any()
    # no tracks and no INTERSECTION polygon in the second scene
    bare = [it for it in maps[1] if it[1] != "INTERSECTION"]
    got = run_twice(dev(states), [maps[0], bare], [tracks[0], []], lines, collided)
    ref, margins = restated(states, [maps[0], bare], [tracks[0], []], lines, collided)
    hold(compare_to("a scene without tracks", got, ref, max(bar_of(g, "moving"), bar_of(g, "standing"))))
    assert (got["no_collision"][5:] == 1.0).all() and (got["ttc"][5:] == 1.0).all()
    assert np.isinf(got["collision_time_idx"][5:]).all() and np.isinf(got["ttc_time_idx"][5:]).all()
    # 65 tracks: 58 far ones in front of the seven that count, so that the last sits alone in the second chunk
    real = R.drop_tokens(scenes[0][4], scenes[0][5])
    far = [R.track(f"far_{i}", 500.0 + 10.0 * i, 300.0, 0.1 * i, 4.0, 2.0, "VEHICLE", 0.0) for i in range(65 - len(real))]
    many = far + real
    assert len(many) == 65
    got = run_twice(dev(states[:1]), maps[:1], [many], lines[:1])
    base = run_twice(dev(states[:1]), maps[:1], [real], lines[:1])
    for k in base:
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    last_only = run_twice(dev(states[:1]), maps[:1], [far + real[-1:]], lines[:1])
    alone = run_twice(dev(states[:1]), maps[:1], [real[-1:]], lines[:1])
    for k in alone:
        assert np.array_equal(last_only[k], alone[k], equal_nan=True), k
    # T_obs = 50: the last map dropped (TTC reads up to 49)
    short = [dict(tr, boxes=tr["boxes"][:50], valid=tr["valid"][:50]) for tr in real]
    got50 = run_twice(dev(states[:1]), maps[:1], [short], lines[:1])
    for k in base:
        assert np.array_equal(got50[k], base[k], equal_nan=True), k


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(gpu, case):
    name, c, expected = case
    n = c["states"].shape[0]
    got = run_twice(dev(c["states"][None]), [c["items"]], [c["tracks"]], [c["line"]], [c["collided"]],
                    reference=None if c["reference"] is None else [c["reference"]])
    ref = R.pdm_score(c["states"], c["items"], c["tracks"], c["line"], reference=c["reference"], collided=c["collided"])
    out = {k: v.reshape(n) for k, v in got.items() if k != "comfort"}
    out["types"], out["ttc_hits"] = ref["types"], ref["ttc_hits"]   # the device does not report these
    check_hand_case(name, out, {k: v for k, v in expected.items()})
    for k in ("no_collision", "ttc", "collision_time_idx", "ttc_time_idx", "drivable_area"):
        assert np.array_equal(out[k], ref[k]), (name, k)


@pytest.mark.parametrize("name", SIM_SETS)
def test_chained_to_the_simulator_on_the_device(gpu, golden, name):
    """pdm_score(simulate_proposals(golden proposals)): the device's states are within 1e-11 of the golden's and the
    golden's margins are 1e-6, so the discrete results are the reference's on the golden states; the continuous ones
    are held against the restatement on the device's own states."""
    from diffusiondrive_amd.simulate import simulate_proposals
    from test_simulate import load as load_sim
    g, sim = golden, load_sim(name)
    states = simulate_proposals(dev(sim["proposals"]), dev(sim["ego_states"]))
    host = states.cpu().numpy()
    gap = np.abs(np.delete(host, A.HEADING, -1) - np.delete(sim["states"], A.HEADING, -1)).max()
    print(f"pdm score chained [{name}]: device states within {gap:.3e} of the golden's")
    assert gap <= 1e-11
    maps, tracks, lines, collided = scene_args(g[f"scene_{name}"])
    got = run_twice(states[None], maps, tracks, lines, collided)
    ref, margins = restated(host[None], maps, tracks, lines, collided)
    hold_margins(f"chained [{name}]", margins)
    hold(compare_to(f"chained [{name}]", got, ref, R.raw_progress_bar(host, lines[0])))
    for k in ("no_collision", "ttc", "collision_time_idx", "ttc_time_idx", "drivable_area", "driving_direction"):
        assert np.array_equal(got[k], g[f"{k}_{name}"]), k


def test_planner_samples_to_pdm_score(gpu, gpu_model, golden):
    """forward_samples at B = 2, S = 3 -> simulate_trajectories -> pdm_score (120 candidates) on seeded scenes laid
    around the two start poses and the device's own paths, against the restatement on the device's states; its own
    margins printed and asserted."""
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    from diffusiondrive_amd import simulate as S
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(2, 31)
    feats = {k: dev(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}
    noise = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 20, 8, 2)).astype(np.float32)).cuda()
    poses = gpu_model.forward_samples(feats, 3, noise=noise, modes=True)["poses_reg"]
    ego = np.array([[0.0, 0.0, 0.0, 4.0, 0.0, 0.2, 0.0, 0.01, 0.0, 0.013, 0.0],
                    [664431.37, 3997675.12, np.pi - 0.05, 6.0, 0.0, -0.3, 0.0, -0.02, 0.01, -0.04, 0.0]])
    states = S.simulate_trajectories(poses, dev(ego))
    assert states.shape == (2, 3, 20, 41, 11)
    host = states.cpu().numpy().reshape(2, 60, 41, 11)
    seed = int(golden["seed"])
    scenes = [R.seeded_scene(seed + 20 + b, host[b], lanes=3 - b) for b in range(2)]
    maps, lines = [s[0] for s in scenes], [s[6] for s in scenes]
    tracks, collided = [s[4] for s in scenes], [s[5] for s in scenes]
    ref, margins = restated(host, maps, tracks, lines, collided)
    hold_margins("planner samples", margins)
    got = run_twice(states, maps, tracks, lines, collided)
    bar = max(R.raw_progress_bar(host[b], lines[b]) for b in range(2))
    hold(compare_to("planner samples", got, ref, bar))
    obs = S.pack_observations([R.duck_observation(t, c) for t, c in zip(tracks, collided)], states.device)
    me = types.SimpleNamespace(_transfuser_model=gpu_model)
    via = DiffusionDriveAgent.pdm_score(me, states, maps, obs, lines)
    assert via.score.shape == (2, 3, 20) and via.comfort.shape == (2, 3, 20, 6)
    assert np.array_equal(via.score.cpu().numpy().reshape(120), got["score"], equal_nan=True)
    via_host = DiffusionDriveAgent.pdm_score(me, states.cpu(), maps, obs, lines)
    assert via_host.score.is_cuda and torch.equal(bits(via_host.score), bits(via.score))
    me.simulate_trajectories = types.MethodType(DiffusionDriveAgent.simulate_trajectories, me)
    from_poses = DiffusionDriveAgent.pdm_score(me, {"poses_reg": poses}, maps, obs, lines, ego_states=dev(ego),
                                               key="poses_reg")
    assert torch.equal(bits(from_poses.score), bits(via.score))


def test_rejections_launch_nothing(gpu, golden):
    """A bad argument returns DD_ERR_INVALID with the field named and the outputs keep their sentinels; the Python
    surface raises ValueError."""
    from diffusiondrive_amd import simulate as S
    from test_collisions import (aggregate_rejection_cases, call_aggregate, call_collisions, call_progress,
                                 collisions_rejection_cases, progress_rejection_cases)
    lib, g = gpu, golden
    buf = torch.full((96 * 41 * 11,), -7.0, dtype=torch.float64, device="cuda")
    for call, cases in ((call_collisions, collisions_rejection_cases()), (call_progress, progress_rejection_cases()),
                        (call_aggregate, aggregate_rejection_cases())):
        for kw, text in cases:
            rc, msg = call(lib, buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **kw)
            assert rc == -1 and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    items, _, _, _, tracks, collided, line = g["scene_moving"]
    one = dev(g["states_moving"][None, :4])
    args = ([items], [R.track_items(tracks)], [line])
    with pytest.raises(ValueError, match="dd_score_params.ttc_weight"):
        S.pdm_score(one, *args, score_params=dict(ttc_weight=-1.0))
    with pytest.raises(ValueError, match="unknown score parameter"):
        S.pdm_score(one, *args, score_params=dict(weight=1.0))
    with pytest.raises(ValueError, match="dd_area_params.half_width"):
        S.pdm_score(one, *args, area_params=dict(half_width=float("nan")))
    with pytest.raises(ValueError, match="states must be"):
        S.pdm_score(one.float(), *args)
    with pytest.raises(ValueError, match="hold 2 scenes"):
        S.pdm_score(one, [items], [R.track_items(tracks), []], [line])
    with pytest.raises(ValueError, match="centerlines holds 2 scenes"):
        S.pdm_score(one, [items], [R.track_items(tracks)], [line, line])
    with pytest.raises(ValueError, match="INTERSECTION polygons on their own"):
        S.pdm_score(one, S.pack_drivable_maps([items], "cuda"), [R.track_items(tracks)], [line])
