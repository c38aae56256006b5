"""dd_proposals (and the chain up to pdm_closed) on the GPU against the reference's PDMGenerator.

The yardstick is the golden written by the reference's own generator (tests/golden/make_proposal_golden.py) and, for
the inputs built in this file, the numpy restatement (tests/pdm_proposal_ref.py) that test_proposals.py holds to the
same golden. Every case runs twice and must be bit-equal; lead_index is EQUAL everywhere; the continuous outputs are
held to the bars derived in test_proposals.py's docstring (the larger of the floor and 16 x float64-against-longdouble
of the restatement on the case, computed at run time). Every case prints its figures before asserting. Measured on an
MI355X: DESIGN.md section 18.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import pdm_area_ref as A
import pdm_collision_ref as R
import pdm_proposal_ref as Q
from test_proposals import golden_of, load

pytestmark = pytest.mark.gpu
OUT = Q.KEYS + ("lead_index",)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def pack(scenes):
    from diffusiondrive_amd import simulate as S
    paths = S.pack_paths([[q["xyh"] for q in s["paths"]] for s in scenes], "cuda")
    items = [Q.lead_items(s) for s in scenes]
    objects = S.pack_lead_objects([i[0] for i in items], "cuda", stop_polygons=[i[1] for i in items],
                                  collided=[s.get("collided", ()) for s in scenes])
    return paths, objects, dev(np.stack([s["ego"] for s in scenes])), np.stack([s["targets"] for s in scenes])


def run_twice(scenes, **kw):
    """generate_proposals twice over the scenes: bit-equal; numpy arrays with the scenes flattened."""
    from diffusiondrive_amd import simulate as S
    args = pack(scenes)
    a = S.generate_proposals(*args, details=True, **kw)
    b = S.generate_proposals(*args, details=True, **kw)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    n = a.proposals.shape[0] * a.proposals.shape[1]
    assert a.proposals.dtype == torch.float64 and a.lead_index.dtype == torch.int32
    return dict(proposals=a.proposals.cpu().numpy().reshape(n, Q.T, 3), idm=a.idm.cpu().numpy().reshape(n, Q.T, 2),
                lead=a.lead.cpu().numpy().reshape(n, Q.T, 3), lead_index=a.lead_index.cpu().numpy().reshape(n, Q.T))


def restated(scenes):
    ref = Q.generate_scenes(scenes)
    print(f"proposals margins: corridor steady {ref['corridor']}, ahead {ref['ahead']:.3e}, argmin {ref['argmin']:.3e}")
    assert ref["corridor"] and ref["ahead"] >= 1e-7 and ref["argmin"] >= 1e-7
    return ref, Q.bars(scenes, ref)[0]


def same(a, b):
    for k in OUT:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", ("origin", "far", "light", "crawl"))
def test_golden_scenes_against_the_reference(gpu, name):
    g = load()
    got = run_twice([g["scenes"][name]])
    Q.compare(f"device vs reference [{name}]", got, golden_of(g, name), g["bars"][name])


def test_golden_scenes_in_one_call_and_reversed(gpu):
    """Scene independence: the four scenes of one call give what four calls give; reversed scenes, reversed results."""
    g = load()
    names = list(g["scenes"])
    scenes = [g["scenes"][k] for k in names]
    together = run_twice(scenes)
    alone = [run_twice([s]) for s in scenes]
    same(together, {k: np.concatenate([a[k] for a in alone]) for k in OUT})
    back = run_twice(scenes[::-1])
    same(back, {k: np.concatenate([a[k] for a in alone[::-1]]) for k in OUT})
    bar = {k: max(g["bars"][n][k] for n in names) for k in Q.KEYS}
    Q.compare("device vs reference [four scenes]", together,
              {k: np.concatenate([g[f"{k}_{n}"] for n in names]) for k in OUT}, bar)


@pytest.mark.parametrize("case", Q.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(gpu, case):
    name, scene, expected = case
    got = run_twice([scene])
    ref, bar = restated([scene])
    Q.compare(name, got, ref, bar)
    Q.check_hand_case(name, got, {k: v for k, v in expected.items() if k != "fallback"}, scene)


def test_hand_cases_as_the_scenes_of_one_call(gpu):
    cases = [c for c in Q.hand_cases() if len(c[1]["targets"]) == 1]
    scenes = [c[1] for c in cases]
    got = run_twice(scenes)
    alone = [run_twice([s]) for s in scenes]
    same(got, {k: np.concatenate([a[k] for a in alone]) for k in OUT})


def crowd(count, at, t_obs=R.T_OBS, rings=()):
    """A straight path with ``count`` tracks: fillers far beside the road and, where count > 0, the decisive one (in
    the corridor, 30 m ahead) at list position ``at``."""
    xs = np.arange(0.0, 201.0, 10.0)
    tracks = [R.track(f"far_{i}", 30.0 + 7.0 * i, 300.0 + 3.0 * (i % 5), 0.1 * i, 4.0, 2.0, "VEHICLE", 1.0, t_obs=t_obs)
              for i in range(max(count - 1, 0))]
    if count:
        tracks.insert(at, R.track("decisive", 50.0 + 0.2 * np.arange(t_obs), 0.1, 0.05, 4.6, 1.9, "VEHICLE", 2.0,
                                  t_obs=t_obs))
    ego = np.zeros(11)
    ego[0], ego[R.VX] = 20.0, 6.0
    return dict(paths=[Q.straight_path(xs)], tracks=tracks, rings=list(rings), ego=ego,
                targets=np.array([4.0, 8.0, 12.0]), collided=[])


@pytest.mark.parametrize("count,at", [(0, 0), (1, 0), (63, 0), (63, 62), (64, 63), (65, 63), (65, 64), (129, 64),
                                      (129, 128)])
def test_track_counts_and_the_decisive_position(gpu, count, at):
    scene = crowd(count, at)
    got = run_twice([scene])
    ref, bar = restated([scene])
    Q.compare(f"{count} tracks, the decisive one at {at}", got, ref, bar)
    want = at if count else Q.FREE
    assert (got["lead_index"][:, 2] == want).all()


@pytest.mark.parametrize("vertices", (3, 4, 65))
def test_ring_sizes(gpu, vertices):
    ang = np.linspace(0.0, 2.0 * np.pi, vertices, endpoint=False) + 0.3
    ring = np.stack([70.0 + 3.0 * np.cos(ang), 0.4 + 3.0 * np.sin(ang)], axis=-1)
    scene = crowd(2, 1, rings=[ring])
    scene["tracks"][1] = R.track("behind_the_light", 95.0, 0.0, 0.0, 4.6, 1.9, "VEHICLE", 0.0)
    got = run_twice([scene])
    ref, bar = restated([scene])
    Q.compare(f"a ring of {vertices}", got, ref, bar)
    assert (got["lead_index"][:, 2] == 2).all()


@pytest.mark.parametrize("scenes,paths,policies", [(1, 1, 1), (3, 1, 3), (3, 3, 1), (65, 3, 5), (1, 3, 5)])
def test_scene_path_and_policy_counts(gpu, scenes, paths, policies):
    """G = 1, 3 and 65 scenes of P L = 1, 3 and 15 proposals: the golden scenes with their first paths and last
    policies, repeated with period 3 (scene i must equal scene i - 3 bit for bit)."""
    g = load()
    names = ("origin", "far", "light")
    made = []
    for i in range(scenes):
        s = dict(g["scenes"][names[i % 3]])
        s["paths"], s["targets"] = s["paths"][:paths], s["targets"][-policies:]
        made.append(s)
    got = run_twice(made)
    per = paths * policies
    assert got["proposals"].shape == (scenes * per, Q.T, 3)
    distinct = made[:3]
    if per == 15:
        ref = {k: np.concatenate([g["ref"][n][k] for n in names[:len(distinct)]]) for k in OUT}
        bar = {k: max(g["bars"][n][k] for n in names[:len(distinct)]) for k in Q.KEYS}
    else:
        ref, bar = restated(distinct)
    n = len(distinct) * per
    Q.compare(f"G = {scenes}, P = {paths}, L = {policies}", {k: v[:n] for k, v in got.items()}, ref, bar)
    for i in range(3, scenes):
        for k in OUT:
            assert np.array_equal(got[k][i * per:(i + 1) * per], got[k][(i - 3) * per:(i - 2) * per]), (i, k)


@pytest.mark.parametrize("t_obs", (50, 70))
def test_observation_lengths(gpu, t_obs):
    scene = crowd(3, 1, t_obs=t_obs)
    got = run_twice([scene])
    base = run_twice([crowd(3, 1)])
    same(got, base)


def test_cull_off_gives_the_same(gpu):
    g = load()
    scenes = [g["scenes"][k] for k in g["scenes"]]
    base = run_twice(scenes)
    os.environ["DDMI_PROPOSALS_CULL"] = "0"
    try:
        uncut = run_twice(scenes)
    finally:
        del os.environ["DDMI_PROPOSALS_CULL"]
    same(base, uncut)


def call_entry(lib, scene_args, **over):
    """dd_proposals directly; ``over`` replaces arguments or struct fields. Returns (rc, message)."""
    from diffusiondrive_amd import _lib, simulate as S
    paths, objects, ego, targets = scene_args
    k, rings = int(objects.heading.numel()), int(objects.ring_off.numel()) - 1
    pp = _lib.DDPaths(paths.verts.data_ptr(), paths.progress.data_ptr(), paths.path_off.data_ptr(),
                      paths.paths_per_scene, int(paths.progress.numel()))
    lo = _lib.DDLeadObjects(objects.boxes.data_ptr(), objects.valid.data_ptr(), objects.heading.data_ptr(),
                            objects.speed.data_ptr(), objects.scene_track_off.data_ptr(), k, int(objects.boxes.shape[1]),
                            objects.stop_verts.data_ptr(), objects.ring_off.data_ptr(),
                            objects.scene_ring_off.data_ptr(), rings)
    ip, ap = S.default_idm_params(lib), S.default_area_params(lib)
    host = np.ascontiguousarray(targets)
    scenes, policies = host.shape
    for name, value in over.items():
        for struct in (pp, lo, ip, ap):
            if name in dict(struct._fields_):
                setattr(struct, name, value)
    size = lib.dd_proposals_work(scenes, paths.paths_per_scene, k, rings)
    n = scenes * paths.paths_per_scene * policies
    keep = call_entry.keep = dict(work=torch.empty(size, dtype=torch.float64, device="cuda"),
                                  out=torch.full((n, Q.T, 3), -7.0, dtype=torch.float64, device="cuda"),
                                  targets=dev(host))
    a = dict(paths=ctypes.byref(pp), objects=ctypes.byref(lo), ego=ego.data_ptr(), targets=keep["targets"].data_ptr(),
             targets_host=host.ctypes.data, G=scenes, L=policies, ip=ctypes.byref(ip), ap=ctypes.byref(ap),
             work=keep["work"].data_ptr(), size=size, out=keep["out"].data_ptr())
    a.update({k_: v for k_, v in over.items() if k_ in a})
    rc = lib.dd_proposals(a["paths"], a["objects"], a["ego"], a["targets"], a["targets_host"], a["G"], a["L"], a["ip"],
                          a["ap"], a["work"], a["size"], a["out"], None, None, None,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, (lib.dd_last_error() or b"").decode(), keep["out"]


def test_rejections_launch_nothing(gpu):
    from diffusiondrive_amd import simulate as S
    lib = gpu
    g = load()
    scene = g["scenes"]["origin"]
    args = pack([scene])
    rc, msg, out = call_entry(lib, args)
    assert rc == 0 and not bool((out == -7.0).any()), msg
    bad_target = args[3].copy()
    bad_target[0, 2] = -1.0
    nan_target = args[3].copy()
    nan_target[0, 0] = np.nan
    cases = [(dict(paths=None), "paths is null"), (dict(objects=None), "objects is null"), (dict(ego=None), "ego_states"),
             (dict(targets=None), "targets is null"), (dict(ip=None), "idm_params"), (dict(ap=None), "area_params"),
             (dict(work=None), "work is null"), (dict(out=None), "out_proposals"), (dict(G=0), "G = 0"),
             (dict(L=0), "L = 0"), (dict(L=65), "L = 65"), (dict(paths_per_scene=0), "paths_per_scene"),
             (dict(verts=None), "dd_paths.verts"), (dict(progress=None), "dd_paths.progress"),
             (dict(path_off=None), "dd_paths.path_off"), (dict(num_verts=5), "num_verts"),
             (dict(boxes=None), "dd_lead_objects.boxes"), (dict(speed=None), "dd_lead_objects.speed"),
             (dict(scene_track_off=None), "scene_track_off"), (dict(scene_ring_off=None), "scene_ring_off"),
             (dict(stop_verts=None), "stop_verts"), (dict(ring_off=None), "dd_lead_objects.ring_off"),
             (dict(num_times=40), "num_times"), (dict(num_tracks=-1), "num_tracks"), (dict(num_rings=-1), "num_rings"),
             (dict(dt=0.0), "dd_idm_params.dt"), (dict(accel_max=float("nan")), "accel_max"),
             (dict(decel_max=-3.0), "decel_max"), (dict(headway_time=float("inf")), "headway_time"),
             (dict(min_gap_to_lead_agent=0.0), "min_gap_to_lead_agent"), (dict(acceleration_exponent=0), "exponent"),
             (dict(leading_agent_update_rate=0), "update_rate"), (dict(leading_agent_update_rate=41), "update_rate"),
             (dict(corridor_poses=0), "corridor_poses"), (dict(half_width=0.0), "half_width"),
             (dict(half_length=float("nan")), "half_length"), (dict(size=3), "work_doubles")]
    for over, text in cases:
        rc, msg, out = call_entry(lib, args, **over)
        assert rc == -1 and text in msg, (over, rc, msg)
        assert bool((out == -7.0).all()), over
    for bad in (bad_target, nan_target):
        rc, msg, out = call_entry(lib, args[:3] + (bad,))
        assert rc == -1 and "targets[0, " in msg and bool((out == -7.0).all()), msg
        with pytest.raises(ValueError, match="targets"):
            S.generate_proposals(*args[:3], bad)
    with pytest.raises(ValueError, match="unknown IDM parameter"):
        S.generate_proposals(*args, params=dict(gap=1.0))
    with pytest.raises(ValueError, match="dd_idm_params.dt"):
        S.generate_proposals(*args, params=dict(dt=-0.1))
    with pytest.raises(ValueError, match="paths holds"):
        S.generate_proposals(args[0], args[1], torch.cat([args[2], args[2]]), np.concatenate([args[3], args[3]]))
    rc = lib.dd_pdm_select(None, None, None, None, None, 4, 2, None, None, None, None)
    assert rc == -1 and b"score is null" in lib.dd_last_error()


def test_non_default_parameters(gpu):
    g = load()
    scene = g["scenes"]["origin"]
    over = dict(min_gap_to_lead_agent=2.0, headway_time=1.0, accel_max=2.0, decel_max=4.0, acceleration_exponent=4,
                leading_agent_update_rate=5, corridor_poses=30)
    got = run_twice([scene], params=over)
    p = Q.idm_params(**over)
    ref = Q.generate_scenes([scene], p)
    assert ref["corridor"] and ref["ahead"] >= 1e-7 and ref["argmin"] >= 1e-7
    Q.compare("non-default parameters", got, ref, Q.bars([scene], ref, p)[0])
    assert (got["idm"] != run_twice([scene])["idm"]).any()


def test_pdm_closed_chain(gpu):
    """generate -> simulate -> pdm_score -> the first maximum, against the same chain over the restatement's
    proposals: simulate_proposals (held to its own golden elsewhere) on them, pdm_collision_ref on those states."""
    from diffusiondrive_amd import simulate as S
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    import types
    g = load()
    names = ("origin", "far", "light")
    # without the vehicle that cuts in a few metres ahead: every proposal runs into it and every score would be 0
    scenes = [dict(g["scenes"][k], tracks=[t for t in g["scenes"][k]["tracks"] if not t["token"].startswith("cut_")])
              for k in names]
    maps, lines, tracks, collided = [], [], [], []
    for i, s in enumerate(scenes):
        items = A.seeded_map(int(g["seed"]) + i, tuple(s["ego"][:3]), lanes=3)[0]
        maps.append(items), lines.append(s["paths"][0]["xyh"][:, :2])
        tracks.append(s["tracks"]), collided.append(s["collided"])
    paths, objects, ego, targets = pack(scenes)
    obs = S.pack_observations([R.track_items(t) for t in tracks], "cuda", collided=collided)
    a = S.pdm_closed(paths, objects, ego, targets, maps, obs, lines)
    b = S.pdm_closed(paths, objects, ego, targets, maps, obs, lines)
    torch.cuda.synchronize()
    assert torch.equal(a.best_index, b.best_index) and torch.equal(bits(a.progress_reference), bits(b.progress_reference))
    assert torch.equal(bits(a.best_states), bits(b.best_states)) and torch.equal(bits(a.scores.score), bits(b.scores.score))
    assert a.scores.score.shape == (3, 15) and a.best_states.shape == (3, Q.T, 11) and a.best_index.dtype == torch.int32
    ref, _ = restated(scenes)
    states = S.simulate_proposals(dev(ref["proposals"]), ego, per_group=15).cpu().numpy().reshape(3, 15, Q.T, 11)
    score = a.scores.score.cpu().numpy()
    for i in range(3):
        want = R.pdm_score(states[i], maps[i], tracks[i], lines[i], collided=collided[i])
        bar = R.score_bars(want, R.raw_progress_bar(states[i], lines[i]))[1]
        gap = float(np.abs(score[i] - want["score"]).max())
        best = int(np.argmax(want["score"]))
        top = np.sort(want["score"])[::-1]
        print(f"pdm_closed [{names[i]}]: score within {gap:.3e} (bar {float(np.max(bar)):.3e}), best {best}, margin "
              f"{top[0] - top[1]:.3e}")
        assert (np.abs(score[i] - want["score"]) <= bar).all()
        mine = int(a.best_index[i])
        assert want["score"][mine] == top[0] or top[0] - want["score"][mine] <= 2 * float(np.max(bar))
        if top[0] - top[1] > 2 * float(np.max(bar)) or top[0] == top[1]:
            assert mine == best
        multi = want["no_collision"] * want["drivable_area"]
        assert abs(float(a.progress_reference[i]) - want["raw_progress"][mine] * multi[mine]) \
            <= R.raw_progress_bar(states[i], lines[i])
        assert torch.equal(bits(a.best_states[i]), bits(a.states[i, mine]))
    picks = a.best_index.cpu().numpy()
    assert len(set(picks.tolist())) > 1 and (score.max(1) > score.min(1) + 1e-3).all(), (picks, score)
    again = S.pdm_score(a.states, maps, obs, lines, progress_reference=a.progress_reference)
    assert again.score.shape == (3, 15)
    me = types.SimpleNamespace(_transfuser_model=types.SimpleNamespace(device=torch.cuda.current_device()))
    via = DiffusionDriveAgent.pdm_closed_reference(me, paths, objects, ego, targets, maps, obs, lines)
    assert torch.equal(bits(via.progress_reference), bits(a.progress_reference))
