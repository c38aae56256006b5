"""dd_ego_areas on the GPU against the reference's PDMScorer.

The yardstick is the golden written by the reference's own pdm_scorer module (tests/golden/make_area_golden.py) and,
where the input exists only on the device or only in this file (the chained cases, the star polygon, the two-scene
cases), the numpy restatement (tests/pdm_area_ref.py) that test_ego_areas.py holds to the same goldens. No candidate is
excluded.

Bars (derived, not tuned; every case prints its figures before asserting):
  flags and scores  EQUAL. Every golden point is at least 1e-6 m from every edge and every finite m at least 1e-6 from
                    both thresholds, so any correct float64 predicate agrees; the cases built here print and assert
                    their own margin (at least 1e-7 m, two hundred times the spacing of a coordinate at 4.0e6 m).
  coords            per value 2 spacing(|ref|) + 16 2^-52 (half_length + half_width + rear_axle_to_center): two
                    roundings at the coordinate's magnitude and a few ulp of device sin / cos error on the lever arms.
  m                 44 spacing(max |coordinate|) + 1e-12: eleven steps, each a difference of two centers that may each
                    sit one rounding off; the summation order of the window is free.
  share cap         at most half of the coord values may differ from the reference's at all, so that the allowance
                    cannot hide a systematic error.
Measured on an MI355X: DESIGN.md section 16.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import pdm_area_ref as R
from test_ego_areas import ALT_ROWS, SIM_SETS, call_ego_areas, compare, compare_to, hold, load, rejection_cases

pytestmark = pytest.mark.gpu

MARGIN = 1e-7


@pytest.fixture(scope="module")
def golden():
    return load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_twice(states, maps, params=None, stream=None):
    """ego_areas with coords, twice: the two runs must be bit-equal (NaNs at the same places), and a run without
    coords must give the same. Returns numpy arrays with the scene dimension flattened away."""
    from diffusiondrive_amd.simulate import ego_areas
    a = ego_areas(states, maps, params, coords=True, stream=stream)
    b = ego_areas(states, maps, params, coords=True, stream=stream)
    c = ego_areas(states, maps, params, stream=stream)
    torch.cuda.synchronize()
    assert a.areas.dtype == torch.bool and a.coords.dtype == torch.float64 and c.coords is None
    lead = tuple(states.shape[:-2])
    assert a.areas.shape == lead + (41, 3) and a.coords.shape == lead + (41, 5, 2)
    assert a.drivable_area.shape == a.driving_direction.shape == a.oncoming_progress.shape == lead
    for other in (b, c):
        assert torch.equal(a.areas, other.areas)
        for k in ("drivable_area", "driving_direction", "oncoming_progress"):
            assert torch.equal(getattr(a, k).view(torch.int64), getattr(other, k).view(torch.int64)), k
    assert torch.equal(a.coords.view(torch.int64), b.coords.view(torch.int64))
    n = int(np.prod(lead))
    return dict(areas=a.areas.cpu().numpy().reshape(n, 41, 3), drivable_area=a.drivable_area.cpu().numpy().reshape(n),
                driving_direction=a.driving_direction.cpu().numpy().reshape(n),
                m=a.oncoming_progress.cpu().numpy().reshape(n), coords=a.coords.cpu().numpy().reshape(n, 41, 5, 2))


def flat(ref):
    """ego_areas_grouped's (G, n, ...) results with the two leading dimensions merged."""
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in ref.items()}


def margin_of(tag, maps, ref):
    """The smallest distance of any point to any edge of its scene, and of any finite m to a threshold."""
    edge = min([R.edge_distance(items, pts) for items, pts in zip(maps, ref["coords"])] + [np.inf])
    f = ref["m"][np.isfinite(ref["m"])]
    mm = float(np.abs(f[:, None] - np.array([2.0, 6.0])).min()) if f.size else np.inf
    print(f"ego areas {tag}: smallest distance to an edge {edge:.3e} m, of m to a threshold {mm:.3e}")
    return min(edge, mm)


@pytest.mark.parametrize("name", SIM_SETS + ("synth",))
def test_golden_sets_against_the_reference(gpu, golden, name):
    """The three simulator sets (the global one at 6.6e5 / 4.0e6 m) and the synthetic set at N = 96, each run twice."""
    g = golden
    got = run_twice(dev(g[f"states_{name}"][None]), [g[f"map_{name}"][0]])
    hold(compare("device vs reference", got, g, name))


def test_duck_typed_map_gives_the_same(gpu, golden):
    """The same set through a duck-typed PDMDrivableMap with route ids (a roadblock's token among them)."""
    from diffusiondrive_amd.simulate import ego_areas
    from test_ego_areas import duck_map
    g = golden
    items, tokens, ids = g["map_synth"]
    states = dev(g["states_synth"][None])
    a, b = ego_areas(states, [items]), ego_areas(states, [(duck_map(items, tokens), ids)])
    assert torch.equal(a.areas, b.areas) and torch.equal(a.drivable_area, b.drivable_area)
    assert torch.equal(a.driving_direction, b.driving_direction)
    assert torch.equal(a.oncoming_progress, b.oncoming_progress)


def test_one_candidate(gpu, golden):
    """N = 1 (three spare wavefronts), through the C entry: the outputs sit inside larger sentinel-filled buffers
    that must stay untouched past the first candidate."""
    from diffusiondrive_amd import _lib, simulate as S
    lib, g = gpu, golden
    row = 40
    states = dev(g["states_synth"][row:row + 1])
    maps = S.pack_drivable_maps([g["map_synth"][0]], "cuda")
    areas = torch.full((4, 41, 3), 9, dtype=torch.uint8, device="cuda")
    scores = torch.full((4, 2), -7.0, dtype=torch.float64, device="cuda")
    progress = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    coords = torch.full((4, 41, 5, 2), -7.0, dtype=torch.float64, device="cuda")
    P = int(maps.poly_kind.numel())
    work = torch.empty(lib.dd_ego_areas_work(P), dtype=torch.float64, device="cuda")
    m = _lib.DDDrivableMaps(*[t.data_ptr() for t in maps], P)
    rc = lib.dd_ego_areas(states.data_ptr(), 1, 1, ctypes.byref(m), 1, ctypes.byref(S.default_area_params(lib)),
                          work.data_ptr(), areas.data_ptr(), scores.data_ptr(), progress.data_ptr(),
                          coords.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.dd_last_error()
    assert bool((areas[1:] == 9).all()) and bool((scores[1:] == -7.0).all()) and bool((progress[1:] == -7.0).all())
    assert bool((coords[1:] == -7.0).all())
    got = dict(areas=areas[:1].cpu().numpy().astype(bool), drivable_area=scores[:1, 0].cpu().numpy(),
               driving_direction=scores[:1, 1].cpu().numpy(), m=progress[:1].cpu().numpy(),
               coords=coords[:1].cpu().numpy())
    ref = {k: g[f"{k}_synth"][row:row + 1] for k in ("areas", "drivable_area", "driving_direction", "m")}
    ref["coords"] = R.coords(g["states_synth"][row:row + 1])   # row 40 is not among the stored coords
    hold(compare_to("N = 1", got, ref))


def test_two_scenes_with_their_own_maps(gpu, golden):
    """N = 10, per_group = 5 (a full workgroup and a quarter per scene): scene 0 on the synthetic set's map, scene 1 on
    another seed's. Each candidate must be scored on its own scene's map: swapping the maps changes the answer."""
    g = golden
    states = g["states_synth"][[3, 17, 29, 41, 56, 60, 71, 77, 83, 95]].reshape(2, 5, 41, 11)
    maps = [g["map_synth"][0], R.seeded_map(int(g["seed"]) + 50, (2.0, -1.5, 0.4), lanes=2)[0]]
    ref = flat(R.ego_areas_grouped(states, maps))
    assert margin_of("two scenes", maps, R.ego_areas_grouped(states, maps)) >= MARGIN
    got = run_twice(dev(states), maps)
    hold(compare_to("two scenes", got, ref))
    swapped = run_twice(dev(states), maps[::-1])
    ref_swapped = flat(R.ego_areas_grouped(states, maps[::-1]))
    assert margin_of("two scenes, swapped", maps[::-1], R.ego_areas_grouped(states, maps[::-1])) >= MARGIN
    hold(compare_to("two scenes, maps swapped", swapped, ref_swapped))
    assert (swapped["areas"][:5] != got["areas"][:5]).any() and (swapped["areas"][5:] != got["areas"][5:]).any()


def test_empty_scene_beside_a_full_one(gpu, golden):
    """A scene with zero polygons first, then one with polygons, then another empty one: the empty scenes' states are
    all non-drivable and oncoming and never in multiple lanes; the full one's answers are the golden's."""
    g = golden
    rows = np.arange(0, 18)
    states = g["states_synth"][rows].reshape(3, 6, 41, 11)
    maps = [[], g["map_synth"][0], []]
    got = run_twice(dev(states), maps)
    ref = flat(R.ego_areas_grouped(states, maps))
    hold(compare_to("empty scenes beside a full one", got, ref))
    assert np.array_equal(got["areas"][6:12], g["areas_synth"][6:12])
    for part in (got["areas"][:6], got["areas"][12:]):
        assert not part[..., R.MULTIPLE_LANES].any() and part[..., R.NON_DRIVABLE].all() and part[..., R.ONCOMING].all()
    assert (got["drivable_area"][:6] == 0.0).all()
    # every scene empty: the map arrays are empty tensors
    only = run_twice(dev(states[:1]), [[]])
    hold(compare_to("an empty map", only, flat(R.ego_areas_grouped(states[:1], [[]]))))


def test_ring_longer_than_a_chunk(gpu, golden):
    """One ring of 40 000 vertices (a seeded star, far longer than the vertex chunk a workgroup stages), as a roadblock
    under an on-route lane, 8 candidates: the crossing parity is carried across the chunks."""
    g = golden
    star = R.star_polygon(int(g["seed"]))
    states = g["states_synth"][[0, 9, 18, 27, 36, 45, 54, 63]][None]
    maps = [[([star], "ROADBLOCK", False), ([R.rect(-20.0, -2.0, 40.0, 2.5)], "LANE", True)]]
    ref = flat(R.ego_areas_grouped(states, maps))
    # the margin with torch on the device: 1 640 points against 40 000 edges, a candidate at a time
    a = dev(star)
    ab = torch.roll(a, -1, 0) - a
    edge = np.inf
    for pts in ref["coords"]:
        q = dev(pts.reshape(-1, 1, 2))
        s = (((q - a) * ab).sum(-1) / (ab * ab).sum(-1)).clamp(0.0, 1.0)
        edge = min(edge, float((q - (a + s[..., None] * ab)).norm(dim=-1).min()))
    f = ref["m"][np.isfinite(ref["m"])]
    print(f"ego areas star: smallest distance to an edge {edge:.3e} m, of m to a threshold "
          f"{np.abs(f[:, None] - np.array([2.0, 6.0])).min():.3e}; inside share {1 - ref['areas'][..., 1].mean():.3f}")
    assert edge >= 1e-9 and np.abs(f[:, None] - np.array([2.0, 6.0])).min() >= MARGIN
    assert 0.1 < ref["areas"][..., R.NON_DRIVABLE].mean() < 0.9
    got = run_twice(dev(states), maps)
    hold(compare_to("star of 40 000 vertices", got, ref))


def test_polygons_that_miss_every_box(gpu, golden):
    """A map whose polygons all lie far from every point: every polygon is culled, the answers are the empty map's."""
    g = golden
    states = g["states_synth"][:8][None]
    far = [[(list(R.to_frame(r, (5000.0, -3000.0, 0.3)) for r in rings), layer, on) for rings, layer, on in
            g["map_synth"][0]]]
    got = run_twice(dev(states), far)
    ref = flat(R.ego_areas_grouped(states, far))
    hold(compare_to("polygons that miss every box", got, ref))
    assert not got["areas"][..., R.MULTIPLE_LANES].any() and got["areas"][..., 1:].all()


def test_nan_row(gpu, golden):
    """One NaN pose: that state is in no polygon, the NaN step reaches m, the driving-direction score falls through to
    0; among ordinary rows it changes nothing."""
    g = golden
    got = run_twice(dev(g["states_nan"][None]), [g["map_nan"][0]])
    print(f"ego areas [nan]: m {got['m']}, scores {got['drivable_area']} {got['driving_direction']}")
    hold(compare("device vs reference", got, g, "nan"))
    assert np.isnan(got["m"]).all() and (got["driving_direction"] == 0.0).all()
    mixed = np.concatenate([g["states_synth"][:3], g["states_nan"], g["states_synth"][3:6]])[None]
    got = run_twice(dev(mixed), [g["map_synth"][0]])
    assert np.array_equal(np.delete(got["areas"], 3, 0), g["areas_synth"][:6])
    assert np.array_equal(got["areas"][3], g["areas_nan"][0])
    assert np.array_equal(np.delete(got["driving_direction"], 3), g["driving_direction_synth"][:6])


def test_non_default_parameters(gpu, golden):
    """Other vehicle lengths, dt = 0.125, horizon 0.5 (a window of five samples) and thresholds 1 / 3."""
    g = golden
    got = run_twice(dev(g["states_alt"][None]), [g["map_alt"][0]], {k: g["alt"][k] for k in R.ALT})
    hold(compare("device vs reference", got, g, "alt"))
    assert (got["areas"] != g["areas_synth"][:ALT_ROWS]).any(axis=(0, 1)).all()   # the lengths reach every flag
    assert (got["m"] != g["m_synth"][:ALT_ROWS]).any()                            # and dt the window


@pytest.mark.parametrize("name", SIM_SETS)
def test_chained_to_the_simulator_on_the_device(gpu, golden, name):
    """ego_areas(simulate_proposals(golden proposals)): the device's states are within 1e-11 of the golden's, the
    golden's points at least 1e-6 m from every edge, so the flags and scores are the reference's on the golden
    states; coords and m are held against the restatement on the device's own states."""
    from diffusiondrive_amd.simulate import simulate_proposals
    from test_simulate import load as load_sim
    g, sim = golden, load_sim(name)
    states = simulate_proposals(dev(sim["proposals"]), dev(sim["ego_states"]))
    host = states.cpu().numpy()
    gap = np.abs(np.delete(host, R.HEADING, -1) - np.delete(sim["states"], R.HEADING, -1)).max()
    print(f"ego areas chained [{name}]: device states within {gap:.3e} of the golden's")
    assert gap <= 1e-11
    got = run_twice(states[None], [g[f"map_{name}"][0]])
    hold(compare_to(f"chained [{name}]", got, R.ego_areas(host, g[f"map_{name}"][0])))
    for k in ("areas", "drivable_area", "driving_direction"):
        assert np.array_equal(got[k], g[f"{k}_{name}"]), k


def test_planner_samples_to_ego_areas(gpu, gpu_model, golden):
    """forward_samples at B = 2, S = 3 -> simulate_trajectories -> ego_areas on seeded maps laid around the two start
    poses: (2, 3, 20, ...), read in place, against the restatement on the device's states."""
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    from diffusiondrive_amd.simulate import ego_areas, pack_drivable_maps, simulate_trajectories
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(2, 31)
    feats = {k: dev(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}
    noise = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 20, 8, 2)).astype(np.float32)).cuda()
    poses = gpu_model.forward_samples(feats, 3, noise=noise, modes=True)["poses_reg"]
    ego = np.array([[0.0, 0.0, 0.0, 4.0, 0.0, 0.2, 0.0, 0.01, 0.0, 0.013, 0.0],
                    [664431.37, 3997675.12, np.pi - 0.05, 6.0, 0.0, -0.3, 0.0, -0.02, 0.01, -0.04, 0.0]])
    states = simulate_trajectories(poses, dev(ego))
    assert states.shape == (2, 3, 20, 41, 11)
    seed = int(golden["seed"])
    maps = [R.seeded_map(seed + 20 + b, tuple(ego[b, :3]), lanes=3 - b)[0] for b in range(2)]
    host = states.cpu().numpy().reshape(2, 60, 41, 11)
    grouped = R.ego_areas_grouped(host, maps)
    assert margin_of("planner samples", maps, grouped) >= MARGIN
    got = run_twice(states, maps)
    hold(compare_to("planner samples", got, flat(grouped)))
    packed = pack_drivable_maps(maps, states.device)
    me = types.SimpleNamespace(_transfuser_model=gpu_model)
    via = DiffusionDriveAgent.ego_areas(me, states, packed)
    direct = ego_areas(states, packed)
    assert via.areas.shape == (2, 3, 20, 41, 3) and via.drivable_area.shape == (2, 3, 20)
    assert torch.equal(via.areas, direct.areas) and torch.equal(via.areas.cpu().reshape(120, 41, 3),
                                                                torch.from_numpy(got["areas"]))
    via_host = DiffusionDriveAgent.ego_areas(me, states.cpu(), packed)
    assert via_host.areas.is_cuda and torch.equal(via_host.areas, via.areas)


def test_non_default_stream(gpu, golden):
    """The call and its outputs on a stream of the caller's: the same bits as on the current stream."""
    g = golden
    states, maps = dev(g["states_synth"][None]), [g["map_synth"][0]]
    base = run_twice(states, maps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = run_twice(states, maps, stream=side)
    side.synchronize()
    for k in base:
        assert np.array_equal(base[k], got[k], equal_nan=True), k


def test_rejections_launch_nothing(gpu, golden):
    """Every bad argument returns DD_ERR_INVALID with the argument or field named, and the outputs keep their
    sentinels; the Python surface raises ValueError."""
    from diffusiondrive_amd import simulate as S
    lib, g = gpu, golden
    states = dev(g["states_synth"])
    maps = S.pack_drivable_maps([g["map_synth"][0]], "cuda")
    out = torch.full((96 * 41 * 3,), -7.0, dtype=torch.float64, device="cuda")
    work = torch.empty(lib.dd_ego_areas_work(int(maps.poly_kind.numel())), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for kw, text in rejection_cases():
        rc, msg = call_ego_areas(lib, states.data_ptr(), maps.verts.data_ptr(), work.data_ptr(), out.data_ptr(),
                                 stream=st, **kw)
        assert rc == -1 and msg.startswith("dd_ego_areas: ") and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    one = states[None]
    for over, text in ((dict(dt=0.0), "dd_area_params.dt"),
                       (dict(half_width=float("nan")), "dd_area_params.half_width"),
                       (dict(driving_direction_horizon=5.0), "int\\(horizon / dt\\)"),
                       (dict(driving_direction_compliance_threshold=7.0), "is above"),
                       (dict(wheel_base=3.0), "unknown area parameter")):
        with pytest.raises(ValueError, match=text):
            S.ego_areas(one, maps, over)
    with pytest.raises(ValueError, match="float64"):
        S.ego_areas(one.float(), maps)
    with pytest.raises(ValueError, match="41, 11"):
        S.ego_areas(one[:, :, :40], maps)
    with pytest.raises(ValueError, match="device tensor"):
        S.ego_areas(one.cpu(), maps)
    with pytest.raises(ValueError, match="1 scenes for 96"):
        S.ego_areas(states[:, None], maps)
    with pytest.raises(ValueError, match="maps.verts"):
        S.ego_areas(one, S.pack_drivable_maps([g["map_synth"][0]], "cpu"))
    # what is documented as accepted: a horizon of 0 (a window of one sample), equal thresholds, optional outputs
    for over in (dict(driving_direction_horizon=0.0), dict(driving_direction_horizon=-0.05),
                 dict(driving_direction_compliance_threshold=6.0), dict(driving_direction_horizon=4.0)):
        r = S.ego_areas(one, maps, over)
        assert r.areas.shape == (1, 96, 41, 3)
    torch.cuda.synchronize()
