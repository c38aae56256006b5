"""dd_simulate / dd_simulate_proposals on the GPU against the reference's PDMSimulator.

The yardstick is the golden written by the reference's own simulator (tests/golden/make_sim_golden.py: 96 kinematic,
stationary, creeping and reversing candidates from a moving, a standing and a global-coordinate start), and for
dd_simulate - whose proposal interpolation the goldens cannot hold, nuPlan's InterpolatedTrajectory being unavailable
offline - the float64 restatement (tests/pdm_sim_ref.py) that test_simulate.py holds to the same goldens. No candidate is
excluded; the heading is compared modulo 2 pi.

Bars: see BAR_EGO / BAR_GLOBAL below. Every case prints its measured figure before asserting.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import pdm_sim_ref as R
from test_simulate import NAMES, load

pytestmark = pytest.mark.gpu

# Largest state difference to the goldens measured on an MI355X, times a margin of 10 for device libm differences in
# sin / cos / tan / atan2 fed through the 40-step feedback loop, and in any case at most CAP (anything looser is a wrong
# branch or wrong arithmetic, not rounding). Measured against the goldens: 9.308e-13 over the ego-frame sets (x of the
# standing start), 4.476e-13 over the global set (the velocity; its x / y, whose ulp at 4e6 m is 4.7e-10, were
# bit-equal). The CPU restatement's own gap to the same goldens is 9.2e-13 / 4.5e-13 (test_simulate.py). Every other
# case here measured below these two figures.
CAP = 1e-7
BAR_EGO = 10 * 9.308e-13
BAR_GLOBAL = 10 * 4.476e-13
assert 0 < BAR_EGO <= CAP and 0 < BAR_GLOBAL <= CAP


def bar_of(name):
    return BAR_GLOBAL if name == "global" else BAR_EGO


@pytest.fixture(scope="module")
def goldens():
    """The three golden files, and the restatement's simulation of their 8-pose inputs (computed once)."""
    g = {name: load(name) for name in NAMES}
    for name, rec in g.items():
        rec["restated"] = R.simulate_trajectories(rec["trajectory"], rec["ego_states"])
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def report(tag, got, ref, bar):
    err = R.state_error(got.cpu().numpy(), ref)
    print(f"simulate {tag}: largest state difference {err:.3e} (bar {bar:.1e})")
    return err


@pytest.mark.parametrize("name", NAMES)
def test_proposals_against_the_reference(gpu, goldens, name):
    """dd_simulate_proposals on the golden's proposals (N = 96, one start state: per_group = 96), twice."""
    from diffusiondrive_amd.simulate import simulate_proposals
    g = goldens[name]
    prop, ego = dev(g["proposals"]), dev(g["ego_states"])
    out = simulate_proposals(prop, ego)
    again = simulate_proposals(prop, ego)
    torch.cuda.synchronize()
    assert out.shape == (96, 41, 11) and out.dtype == torch.float64
    assert torch.equal(out, again)
    assert report(f"proposals [{name}]", out, g["states"], bar_of(name)) <= bar_of(name)
    h = out[..., R.HEADING]
    assert bool((h >= -np.pi).all()) and bool((h < np.pi).all())


@pytest.mark.parametrize("name", NAMES)
def test_trajectories_against_the_restatement(gpu, goldens, name):
    """dd_simulate on the golden's float32 planner poses: the proposal built on the device, then the simulation."""
    from diffusiondrive_amd.simulate import simulate_trajectories
    g = goldens[name]
    traj, ego = dev(g["trajectory"][None]), dev(g["ego_states"])  # (1, 96, 8, 3): one scene of 96 candidates
    out = simulate_trajectories(traj, ego)
    again = simulate_trajectories(traj, ego)
    torch.cuda.synchronize()
    assert out.shape == (1, 96, 41, 11)
    assert torch.equal(out, again)
    assert report(f"trajectories [{name}]", out[0], g["restated"], bar_of(name)) <= bar_of(name)
    # and so against the reference itself
    assert report(f"trajectories vs reference [{name}]", out[0], g["states"], bar_of(name)) <= bar_of(name)


def test_one_candidate(gpu, goldens):
    """N = 1 (a single, mostly spare workgroup in every kernel), each kind of plan: a kinematic one, a stationary one,
    a reversing one."""
    from diffusiondrive_amd.simulate import simulate_proposals, simulate_trajectories
    g = goldens["moving"]
    for i in (0, 72, 95):
        out = simulate_proposals(dev(g["proposals"][i:i + 1]), dev(g["ego_states"]))
        assert report(f"N=1 candidate {i}", out, g["states"][i:i + 1], BAR_EGO) <= BAR_EGO
        out = simulate_trajectories(dev(g["trajectory"][i:i + 1]), dev(g["ego_states"]))
        assert report(f"N=1 candidate {i} from poses", out, g["restated"][i:i + 1], BAR_EGO) <= BAR_EGO


@pytest.mark.parametrize("per_group,n", [(1, 96), (20, 60), (96, 288)])
def test_groups_read_their_own_start_state(gpu, goldens, per_group, n):
    """Candidate c starts from ego_states[c / per_group]: groups cycle through the three start states (moving,
    standing, global), so a wrong divisor reads another start. Group k takes candidates [k * per_group, (k + 1) *
    per_group) of golden file k % 3; the proposals are that file's, the expected states too."""
    from diffusiondrive_amd.simulate import simulate_proposals, simulate_trajectories
    order = ["moving", "standing", "global"]
    idx = np.arange(n)
    grp = idx // per_group
    cand = idx % 96
    pick = lambda key: np.stack([goldens[order[k % 3]][key][c] for k, c in zip(grp, cand)])  # noqa: E731
    ego = np.stack([goldens[order[k % 3]]["ego_states"][0] for k in range(n // per_group)])
    bars = np.array([bar_of(order[k % 3]) for k in grp])
    glob = np.array([order[k % 3] == "global" for k in grp])
    for tag, out, ref in (
            ("proposals", simulate_proposals(dev(pick("proposals")), dev(ego), per_group=per_group), pick("states")),
            ("poses", simulate_trajectories(dev(pick("trajectory")).view(n // per_group, per_group, 8, 3), dev(ego))
             .view(n, 41, 11), pick("restated"))):
        got = out.cpu().numpy()
        errs = np.array([R.state_error(got[i], ref[i]) for i in range(n)])
        print(f"simulate per_group={per_group} N={n} {tag}: ego-frame {errs[~glob].max():.3e} "
              f"global {errs[glob].max():.3e}")
        assert (errs <= bars).all(), (tag, errs.max())


def test_forward_samples_poses_are_read_in_place(gpu, gpu_model):
    """B = 2, S = 3: forward_samples' poses_reg (2, 3, 20, 8, 3) straight into the simulator (N = 120, 60 candidates
    per scene), against the restatement on the same tensor; scene 1 starts at global coordinates."""
    from diffusiondrive_amd.simulate import simulate_trajectories
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(2, 31)
    feats = {k: dev(inp[k]) for k in ("camera_feature", "lidar_feature", "status_feature")}
    noise = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 20, 8, 2)).astype(np.float32)).cuda()
    poses = gpu_model.forward_samples(feats, 3, noise=noise, modes=True)["poses_reg"]
    assert poses.shape == (2, 3, 20, 8, 3) and poses.is_cuda
    ego = np.array([[0.0, 0.0, 0.0, 4.0, 0.0, 0.2, 0.0, 0.01, 0.0, 0.013, 0.0],
                    [664431.37, 3997675.12, np.pi - 0.05, 6.0, 0.0, -0.3, 0.0, -0.02, 0.01, -0.04, 0.0]])
    out = simulate_trajectories(poses, dev(ego))
    again = simulate_trajectories(poses, dev(ego))
    torch.cuda.synchronize()
    assert out.shape == (2, 3, 20, 41, 11)
    assert torch.equal(out, again)
    ref = R.simulate_trajectories(poses.cpu().numpy().reshape(120, 8, 3), ego).reshape(2, 3, 20, 41, 11)
    assert report("forward_samples scene 0 (ego frame)", out[0], ref[0], BAR_EGO) <= BAR_EGO
    assert report("forward_samples scene 1 (global)", out[1], ref[1], BAR_GLOBAL) <= BAR_GLOBAL
    # the agent's method is the same call, on a forward's output dict or a tensor, host tensors moved to the device
    from diffusiondrive_amd.agent import DiffusionDriveAgent
    me = types.SimpleNamespace(_transfuser_model=gpu_model)
    via = DiffusionDriveAgent.simulate_trajectories(me, {"poses_reg": poses.cpu()}, torch.from_numpy(ego),
                                                    key="poses_reg")
    assert torch.equal(via, out)


def test_params_reach_the_kernels(gpu, goldens):
    """A non-default parameter set (horizon 4, other gains, time constants and wheel base) against the restatement
    with the same set; the defaults are the reference's."""
    from diffusiondrive_amd import simulate as S
    p = S.default_params()
    for k, v in R.DEFAULTS.items():
        assert (tuple(getattr(p, k)) if k == "q_lat" else getattr(p, k)) == v, k
    over = dict(tracking_horizon=4, wheel_base=2.7, q_lon=4.0, r_lon=0.5, q_lat=(2.0, 5.0, 0.1), r_lat=0.7,
                jerk_penalty=3e-4, curvature_rate_penalty=2e-2, stopping_gain=0.8, stopping_velocity=0.35,
                max_steering_angle=0.4, accel_time_constant=0.3, steering_time_constant=0.1)
    g = goldens["moving"]
    ref = R.simulate_proposals(g["proposals"], g["ego_states"], p=R.params(**over))
    assert R.state_error(ref, g["states"]) > 1e-3  # the set matters
    out = S.simulate_proposals(dev(g["proposals"]), dev(g["ego_states"]), params=over)
    assert report("non-default parameters", out, ref, BAR_EGO) <= BAR_EGO


def test_rejections_launch_nothing(gpu, goldens):
    """Every bad argument returns DD_ERR_INVALID with the argument or field named, and the output keeps its sentinel."""
    from diffusiondrive_amd import simulate as S
    lib = gpu
    g = goldens["moving"]
    prop, traj, ego = dev(g["proposals"]), dev(g["trajectory"]), dev(g["ego_states"])
    out = torch.full((96, 41, 11), -7.0, dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.dd_simulate_work(96), dtype=torch.float64, device="cuda")
    assert lib.dd_simulate_work(96) >= 96 * (41 * 3 + 80) and lib.dd_simulate_work(0) == 0
    st = torch.cuda.current_stream().cuda_stream

    def call(n=96, per_group=96, p=None, prop_=prop, ego_=ego, work_=work, out_=out, null_params=False, poses=None,
             traj_=traj):
        p = p or S.default_params(lib)
        pp = None if null_params else ctypes.byref(p)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        if poses is None:
            rc = lib.dd_simulate_proposals(ptr(prop_), ptr(ego_), n, per_group, pp, ptr(work_), ptr(out_), st)
        else:
            rc = lib.dd_simulate(ptr(traj_), poses, ptr(ego_), n, per_group, pp, ptr(work_), ptr(out_), st)
        return rc, lib.dd_last_error().decode()

    def params(**kw):
        p = S.default_params(lib)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = [
        (dict(n=0), "N = 0"), (dict(n=-3), "N = -3"), (dict(per_group=0), "per_group = 0"),
        (dict(per_group=-1), "per_group = -1"), (dict(per_group=20), "not a multiple of per_group = 20"),
        (dict(prop_=None), "proposals is null"), (dict(ego_=None), "ego_states is null"),
        (dict(work_=None), "work is null"), (dict(out_=None), "out_states is null"),
        (dict(null_params=True), "params is null"),
        (dict(poses=8, traj_=None), "traj is null"), (dict(poses=6), "num_poses = 6"), (dict(poses=40), "num_poses = 40"),
        (dict(p=params(dt=0.0)), "dd_sim_params.dt"), (dict(p=params(dt=-0.1)), "dd_sim_params.dt"),
        (dict(p=params(jerk_penalty=0.0)), "dd_sim_params.jerk_penalty"),
        (dict(p=params(curvature_rate_penalty=-1.0)), "dd_sim_params.curvature_rate_penalty"),
        (dict(p=params(initial_curvature_penalty=0.0)), "dd_sim_params.initial_curvature_penalty"),
        (dict(p=params(tracking_horizon=0)), "dd_sim_params.tracking_horizon"),
        (dict(p=params(tracking_horizon=1)), "dd_sim_params.tracking_horizon"),
        (dict(p=params(tracking_horizon=41)), "dd_sim_params.tracking_horizon"),
        (dict(p=params(tracking_horizon=-2)), "dd_sim_params.tracking_horizon"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # the Python surface raises ValueError carrying dd_last_error()'s text
    with pytest.raises(ValueError, match="tracking_horizon = 41"):
        S.simulate_proposals(prop, ego, params=dict(tracking_horizon=41))
    with pytest.raises(ValueError, match="not a multiple of per_group = 20"):
        S.simulate_proposals(prop, dev(np.repeat(g["ego_states"], 4, 0)), per_group=20)
    with pytest.raises(ValueError, match="num_poses = 6"):
        S.simulate_trajectories(traj[:, :6].contiguous(), ego.expand(96, 11))
    with pytest.raises(ValueError, match="float64"):
        S.simulate_trajectories(traj, ego.float())
    # the horizon's limits themselves are accepted
    for h in (2, 40):
        rc, msg = call(p=params(tracking_horizon=h))
        assert rc == 0, (h, msg)
    torch.cuda.synchronize()
