"""float64 numpy restatement of NAVSIM's PDM proposal simulation (the truth of dd_simulate / dd_simulate_proposals).

Restates, batched over N candidates:

* the proposal: ``transform_trajectory`` + ``get_trajectory_as_array`` (pdm_score.py:24-80) on the exact 0.1 s grid -
  knot 0 the ego rear-axle pose, knots 1..8 ``ego o pose_k``, x / y linear between knots at weights j / 5, heading
  unwrapped along the knots (np.unwrap) then linear (nuPlan's InterpolatedTrajectory is not available offline; the
  reference's truncation of absolute timestamps to whole microseconds moves a sample by <= 1 us);
* the tracker's profile fits (batch_lqr_utils.py:59-249), with the regularisation matrix R built exactly as
  ``_make_banded_difference_matrix`` builds it (:59-70: the second slice assignment overwrites the first's +1s);
* the 40 closed-loop steps: BatchLQRTracker.track_trajectory (batch_lqr.py:134-464) and
  BatchKinematicBicycleModel.propagate_state (batch_kinematic_bicycle.py:76-185), driven as
  PDMSimulator.simulate_proposals drives them (pdm_simulator.py:32-79).

The normal equations are solved with np.linalg.solve where the reference multiplies by torch.linalg.pinv: both
matrices are symmetric positive definite (the regularisers are), so the two agree to rounding; tests/test_simulate.py
holds this file to goldens written by the reference's own PDMSimulator.
"""
import numpy as np

STATES = 11
X, Y, HEADING, VX, VY, AX, AY, STEER, STEER_RATE, ANG_VEL, ANG_ACC = range(STATES)
NUM_POSES = 8          # planner output: 8 poses at 0.5 s
SUB = 5                # 0.1 s samples per 0.5 s knot interval
M = NUM_POSES * SUB    # 40 displacements / simulation steps
T = M + 1              # 41 states

DEFAULTS = dict(
    wheel_base=3.089, dt=0.1, tracking_horizon=10, q_lon=10.0, r_lon=1.0, q_lat=(1.0, 10.0, 0.0), r_lat=1.0,
    jerk_penalty=1e-4, curvature_rate_penalty=1e-2, initial_curvature_penalty=1e-10, stopping_gain=0.5,
    stopping_velocity=0.2, max_steering_angle=np.pi / 3, accel_time_constant=0.2, steering_time_constant=0.05)


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def normalize_angle(a):
    return np.arctan2(np.sin(a), np.cos(a))


def principal_value(a):
    """nuPlan's principal_value(angle, min_=-pi)."""
    return (a + np.pi) % (2 * np.pi) - np.pi


def step_time(dt):
    """The bicycle model's step: a TimeDuration of int(dt * 1e6) microseconds read back as ``time_us * 1e-6``
    (pdm_simulator.py:56,62) - 0.09999999999999999 for dt = 0.1, one ulp below the tracker's dt."""
    return int(dt * 1e6) * 1e-6


def knots_from_trajectory(traj, ego):
    """(N, 8, 3) ego-frame poses + (N, 11) start states -> (N, 9, 3) global knots, heading unwrapped."""
    traj = np.asarray(traj, np.float64)
    x0, y0, h0 = ego[:, None, X], ego[:, None, Y], ego[:, None, HEADING]
    c, s = np.cos(h0), np.sin(h0)
    kx = x0 + c * traj[..., 0] - s * traj[..., 1]
    ky = y0 + s * traj[..., 0] + c * traj[..., 1]
    kh = h0 + traj[..., 2]
    k = np.stack([np.concatenate([x0, kx], 1), np.concatenate([y0, ky], 1), np.concatenate([h0, kh], 1)], -1)
    k[..., 2] = np.unwrap(k[..., 2], axis=1)
    return k


def interpolate_proposals(traj, ego_states, per_group=None):
    """(N, 8, 3) planner poses (ego frame) -> (N, 41, 3) float64 proposals on the 0.1 s grid; candidate n starts from
    ego_states[n // per_group] (per_group = N / G by default)."""
    traj = np.asarray(traj)
    n = traj.shape[0]
    ego = _per_candidate(ego_states, n, per_group)
    k = knots_from_trajectory(traj, ego)
    out = np.empty((n, T, 3), np.float64)
    for j in range(SUB):
        w = j / float(SUB)
        out[:, j:M:SUB] = k[:, :-1] + (k[:, 1:] - k[:, :-1]) * w
    out[:, M] = k[:, -1]
    return out


def _per_candidate(ego_states, n, per_group):
    ego = np.asarray(ego_states, np.float64).reshape(-1, STATES)
    if per_group is None:
        assert n % ego.shape[0] == 0
        per_group = n // ego.shape[0]
    assert n % per_group == 0 and ego.shape[0] == n // per_group, (n, per_group, ego.shape)
    return np.repeat(ego, per_group, axis=0)


def jerk_matrix(m=M):
    """R of the velocity fit, (m - 2) x m, exactly as batch_lqr_utils.py:59-70,116-117 leave it: -1 at (r, r + 1) and a
    single +1 at (m - 3, m - 1). NOT a difference matrix."""
    rows = m - 2
    banded = np.zeros((rows, rows + 1))
    eye = np.eye(rows)
    banded[:, 1:] = eye
    banded[:, :-1] = -eye
    return np.block([np.zeros((rows, 1)), banded])


def textbook_jerk_matrix(m=M):
    """What the docstring of _make_banded_difference_matrix promises (x_{k+1} - x_k): used by tests only, to show that
    the goldens tell the two apart."""
    rows = m - 2
    banded = np.zeros((rows, rows + 1))
    banded[np.arange(rows), np.arange(rows)] = -1.0
    banded[np.arange(rows), np.arange(rows) + 1] = 1.0
    return np.block([np.zeros((rows, 1)), banded])


def velocity_normal_matrix(dt, jerk_penalty, R=None, m=M):
    """L^T L + jerk_penalty R^T R: the design matrix's rows are (cos h_i, sin h_i) x L[i], L lower triangular with
    column 0 = dt and the others dt^2, so A^T A = L^T L whatever the candidate."""
    L = np.tril(np.full((m, m), dt * dt))
    L[:, 0] = dt
    R = jerk_matrix(m) if R is None else R
    return L, L.T @ L + jerk_penalty * (R.T @ R)


def fit_profiles(proposals, p=None, R=None):
    """(N, 41, 3) -> velocity profile (N, 40), curvature profile (N, 40) (batch_lqr_utils.py:189-249)."""
    p = p or DEFAULTS
    dt = p["dt"]
    poses = np.asarray(proposals, np.float64)
    n, m = poses.shape[0], poses.shape[1] - 1
    d = np.diff(poses, axis=1)
    head = poses[:, :-1, 2]
    # velocity fit
    L, G = velocity_normal_matrix(dt, p["jerk_penalty"], R, m)
    proj = d[..., 0] * np.cos(head) + d[..., 1] * np.sin(head)
    x = np.linalg.solve(G, (proj @ L).T).T
    vel = x[:, :1] + np.pad(np.cumsum(x[:, 1:] * dt, axis=-1), [(0, 0), (1, 0)])
    # curvature fit: A[i][0] = v_i dt, A[i][j] = v_i dt^2 for 1 <= j <= i
    y = normalize_angle(d[..., 2])
    A = np.repeat(np.tri(m)[None], n, axis=0)
    A[:, :, 0] = vel * dt
    A[:, 1:, 1:] *= (vel * dt ** 2)[:, 1:, None]
    Q = p["curvature_rate_penalty"] * np.eye(m)
    Q[0, 0] = p["initial_curvature_penalty"]
    At = A.transpose(0, 2, 1)
    x = np.linalg.solve(At @ A + Q, np.einsum("bij,bj->bi", At, y)[..., None])[..., 0]
    curv = x[:, :1] + np.pad(np.cumsum(x[:, 1:] * dt, axis=-1), [(0, 0), (1, 0)])
    return vel, curv


def track(proposals, vel, curv, state, it, p):
    """One tracker call at iteration ``it`` (batch_lqr.py:134-200): acceleration and steering-rate commands, and the
    two velocities the stopping decision compares with stopping_velocity."""
    dt, H, wb = p["dt"], p["tracking_horizon"], p["wheel_base"]
    n, m = vel.shape
    ref = proposals[:, it]
    xe, ye = state[:, X] - ref[:, 0], state[:, Y] - ref[:, 1]
    lat = -xe * np.sin(ref[:, 2]) + ye * np.cos(ref[:, 2])
    x0 = np.stack([lat, normalize_angle(state[:, HEADING] - ref[:, 2]), state[:, STEER]], -1)
    v0 = state[:, VX]
    ridx = min(it + H, m - 1)
    vref = vel[:, ridx]
    kap = np.zeros((n, H))
    length = ridx - it
    kap[:, :length] = curv[:, it:ridx]
    if length < H:
        kap[:, length:] = curv[:, ridx, None]
    stop = np.logical_and(vref <= p["stopping_velocity"], v0 <= p["stopping_velocity"])
    # longitudinal: one-step LQR over H * dt, or the stopping P controller
    B = H * dt
    inverse = -1 / (B * p["q_lon"] * B + p["r_lon"])
    accel = np.where(stop, -p["stopping_gain"] * (v0 - vref), inverse * B * p["q_lon"] * (v0 - vref))
    # lateral: H Euler steps of the linearised error dynamics, then the one-step LQR
    vprof = v0[:, None] + np.pad(np.cumsum(np.repeat(accel[:, None] * dt, H, axis=1), axis=1), [(0, 0), (1, 0)])[:, :H]
    A = np.tile(np.eye(3), (n, 1, 1))
    Bm = np.zeros((n, 3))
    g = np.zeros((n, 3))
    inm = np.array([0.0, 0.0, dt])
    for k in range(H):
        Mk = np.tile(np.eye(3), (n, 1, 1))
        Mk[:, 0, 1] = vprof[:, k] * dt
        Mk[:, 1, 2] = vprof[:, k] * dt / wb
        aff = np.zeros((n, 3))
        aff[:, 1] = -vprof[:, k] * kap[:, k] * dt
        A = Mk @ A
        Bm = np.einsum("bij,bj->bi", Mk, Bm) + inm
        g = np.einsum("bij,bj->bi", Mk, g) + aff
    err = np.einsum("bij,bj->bi", A, x0) + g
    err[:, 1:] = np.arctan2(np.sin(err[:, 1:]), np.cos(err[:, 1:]))
    btq = Bm * np.asarray(p["q_lat"], np.float64)
    steer_rate = -1 / ((btq * Bm).sum(-1) + p["r_lat"]) * (btq * err).sum(-1)
    return accel, np.where(stop, 0.0, steer_rate), vref, v0


def propagate(state, accel_cmd, rate_cmd, p):
    """batch_kinematic_bicycle.py:76-185. The low-passed steering ANGLE is never written into the propagating state:
    the heading integrates tan of the old angle, the new angle is clip(old + updated_rate * dt)."""
    dtc, wb = step_time(p["dt"]), p["wheel_base"]
    accel, steer = state[:, AX], state[:, STEER]
    ideal_steer = dtc * rate_cmd + steer
    upd_accel = dtc / (dtc + p["accel_time_constant"]) * (accel_cmd - accel) + accel
    upd_steer = dtc / (dtc + p["steering_time_constant"]) * (ideal_steer - steer) + steer
    upd_rate = (upd_steer - steer) / dtc
    v, h = state[:, VX], state[:, HEADING]
    out = state.copy()
    out[:, X] = state[:, X] + v * np.cos(h) * dtc
    out[:, Y] = state[:, Y] + v * np.sin(h) * dtc
    out[:, HEADING] = principal_value(h + v * np.tan(steer) / wb * dtc)
    out[:, VX] = v + upd_accel * dtc
    out[:, VY] = 0.0
    out[:, STEER] = np.clip(steer + upd_rate * dtc, -p["max_steering_angle"], p["max_steering_angle"])
    out[:, ANG_VEL] = out[:, VX] * np.tan(out[:, STEER]) / wb
    out[:, AX] = upd_accel
    out[:, AY] = 0.0
    out[:, ANG_ACC] = (out[:, ANG_VEL] - state[:, ANG_VEL]) / dtc
    out[:, STEER_RATE] = upd_rate
    return out


def simulate_proposals(proposals, ego_states, per_group=None, p=None, R=None, details=None):
    """(N, 41, 3) proposals, (G, 11) start states -> (N, 41, 11) simulated states. ``details`` (a dict) receives the
    fitted profiles and, per step, the two velocities of the stopping decision."""
    p = p or DEFAULTS
    proposals = np.asarray(proposals, np.float64)
    n = proposals.shape[0]
    assert proposals.shape[1:] == (T, 3), proposals.shape
    vel, curv = fit_profiles(proposals, p, R)
    out = np.zeros((n, T, STATES))
    out[:, 0] = _per_candidate(ego_states, n, per_group)
    vrefs, v0s = [], []
    for t in range(1, T):
        accel, rate, vref, v0 = track(proposals, vel, curv, out[:, t - 1], t - 1, p)
        out[:, t] = propagate(out[:, t - 1], accel, rate, p)
        vrefs.append(vref)
        v0s.append(v0)
    if details is not None:
        details.update(velocity_profile=vel, curvature_profile=curv, v_ref=np.stack(vrefs, 1), v_now=np.stack(v0s, 1))
    return out


def simulate_trajectories(traj, ego_states, per_group=None, p=None):
    """(N, 8, 3) planner poses -> (N, 41, 11): the proposal interpolation, then the simulator."""
    return simulate_proposals(interpolate_proposals(traj, ego_states, per_group), ego_states, per_group, p)


def stop_margin(v_ref, v_now, thr=DEFAULTS["stopping_velocity"]):
    """Distance of each stopping decision (v_ref <= thr and v_now <= thr) to its flip: stopping flips when either
    velocity rises past thr (the smaller gap); tracking flips only when every velocity above thr falls to it (the
    larger gap of those above)."""
    a, b = v_ref - thr, v_now - thr
    stop = (a <= 0) & (b <= 0)
    return np.where(stop, np.minimum(-a, -b), np.maximum(np.where(a > 0, a, 0.0), np.where(b > 0, b, 0.0)))


def heading_diff(a, b):
    """|a - b| modulo 2 pi."""
    d = (np.asarray(a) - np.asarray(b) + np.pi) % (2 * np.pi) - np.pi
    return np.abs(d)


def state_error(got, ref):
    """Largest state difference, the heading compared modulo 2 pi."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    d[..., HEADING] = heading_diff(got[..., HEADING], ref[..., HEADING])
    return float(d.max())
