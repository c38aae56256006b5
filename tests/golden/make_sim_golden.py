#!/usr/bin/env python3
"""Golden vectors of the PDM proposal simulation, from the REFERENCE's PDMSimulator run unmodified (build container
only).

``PDMSimulator.simulate_proposals`` (pdm_planner/simulation/pdm_simulator.py:32-79: BatchLQRTracker +
BatchKinematicBicycleModel over 40 steps) is imported from the reference tree through the ``refshim`` stub finder.
The few nuPlan names its arithmetic really uses are registered as small real stand-ins before the import:
``VehicleParameters`` / ``get_pacifica_parameters`` (wheel_base 3.089), ``TimePoint`` / ``TimeDuration`` (integer
microseconds, ``time_s = time_us * 1e-6``), ``SimulationIteration`` and ``principal_value``; the simulator is fed a
duck-typed ego state.

Candidates (N = 96 per file, the same planner poses in every file): seeded kinematic plans (v0 0-12 m/s, acceleration
-2..1.5 m/s^2, yaw rate +-0.25 rad/s, 2 cm pose noise, rounded through float32), all-zero stationary plans, creeping
plans (x 0.02) and reversing plans. Each set is run from three start states: a moving start and a standing start in
the ego frame, and a moving start at nuPlan-sized global coordinates with a heading near pi. The proposals are the
candidates on the 0.1 s grid (tests/pdm_sim_ref.py:interpolate_proposals; nuPlan's InterpolatedTrajectory is not
available offline).

The generator asserts that every stopping decision the reference takes (v_ref <= 0.2 and v <= 0.2, batch_lqr.py:169)
is at least 1e-6 m/s from flipping, for every candidate and step; a seed that fails is replaced by the next one. No
candidate is excluded.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sim_golden.py [seed]
Writes tests/golden/pdm_sim_s{seed}_{moving,standing,global}.npz. Only data is stored; nothing of the reference's
source.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import pdm_sim_ref as R  # noqa: E402

SEED = 3
N_KINEMATIC, N_STATIONARY, N_CREEPING, N_REVERSING = 72, 4, 10, 10
MARGIN = 1e-6

# start states in StateIndex order: x, y, heading, vx, vy, ax, ay, steering angle, steering rate, yaw rate, yaw accel
STARTS = {
    "moving": [0.0, 0.0, 0.0, 5.2, 0.0, 0.4, 0.0, 0.015, 0.01, 0.025, 0.002],
    "standing": [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
    "global": [664431.37, 3997675.12, np.pi - 0.05, 7.9, 0.0, -0.6, 0.0, -0.03, 0.02, -0.08, 0.01],
}


# ---- stand-ins for the nuPlan names the simulator's arithmetic uses
class VehicleParameters:
    def __init__(self, wheel_base):
        self.wheel_base = wheel_base


def get_pacifica_parameters():
    return VehicleParameters(wheel_base=3.089)


class TimeDuration:
    def __init__(self, time_us):
        self.time_us = int(time_us)

    @classmethod
    def from_s(cls, t_s):
        return cls(int(t_s * 1e6))

    @property
    def time_s(self):
        return self.time_us * 1e-6


class TimePoint:
    def __init__(self, time_us):
        self.time_us = int(time_us)

    @property
    def time_s(self):
        return self.time_us * 1e-6

    def __add__(self, other):
        return TimePoint(self.time_us + other.time_us)

    def __sub__(self, other):
        if isinstance(other, TimePoint):
            return TimeDuration(self.time_us - other.time_us)
        return TimePoint(self.time_us - other.time_us)


class SimulationIteration:
    def __init__(self, time_point, index):
        self.time_point = time_point
        self.index = index


def principal_value(angle, min_=-np.pi):
    return (angle - min_) % (2 * np.pi) + min_


def _register(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod


class _Vec:
    def __init__(self, x, y):
        self.array = np.array([x, y], np.float64)


class _Pose:
    def __init__(self, x, y, h):
        self.x, self.y, self.heading = x, y, h

    def serialize(self):
        return [self.x, self.y, self.heading]


class DuckEgoState:
    """The attributes ego_state_to_state_array and simulate_proposals read (pdm_array_representation.py:63-81)."""

    def __init__(self, s, time_us=1_600_000_000_000_000):
        self.rear_axle = _Pose(s[0], s[1], s[2])
        dyn = types.SimpleNamespace(rear_axle_velocity_2d=_Vec(s[3], s[4]), rear_axle_acceleration_2d=_Vec(s[5], s[6]),
                                    tire_steering_rate=s[8], angular_velocity=s[9], angular_acceleration=s[10])
        self.dynamic_car_state = dyn
        self.tire_steering_angle = s[7]
        self.car_footprint = types.SimpleNamespace(vehicle_parameters=get_pacifica_parameters())
        self.time_point = TimePoint(time_us)


# ---- candidates
def kinematic_plans(rng, n):
    """Constant-acceleration, constant-yaw-rate plans sampled at 0.5 s, 2 cm pose noise."""
    v0 = rng.uniform(0.0, 12.0, n)
    acc = rng.uniform(-2.0, 1.5, n)
    yaw = rng.uniform(-0.25, 0.25, n)
    out = np.zeros((n, R.NUM_POSES, 3))
    fine = 50
    for i in range(n):
        x = y = h = 0.0
        v = v0[i]
        for k in range(R.NUM_POSES):
            for _ in range(fine):
                step = 0.5 / fine
                x += v * np.cos(h) * step
                y += v * np.sin(h) * step
                h += yaw[i] * min(v, 1.0) * step
                v = max(v + acc[i] * step, 0.0)
            out[i, k] = (x, y, h)
    out[..., :2] += rng.normal(0.0, 0.02, out[..., :2].shape)
    out[..., 2] += rng.normal(0.0, 0.002, out[..., 2].shape)
    return out


def candidates(seed):
    rng = np.random.default_rng(seed)
    kin = kinematic_plans(rng, N_KINEMATIC)
    still = np.zeros((N_STATIONARY, R.NUM_POSES, 3))
    creep = kinematic_plans(rng, N_CREEPING) * 0.02
    rev = kinematic_plans(rng, N_REVERSING)
    rev[..., 0] *= -0.3   # backwards along x, heading still forwards
    rev[..., 1] *= 0.3
    rev[..., 2] *= 0.3
    return np.concatenate([kin, still, creep, rev]).astype(np.float32)


def run_reference(simulator, tracker_log, proposals, start):
    from navsim.planning.simulation.planner.pdm_planner.utils.pdm_enums import StateIndex
    states = np.zeros((proposals.shape[0], R.T, StateIndex.size()))
    states[..., :3] = proposals
    tracker_log.clear()
    sim = simulator.simulate_proposals(states, DuckEgoState(start))
    return sim


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    import refshim
    refshim.install_stub_finder()
    _register("nuplan.common.actor_state.vehicle_parameters", VehicleParameters=VehicleParameters,
              get_pacifica_parameters=get_pacifica_parameters)
    # StateSE2 / StateVector2D are imported by name only (type annotations of helpers the simulator never calls)
    _register("nuplan.common.actor_state.state_representation", TimePoint=TimePoint, TimeDuration=TimeDuration,
              StateSE2=_Pose, StateVector2D=_Vec)
    _register("nuplan.planning.simulation.simulation_time_controller.simulation_iteration",
              SimulationIteration=SimulationIteration)
    _register("nuplan.common.geometry.compute", principal_value=principal_value)
    sys.path.insert(0, REF)
    from navsim.planning.simulation.planner.pdm_planner.simulation.pdm_simulator import PDMSimulator
    from nuplan.planning.simulation.trajectory.trajectory_sampling import TrajectorySampling

    simulator = PDMSimulator(TrajectorySampling(num_poses=R.M, interval_length=0.1))
    # record (not change) what the tracker compares with the stopping velocity, and the profiles it fits
    tracker = simulator._tracker
    log = []
    inner_ref = tracker._compute_reference_velocity_and_curvature_profile
    inner_now = tracker._compute_initial_velocity_and_lateral_state

    def ref_hook(it):
        out = inner_ref(it)
        log.append(("ref", out[0].copy()))
        return out

    def now_hook(it, values):
        out = inner_now(it, values)
        log.append(("now", out[0].copy()))
        return out

    tracker._compute_reference_velocity_and_curvature_profile = ref_hook
    tracker._compute_initial_velocity_and_lateral_state = now_hook

    while True:
        traj = candidates(seed)
        files, worst = {}, np.inf
        for name, start in STARTS.items():
            ego = np.array([start], np.float64)
            proposals = R.interpolate_proposals(traj, ego)
            sim = run_reference(simulator, log, proposals, start)
            v_ref = np.stack([v for k, v in log if k == "ref"], 1)
            v_now = np.stack([v for k, v in log if k == "now"], 1)
            assert v_ref.shape == v_now.shape == (traj.shape[0], R.M)
            margin = R.stop_margin(v_ref, v_now)
            worst = min(worst, float(margin.min()))
            files[name] = dict(seed=np.array(seed), trajectory=traj, ego_states=ego, proposals=proposals, states=sim,
                               velocity_profile=tracker._velocity_profile.copy(),
                               curvature_profile=tracker._curvature_profile.copy(),
                               stop_steps=np.array(int(((v_ref <= 0.2) & (v_now <= 0.2)).sum())),
                               stop_margin=np.array(float(margin.min())))
        if worst >= MARGIN:
            break
        print(f"seed {seed}: a stopping decision is {worst:.3e} m/s from flipping (< {MARGIN}); next seed")
        seed += 1
    for name, rec in files.items():
        path = os.path.join(HERE, f"pdm_sim_s{seed}_{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, N={traj.shape[0]}, stop steps {int(rec['stop_steps'])}, "
              f"stop margin {float(rec['stop_margin']):.3e}")


if __name__ == "__main__":
    main()
