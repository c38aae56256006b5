"""Shared pieces of the configuration-matrix tests (test_config_matrix_gpu.py and its CPU companion
test_config_matrix.py): the cases - every dd_config field dd_create accepts, away from its default -, their configs,
state dicts and scenes, the float64 oracle run of a case (the config, the step count and the schedule passed on) and
the error reduction with a bar on every (step, layer).

The error reduction and the bars are batch_sweep_util's (errors / bar_of); forward_train's oracle, the float64
LossComputer and the per-scene partials are train_sweep_util's."""
import numpy as np

import batch_sweep_util as U
import train_sweep_util as T

BATCH = 3          # the smallest batch DDMI_MAX_CHUNK=2 splits unevenly (2 + 1)
SCENE_SEED = 97    # synthetic_inputs / synthetic_targets seed of the scenes (used by no other test)
WEIGHT_SEED = 0    # seeded_state_dict seed (weights are keyed by (seed, key): the trunks of every ResNet-34 case are
                   # conftest's seeded_sd's, and cases that differ in the mode count or the schedule share everything
                   # but the anchors)
TRAIN_TIMESTEPS = (0, 49, 999)  # per scene: both ends of [0, 1000) and the reference's largest draw
MAX_MODES = 128    # DD_MAX_MODES (include/ddmi.h)
FEATS = U.INPUT_KEYS[:3]

# case -> (TransfuserConfig fields, steps, schedule). "trunk": the cases with the same key share the oracle's run of
# everything before the trajectory head (same weights, same camera / LiDAR / status).
CASES = {
    "lidar2": (dict(use_ground_plane=True), 2, "truncated"),
    "lidar3": (dict(lidar_seq_len=3), 2, "truncated"),
    "lidar4": (dict(use_ground_plane=True, lidar_seq_len=2), 2, "truncated"),
    "r50_lidar2": (dict(image_architecture="resnet50", use_ground_plane=True), 2, "truncated"),
    "modes1": (dict(num_modes=1), 2, "truncated"),
    "modes33": (dict(num_modes=33), 2, "truncated"),
    "modes64": (dict(num_modes=64), 2, "truncated"),
    "modes128": (dict(num_modes=MAX_MODES), 2, "truncated"),
    "trunc0_span1": (dict(trunc_timestep=0, step_span=1), 1, "truncated"),
    "trunc999_span1000": (dict(trunc_timestep=999, step_span=1000), 4, "truncated"),  # roll 750, 500, 250, 0
    # the default config (the session's handle): the step counts no test has run
    "steps3": ({}, 3, "truncated"),      # roll 13, 7, 0 (20 / 3 does not divide: 6.67 -> 7, truncation gives 6)
    "steps7": ({}, 7, "truncated"),      # roll 17, 14, 11, 9, 6, 3, 0
    "steps20": ({}, 20, "truncated"),    # roll 19 .. 0: steps = step_span
    "vanilla3": ({}, 3, "vanilla"),      # 1000 // 3 = 333 does not divide: 666, 333, 0
    "vanilla1": ({}, 1, "vanilla"),
}
LIDAR_CASES = ("lidar2", "lidar3", "lidar4", "r50_lidar2")
MODE_CASES = ("modes1", "modes33", "modes64", "modes128")
SCHEDULE_CASES = ("trunc0_span1", "trunc999_span1000")
DEFAULT_CASES = ("steps3", "steps7", "steps20", "vanilla3", "vanilla1")
FRESH_CASES = LIDAR_CASES + MODE_CASES + SCHEDULE_CASES  # one fresh handle each
F16X3_ONLY = ("r50_lidar2",)
CHUNK_CASES = ("lidar2", "modes33")                      # the DDMI_MAX_CHUNK=2 comparison
TRAIN_CASES = ("lidar2", "modes33", "modes64", "modes128")
assert set(CASES) == set(FRESH_CASES + DEFAULT_CASES)


def gemm_modes(case):
    return ("f16x3",) if case in F16X3_ONLY else ("f16x3", "fp32")


def case_config(case):
    from diffusiondrive_amd.config import TransfuserConfig
    return TransfuserConfig(**CASES[case][0])


def case_steps(case):
    """(steps, schedule)"""
    return CASES[case][1], CASES[case][2]


def trunk_key(case):
    """Cases with the same key run the same network on the same inputs up to the trajectory head."""
    return case if case in LIDAR_CASES else "default"


def case_state_dict(case):
    from diffusiondrive_amd.weights import seeded_state_dict
    return seeded_state_dict(case_config(case), WEIGHT_SEED)


def case_inputs(case):
    """The BATCH scenes of the case: inputs with noise, timesteps (BATCH,) int64, target trajectories (BATCH, 8, 3)."""
    from diffusiondrive_amd.weights import synthetic_inputs, synthetic_targets
    cfg = case_config(case)
    inp = synthetic_inputs(BATCH, SCENE_SEED, cfg)
    tg = synthetic_targets(BATCH, SCENE_SEED, cfg)["trajectory"]
    return inp, np.array(TRAIN_TIMESTEPS, dtype=np.int64), np.ascontiguousarray(tg, dtype=np.float32)


def step_layers(case):
    steps, _ = case_steps(case)
    return [(s, l) for s in range(steps) for l in range(2)]


def roll_of(case):
    """The denoise timesteps of the case, first step first (oracle.model.trajectory_head's arithmetic)."""
    cfg, (steps, schedule) = case_config(case), case_steps(case)
    if schedule == "vanilla":
        return ((np.arange(steps) * (cfg.num_train_timesteps // steps))[::-1]).astype(np.int64).tolist()
    return (np.arange(steps) * (cfg.step_span / steps)).round()[::-1].astype(np.int64).tolist()


# --------------------------------------------------------------------------- oracle
def oracle_trunk(sd, inp, cfg, dtype=np.float64):
    """Everything of the oracle before the trajectory head, in ``dtype`` with the config: the features
    (ego query, agent queries, BEV map, p3) and the taps of that part by the names the GPU side uses (NHWC)."""
    import torch
    from oracle.model import OracleModel, Taps
    om = OracleModel(T._cast_sd(sd, dtype), cfg)
    taps = Taps()
    with torch.no_grad():
        feats = om._features(*(np.asarray(inp[k]).astype(dtype) for k in FEATS), taps=taps)
    B = feats[0].shape[0]
    ref = {"img_l4": taps["img_l4"].permute(0, 2, 3, 1).contiguous().numpy(),
           "p3": taps["p3"].permute(0, 2, 3, 1).contiguous().numpy(),
           "bev_feature": taps["bev_feature"].permute(0, 2, 3, 1).contiguous().numpy(),
           "keyval": taps["keyval"].numpy(),
           "cross_bev": taps["cross_bev"].permute(0, 2, 3, 1).reshape(B, -1, taps["cross_bev"].shape[1]).numpy(),
           "query_out": taps["query_out"].numpy()}
    return feats, ref


def oracle_case(sd, inp, cfg, steps, schedule, dtype=np.float64, trunk=None):
    """One oracle forward of a case in ``dtype``: batch_sweep_util.oracle_run with the config, the step count and the
    schedule (gs / reg / cls taps at every (step, layer) the case runs). ``trunk``: an oracle_trunk result of the
    same weights before the head, inputs and dtype to reuse."""
    import torch
    from oracle.model import OracleModel, Taps, trajectory_head
    feats, ref = trunk if trunk is not None else oracle_trunk(sd, inp, cfg, dtype)
    ref = dict(ref)
    om = OracleModel(T._cast_sd(sd, dtype), cfg)
    ego_q, agents_q, cross, p3 = feats
    taps = Taps()
    with torch.no_grad():
        nz = torch.as_tensor(np.asarray(inp["noise"]).astype(dtype))
        traj, reg, cls = trajectory_head(ego_q, agents_q, cross, om.sd, cfg, nz, steps, taps, schedule)
        heads = om._heads(p3, agents_q)
    ref.update(trajectory=traj.numpy(), poses_reg=reg.numpy(), poses_cls=cls.numpy())
    ref.update({k: v.numpy() for k, v in heads.items()})
    for s in range(steps):
        for l in range(2):
            for k in ("gs", "reg", "cls"):
                ref[f"{k}_s{s}l{l}"] = taps[f"{k}_s{s}l{l}"].numpy()
    for k, v in ref.items():
        assert v.dtype == dtype, (k, v.dtype)
    return ref


def start_image(sd, inp, cfg, dtype=np.float64):
    """The truncated schedule's start of the denoising before its clamp: add_noise(norm_odo(anchor), noise,
    trunc_timestep) (transfuser_model_v2.py:593-597), (B, Q, P, 2)."""
    import torch
    from oracle.model import DDIM, norm_odo
    anchor = torch.as_tensor(np.asarray(sd["_trajectory_head.plan_anchor"]).astype(dtype))[None]
    nz = torch.as_tensor(np.asarray(inp["noise"]).astype(dtype))
    return DDIM(cfg.num_train_timesteps, dtype=nz.dtype).add_noise(norm_odo(anchor), nz, cfg.trunc_timestep).numpy()


# --------------------------------------------------------------------------- errors
def _is_mode_tap(name):
    return name[:5] in ("reg_s", "cls_s")


def errors(got, ref):
    """batch_sweep_util.errors with the reg / cls taps of every step absolute (its own list of those names stops at
    two steps)."""
    e = U.errors({k: v for k, v in got.items() if not _is_mode_tap(k)}, ref)
    for k, v in got.items():
        if _is_mode_tap(k):
            g, r = np.asarray(v, np.float64), np.asarray(ref[k], np.float64)
            assert g.shape == r.shape, (k, g.shape, r.shape)
            e[k] = float(np.abs(g - r).max())
    return e


def bar_of(name, bars):
    return bars["mode"] if _is_mode_tap(name) else U.bar_of(name, bars)
