"""Shared pieces of the training-mode sweep (test_train_sweep_gpu.py and its CPU companion test_train_sweep.py): the
sweep's batches, the distinct scenes with their timesteps and targets, the float64 oracle run of forward_train, the
float64 LossComputer on given outputs (batch loss and per-scene partial sums) and the doctored training cases.

The replica builder, the chunking and the launch-log helpers are batch_sweep_util's."""
import numpy as np

import batch_sweep_util as U
from decoder_edge_util import BATCH, DL, INPUT_SEED, make_case

# The batches of the GPU sweep, run in this order on one handle: the order grows, shrinks and regrows the handle-wide
# partials buffer (train_part); 16 | 17 and 32 | 33 are decoder_mk's 4 | 2 | 1 query-group boundaries, 129 runs as
# 65 + 64 and 257 (chunks 86, 86, 85) is the smallest batch at which traj_loss_reduce_kernel's thread loop runs twice.
# The three training-only GEMM shapes - rows = B with (K, N) = (256, 1024), (1024, 256), (256, 512), the time MLP and
# the FiLM Linear - take one route at every batch: gemm() passes no K-split scratch, conv_x6 takes 3 x 3 convs only,
# conv_x5 wants M >= 16384 or at least 128 256-row tiles, and with rows <= 128 per chunk conv_x3's own choice
# (ceil(M / 128) * ceil(N / 128) <= 8 < 512) is the 64 x 64 tile, as conv_gemm's is in the fp32 mode. What changes with
# the batch is the number of 64-row tiles and their ragged tail: one partial tile up to B = 63 (1, 3, 16, 17, 32, 33
# rows here), two tiles at 65 (a tail of one row), 64 (full), 85 / 86 (a tail of 21 / 22). No batch is added.
TRAIN_SWEEP = [3, 33, 1, 257, 16, 17, 129, 32]
TIMESTEPS = (0, 49, 7, 999, 500)  # per distinct scene: both ends of [0, 1000), and two values below 50
FORM_BATCH = 3                    # the batch of the other forms (groups1 / groups2 / unfused / fp32)

Q, P = U.Q, U.P
FEATS = U.INPUT_KEYS[:3]

# doctored training cases (decoder_edge_util.make_case's B = 2 batch): per-scene timesteps and the targets' seed
CASE_TIMESTEPS = (49, 0)
CASE_TARGET_SEED = 7
SATURATION = 60.0  # the shift of saturated_cls (the CPU companion shows the premise at this value)
TRAIN_CASES = ("equal_modes", "tied_anchors", "clamp_noise", "saturated_cls_pos", "saturated_cls_neg")


def distinct_scenes():
    """(inputs with noise, timesteps (5,) int64, target trajectories (5, 8, 3) fp32) of the 5 distinct scenes."""
    from diffusiondrive_amd.weights import synthetic_inputs, synthetic_targets
    inp = synthetic_inputs(U.N_DISTINCT, U.SCENE_SEED)
    tg = synthetic_targets(U.N_DISTINCT, U.SCENE_SEED)["trajectory"]
    return inp, np.array(TIMESTEPS, dtype=np.int64), np.ascontiguousarray(tg, dtype=np.float32)


def make_train_case(seeded_sd, name):
    """(state dict, inputs, timesteps (2,), target trajectories (2, 8, 3)) of a doctored training case:
    decoder_edge_util's equal_modes / clamp_noise, tied_anchors (equal_modes' anchors with the noise as drawn: the 20
    anchor distances tie while the modes' rows differ, so the loss tells which mode the argmin took), or
    saturated_cls_pos / _neg (the last Linear's bias of both layers' cls branch shifted by +- SATURATION: every logit
    saturates the sigmoid of the focal loss)."""
    from diffusiondrive_amd.weights import synthetic_inputs, synthetic_targets
    if name in ("saturated_cls_pos", "saturated_cls_neg"):
        sd = {k: np.array(v, copy=True) for k, v in seeded_sd.items()}
        inp = dict(synthetic_inputs(BATCH, INPUT_SEED))  # the batch of make_case, noise as drawn
        shift = SATURATION if name.endswith("pos") else -SATURATION
        for l in range(2):
            sd[DL + f"{l}.task_decoder.plan_cls_branch.6.bias"] += np.float32(shift)
    elif name == "tied_anchors":
        sd, inp = make_case(seeded_sd, "equal_modes")
        inp["noise"] = synthetic_inputs(BATCH, INPUT_SEED)["noise"]
    else:
        sd, inp = make_case(seeded_sd, name)
    tg = synthetic_targets(BATCH, CASE_TARGET_SEED)["trajectory"]
    return sd, inp, np.array(CASE_TIMESTEPS, dtype=np.int64), np.ascontiguousarray(tg, dtype=np.float32)


# --------------------------------------------------------------------------- oracle
def _cast_sd(sd, dtype):
    return {k: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in sd.items()}


def oracle_features(sd, inp, dtype=np.float64):
    """Everything of the oracle before the trajectory head, in ``dtype``: (ego query, agent queries, BEV map). It
    depends on the inputs and on no weight of the trajectory head, so the doctored cases (which edit only that head and
    the noise) share one run."""
    import torch
    from oracle.model import OracleModel
    om = OracleModel(_cast_sd(sd, dtype))
    with torch.no_grad():
        ego_q, agents_q, cross, _ = om._features(*(np.asarray(inp[k]).astype(dtype) for k in FEATS))
    return ego_q, agents_q, cross


def oracle_train(sd, inp, timesteps, targets, dtype=np.float64, features=None):
    """One oracle forward_train in ``dtype`` (state dict, inputs, noise and targets cast to it): reg_l0 / reg_l1
    (B, 20, 8, 3), cls_l0 / cls_l1 (B, 20), trajectory (B, 8, 3) and the three losses, as numpy arrays of ``dtype``.
    ``features``: an oracle_features result of the same inputs and dtype to reuse."""
    import torch
    from oracle.model import OracleModel, loss_computer, trajectory_head_train
    om = OracleModel(_cast_sd(sd, dtype))
    nz = torch.as_tensor(np.asarray(inp["noise"]).astype(dtype))
    tt = torch.as_tensor(np.asarray(targets).astype(dtype))
    with torch.no_grad():
        if features is None:
            out = om.forward_train(*(np.asarray(inp[k]).astype(dtype) for k in FEATS), nz, np.asarray(timesteps),
                                   {"trajectory": tt}, heads=False)
            best, regs, clss = out["trajectory"], out["poses_reg_list"], out["poses_cls_list"]
            losses = [out["trajectory_loss_dict"][f"trajectory_loss_{l}"] for l in range(2)]
        else:
            ego_q, agents_q, cross = features
            best, regs, clss = trajectory_head_train(ego_q, agents_q, cross, om.sd, om.cfg, nz, np.asarray(timesteps))
            anchor = om.sd["_trajectory_head.plan_anchor"].unsqueeze(0).repeat(nz.shape[0], 1, 1, 1)
            losses = [loss_computer(r, c, tt, anchor, om.cfg) for r, c in zip(regs, clss)]
    ref = {"trajectory": best.numpy()}
    for l in range(2):
        ref[f"reg_l{l}"], ref[f"cls_l{l}"] = regs[l].numpy(), clss[l].numpy()
        ref[f"loss_{l}"] = np.asarray(losses[l].numpy())
    ref["loss"] = np.asarray((losses[0] + losses[1]).numpy())
    for k, v in ref.items():
        assert v.dtype == dtype, (k, v.dtype)
    return ref


def loss64(reg, cls, target, anchor, cfg=None):
    """oracle.loss_computer in float64 on the given outputs (any float arrays; B on axis 0) and targets: a float."""
    import torch
    from diffusiondrive_amd.config import TransfuserConfig
    from oracle.model import loss_computer
    r, c, t, a = (torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in (reg, cls, target, anchor))
    return float(loss_computer(r, c, t, a[None].repeat(r.shape[0], 1, 1, 1), cfg or TransfuserConfig()))


def nearest_modes(target, anchor):
    """LossComputer's class target in float64: (mode (B,), mean distance per mode (B, 20))."""
    t, a = np.asarray(target, np.float64), np.asarray(anchor, np.float64)
    dist = np.sqrt(((t[:, None, :, :2] - a[None]) ** 2).sum(-1)).mean(-1)
    return dist.argmin(-1), dist


def scene_partials64(reg, cls, target, anchor, mode=None):
    """The per-scene sums LossComputer's means are made of, in float64: (B, 2) = (sum over the 20 modes of the sigmoid
    focal term against the one-hot nearest mode, sum over poses and channels of |reg[mode] - target|). The batch loss
    is cls_w * sum(col 0) / (B * 20) + reg_w * sum(col 1) / (B * 24) (the CPU companion checks that against
    oracle.loss_computer). ``mode`` (B,): a class target to use instead of the nearest anchor (what a wrong argmin
    would have picked)."""
    import torch
    import torch.nn.functional as F
    r, c, t = (torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in (reg, cls, target))
    mode = torch.as_tensor(nearest_modes(target, anchor)[0] if mode is None else np.asarray(mode, dtype=np.int64))
    B = r.shape[0]
    onehot = torch.zeros_like(c)
    onehot[torch.arange(B), mode] = 1
    ps = c.sigmoid()
    pt = (1 - ps) * onehot + ps * (1 - onehot)
    fw = (0.25 * onehot + 0.75 * (1 - onehot)) * pt.pow(2.0)
    focal = (F.binary_cross_entropy_with_logits(c, onehot, reduction="none") * fw).sum(-1)
    l1 = (r[torch.arange(B), mode] - t).abs().flatten(1).sum(-1)
    return torch.stack([focal, l1], -1).numpy()


def train_errors(got, ref):
    """Largest error of ``got`` (name -> array over some scenes) against ``ref`` (the same scenes): absolute on reg_l* /
    cls_l*, the waypoint L2 (max over scenes) and the heading of the trajectory."""
    e = {}
    for k, v in got.items():
        g, r = np.asarray(v, np.float64), np.asarray(ref[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k == "trajectory":
            d = (g[..., :2] - r[..., :2]).reshape(g.shape[0], -1)
            e["waypoint_l2"] = float(np.sqrt((d ** 2).sum(-1)).max())
            e["heading"] = float(np.abs(g[..., 2] - r[..., 2]).max())
        else:
            e[k] = float(np.abs(g - r).max())
    return e
