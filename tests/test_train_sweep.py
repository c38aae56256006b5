"""CPU companion of test_train_sweep_gpu.py: what the training-mode sweep rests on, shown without a GPU.

- the sweep's batches are the documented ones and chunk as the GPU tests assume; the replicas repeat the distinct
  scenes' inputs, noise, timesteps and targets byte for byte with period 5;
- oracle.trajectory_head_train follows the dtype of its inputs: a float64 state dict with float64 inputs runs the
  training head in float64 (no fp32 constant left in the schedule or the timestep embedding), and that run does not
  depend on the batch (a scene in a batch of 2 against the scene alone, <= 1e-10), so one float64 run of the 5 distinct
  scenes is the truth for every replica and every batch;
- the training head is well conditioned at every timestep of the sweep, t = 999 and 500 included: the fp32 oracle
  stays within half of the parity bars of its float64 self;
- LossComputer's nearest anchor is decided by a margin far above fp32 rounding on every scene, so the GPU's fp32
  argmin cannot legitimately differ from the float64 one;
- the per-scene partial sums of train_sweep_util.scene_partials64 add up to oracle.loss_computer;
- the doctored training cases reach what they claim.
"""
import numpy as np
import pytest
import torch

import batch_sweep_util as U
import train_sweep_util as T
from test_parity_gpu import HEADING_TOL, MODE_TOL, WAYPOINT_L2_TOL

OUT_KEYS = ("trajectory", "reg_l0", "reg_l1", "cls_l0", "cls_l1")


def _bar(name):
    return WAYPOINT_L2_TOL if name == "waypoint_l2" else HEADING_TOL if name == "heading" else MODE_TOL


def _outs(ref, sl=slice(None)):
    return {k: ref[k][sl] for k in OUT_KEYS}


@pytest.fixture(scope="module")
def scenes():
    return T.distinct_scenes()


@pytest.fixture(scope="module")
def truth(seeded_sd, scenes):
    inp, t, tg = scenes
    return T.oracle_train(seeded_sd, inp, t, tg)


@pytest.fixture(scope="module")
def case_features(seeded_sd):
    """The oracle before the trajectory head on the doctored cases' batch, per dtype (the cases edit the head only)."""
    _, inp, _, _ = T.make_train_case(seeded_sd, "clamp_noise")
    return {dt: T.oracle_features(seeded_sd, inp, dt) for dt in (np.float64, np.float32)}


def test_sweep_is_the_documented_one():
    assert T.TRAIN_SWEEP == [3, 33, 1, 257, 16, 17, 129, 32] and T.TIMESTEPS == (0, 49, 7, 999, 500)
    assert len(T.TIMESTEPS) == U.N_DISTINCT and T.FORM_BATCH in T.TRAIN_SWEEP
    assert U.chunk_ranges(257) == [(0, 86), (86, 86), (172, 85)] and U.chunk_ranges(129) == [(0, 65), (65, 64)]
    assert all(len(U.chunk_ranges(B)) == 1 for B in T.TRAIN_SWEEP if B <= 128)
    # the partials buffer grows (3 -> 33, 33 -> 257), is kept through smaller batches, and 257 > 256 partials per layer
    assert max(T.TRAIN_SWEEP) == 257 and T.TRAIN_SWEEP.index(257) not in (0, len(T.TRAIN_SWEEP) - 1)
    # both sides of the decoder's group boundaries, and one batch per group count on either side of a chunked one
    groups = {B: (4 if B <= 16 else 2 if B <= 32 else 1) for B in T.TRAIN_SWEEP}
    assert groups[16] == 4 and groups[17] == 2 and groups[32] == 2 and groups[33] == 1
    # a later chunk starts in the middle of a period: its scenes carry other timesteps than the same places of chunk 0
    idx = U.replica_index(257)
    assert [T.TIMESTEPS[i] for i in idx[86:89]] == [49, 7, 999] and [T.TIMESTEPS[i] for i in idx[:3]] == [0, 49, 7]


def test_replicas_are_byte_identical(scenes):
    inp, t, tg = scenes
    assert t.tolist() == list(T.TIMESTEPS) and tg.shape == (U.N_DISTINCT, T.P, 3) and tg.dtype == np.float32
    # two rows of every camera / LiDAR plane are enough for the builder (it indexes axis 0)
    small = {k: inp[k] if k in ("status_feature", "noise") else inp[k][:, :, :2] for k in U.INPUT_KEYS}
    for B in (1, 3, 17, 33):
        idx = U.replica_index(B)
        rep = U.build_replicas(small, B)
        tb, tgb = t[idx], tg[idx]
        for i in range(B):
            d = i % U.N_DISTINCT
            assert rep["noise"][i].tobytes() == inp["noise"][d].tobytes()
            assert rep["status_feature"][i].tobytes() == inp["status_feature"][d].tobytes()
            assert rep["camera_feature"][i].tobytes() == inp["camera_feature"][d, :, :2].tobytes()
            assert tb[i] == T.TIMESTEPS[d] and tgb[i].tobytes() == tg[d].tobytes()
    # period 5 against the groupings: a FiLM row or coefficient taken from a neighbouring scene is another timestep's
    assert all(T.TIMESTEPS[i % 5] != T.TIMESTEPS[(i + 1) % 5] for i in range(5))
    assert len({(int(d), i % 4) for i, d in enumerate(U.replica_index(20))}) == 20


def test_training_head_follows_the_dtype(truth):
    for k, v in truth.items():
        assert v.dtype == np.float64 and np.isfinite(v).all(), k


def test_float64_training_oracle_does_not_depend_on_the_batch(seeded_sd, scenes, truth):
    """Scenes 3 and 4 (t = 999 and 500) as a batch of 2, each alone, and as part of the batch of 5: every output
    within 1e-10."""
    inp, t, tg = scenes
    sub = lambda sl: ({k: inp[k][sl] for k in U.INPUT_KEYS}, t[sl], tg[sl])  # noqa: E731
    both = T.oracle_train(seeded_sd, *sub(slice(3, 5)))
    e = T.train_errors(_outs(both), _outs(truth, slice(3, 5)))
    assert max(e.values()) <= 1e-10, e
    for i in (3, 4):
        one = T.oracle_train(seeded_sd, *sub(slice(i, i + 1)))
        e = T.train_errors(_outs(one), _outs(both, slice(i - 3, i - 2)))
        assert max(e.values()) <= 1e-10, (i, e)


def test_fp32_oracle_is_well_conditioned_at_every_timestep(seeded_sd, scenes, truth):
    """fp32 oracle against float64 oracle on the 5 scenes: within half of the parity bars, the same argmax mode.
    Measured: reg <= 1.9e-5, cls <= 1.1e-5 at t = 999 and 500, <= 8.2e-6 at t < 50; waypoint L2 <= 1.3e-5."""
    inp, t, tg = scenes
    r32 = T.oracle_train(seeded_sd, inp, t, tg, np.float32)
    for i in range(U.N_DISTINCT):
        e = T.train_errors(_outs(r32, slice(i, i + 1)), _outs(truth, slice(i, i + 1)))
        print(f"t = {t[i]}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= 0.5 * _bar(k), (i, k, v)
    for l in range(2):
        assert np.array_equal(r32[f"cls_l{l}"].argmax(-1), truth[f"cls_l{l}"].argmax(-1)), l
    for k in ("loss_0", "loss_1", "loss"):
        assert abs(float(r32[k]) - float(truth[k])) <= 1e-5 * abs(float(truth[k])), k


def test_nearest_anchor_margins(seeded_sd, scenes):
    """Second-smallest minus smallest mean anchor distance >= 1e-3 m on every scene (measured: 0.16 m the smallest;
    fp32 rounding of a mean of 8 distances of tens of metres is below 1e-5 m), the nearest modes all distinct."""
    _, _, tg = scenes
    mode, dist = T.nearest_modes(tg, seeded_sd["_trajectory_head.plan_anchor"])
    ds = np.sort(dist, -1)
    assert (ds[:, 1] - ds[:, 0]).min() >= 1e-3, ds[:, 1] - ds[:, 0]
    assert mode.tolist() == [4, 5, 6, 9, 7]


def test_scene_partials_add_up_to_the_loss(seeded_sd, scenes, truth):
    """cls_w * sum(focal) / (B * 20) + reg_w * sum(l1) / (B * 24) is oracle.loss_computer, on the truth's outputs and
    on a batch of replicas of them (the loss truth of a batch of the sweep)."""
    from diffusiondrive_amd.config import TransfuserConfig
    cfg = TransfuserConfig()
    _, _, tg = scenes
    anchor = seeded_sd["_trajectory_head.plan_anchor"]
    for l in range(2):
        for B in (5, 13):
            idx = U.replica_index(B)
            reg, cls = truth[f"reg_l{l}"][idx], truth[f"cls_l{l}"][idx]
            part = T.scene_partials64(reg, cls, tg[idx], anchor)
            tot = (cfg.trajectory_cls_weight * part[:, 0].sum() / (B * T.Q)
                   + cfg.trajectory_reg_weight * part[:, 1].sum() / (B * T.P * 3))
            ref = T.loss64(reg, cls, tg[idx], anchor)
            assert abs(tot - ref) <= 1e-12 * abs(ref), (l, B, tot, ref)
        assert abs(T.loss64(truth[f"reg_l{l}"], truth[f"cls_l{l}"], tg, anchor) - float(truth[f"loss_{l}"])) <= 1e-12


# --------------------------------------------------------------------------- the doctored cases
def _case(seeded_sd, case_features, name, dtype=np.float64):
    sd, inp, t, tg = T.make_train_case(seeded_sd, name)
    return sd, inp, t, tg, T.oracle_train(sd, inp, t, tg, dtype, features=case_features[dtype])


def test_shared_features_equal_a_whole_forward(seeded_sd, case_features):
    """oracle_train on shared features is the whole forward_train (the cases edit the trajectory head only)."""
    sd, inp, t, tg = T.make_train_case(seeded_sd, "saturated_cls_pos")
    a = T.oracle_train(sd, inp, t, tg, np.float32, features=case_features[np.float32])
    b = T.oracle_train(sd, inp, t, tg, np.float32)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert T.CASE_TIMESTEPS == (49, 0)
    assert T.TRAIN_CASES == ("equal_modes", "tied_anchors", "clamp_noise", "saturated_cls_pos", "saturated_cls_neg")


def test_equal_modes_ties_every_anchor_distance(seeded_sd, case_features):
    """Every anchor equals anchor 7: the 20 mean distances are one value, LossComputer's class target is mode 0 (the
    first minimum), the oracle's rows agree to rounding and its trajectory is mode 0's row to rounding."""
    sd, inp, t, tg, ref = _case(seeded_sd, case_features, "equal_modes")
    mode, dist = T.nearest_modes(tg, sd["_trajectory_head.plan_anchor"])
    assert (dist == dist[:, :1]).all() and mode.tolist() == [0, 0]
    tt = torch.as_tensor(tg.astype(np.float64))
    a = torch.as_tensor(sd["_trajectory_head.plan_anchor"].astype(np.float64))
    assert torch.linalg.norm(tt[:, None, :, :2] - a[None], dim=-1).mean(-1).argmin(-1).tolist() == [0, 0]
    for l in range(2):
        for k in ("reg", "cls"):
            v = ref[f"{k}_l{l}"]
            assert np.abs(v - v[:, :1]).max() <= 1e-10, (k, l)
    assert np.abs(ref["trajectory"] - ref["reg_l1"][:, 0]).max() <= 1e-10


def test_tied_anchors_tell_the_modes_apart(seeded_sd, case_features):
    """equal_modes' anchors with the noise as drawn: the 20 distances still tie (class target mode 0), the modes' rows
    differ, and both per-scene sums under any other class target - the last minimum, mode 19, among them - are more
    than ten times the GPU test's bar (1e-5 * max(1, |ref|)) from mode 0's: an argmin that does not take the first
    minimum cannot pass."""
    sd, inp, t, tg, ref = _case(seeded_sd, case_features, "tied_anchors")
    anchor = sd["_trajectory_head.plan_anchor"]
    mode, dist = T.nearest_modes(tg, anchor)
    assert (dist == dist[:, :1]).all() and mode.tolist() == [0, 0]
    assert not (inp["noise"] == inp["noise"][:, :1]).all()
    for l in range(2):
        p0 = T.scene_partials64(ref[f"reg_l{l}"], ref[f"cls_l{l}"], tg, anchor)
        for m in range(1, T.Q):
            pm = T.scene_partials64(ref[f"reg_l{l}"], ref[f"cls_l{l}"], tg, anchor, mode=[m, m])
            assert (np.abs(pm - p0) > 10 * 1e-5 * np.maximum(1.0, np.abs(p0))).all(), (l, m, pm, p0)


def test_clamp_noise_clamps_scene_1_under_its_own_coefficients(seeded_sd, case_features):
    """Scene 1 (t = 0: sqrt(1 - a) = 0.01 against scene 0's 0.094 at t = 49) with its noise x 40: about a quarter of its
    coordinates clamp, at all four bounds (x = 55.7 / -1.2, y = 26 / -20), the rest stay inside; under scene 0's
    coefficients three quarters would clamp and points would move by tens of metres, so a coefficient taken from the
    neighbouring scene cannot pass. The fp32 oracle stays within half the bars of the float64 one."""
    from oracle.model import DDIM, denorm_odo, norm_odo
    sd, inp, t, tg, ref = _case(seeded_sd, case_features, "clamp_noise")
    a = torch.as_tensor(sd["_trajectory_head.plan_anchor"].astype(np.float64))[None]
    nz = torch.as_tensor(inp["noise"].astype(np.float64))
    ac = DDIM(dtype=torch.float64).ac[torch.as_tensor(t)].view(2, 1, 1, 1)
    img = ac ** 0.5 * norm_odo(a) + (1 - ac) ** 0.5 * nz
    frac = (img.abs() > 1).double().mean((1, 2, 3))
    assert 0.15 <= float(frac[1]) <= 0.35 and float(frac[0]) > 0, frac
    pts = denorm_odo(img.clamp(-1, 1))[1]
    assert np.isclose(float(pts[..., 0].max()), 55.7) and np.isclose(float(pts[..., 0].min()), -1.2)
    assert np.isclose(float(pts[..., 1].max()), 26.0) and np.isclose(float(pts[..., 1].min()), -20.0)
    sw = ac.flip(0)
    img_sw = sw ** 0.5 * norm_odo(a) + (1 - sw) ** 0.5 * nz
    assert float((img_sw[1].abs() > 1).double().mean()) > 0.6
    assert float((denorm_odo(img_sw.clamp(-1, 1))[1] - pts).abs().max()) > 10.0
    r32 = _case(seeded_sd, case_features, "clamp_noise", np.float32)[-1]
    for k, v in T.train_errors(_outs(r32), _outs(ref)).items():
        assert v <= 0.5 * _bar(k), (k, v)


@pytest.mark.parametrize("name", ["saturated_cls_pos", "saturated_cls_neg"])
def test_saturated_cls_keeps_the_focal_loss_well_conditioned(seeded_sd, case_features, name):
    """plan_cls_branch.6.bias of both layers shifted by +-60: every logit is beyond +-58 (sigmoid 1 - 1e-26 / 1e-26:
    (1 - sigmoid) and its square are 0 or below the smallest fp32 subnormal), and the fp32 oracle's focal loss is
    within 1e-5 relative of the float64 one at that shift (measured: <= 5.4e-8), everything finite."""
    from oracle.model import sigmoid_focal_loss
    assert T.SATURATION == 60.0
    sd, inp, t, tg, r64 = _case(seeded_sd, case_features, name)
    r32 = _case(seeded_sd, case_features, name, np.float32)[-1]
    mode = T.nearest_modes(tg, sd["_trajectory_head.plan_anchor"])[0]
    onehot = np.zeros((2, T.Q))
    onehot[np.arange(2), mode] = 1
    sign = 1.0 if name.endswith("pos") else -1.0
    for l in range(2):
        assert (sign * r64[f"cls_l{l}"] > 58.0).all()
        f32 = float(sigmoid_focal_loss(torch.as_tensor(r32[f"cls_l{l}"]), torch.as_tensor(onehot.astype(np.float32))))
        f64 = float(sigmoid_focal_loss(torch.as_tensor(r64[f"cls_l{l}"]), torch.as_tensor(onehot)))
        print(f"{name} layer {l}: focal fp32 {f32:.9g} float64 {f64:.9g}")
        assert np.isfinite(f32) and f64 > 0 and abs(f32 - f64) <= 1e-5 * f64, (l, f32, f64)
        assert np.isfinite(float(r32[f"loss_{l}"]))
        assert abs(float(r32[f"loss_{l}"]) - float(r64[f"loss_{l}"])) <= 1e-5 * float(r64[f"loss_{l}"])
