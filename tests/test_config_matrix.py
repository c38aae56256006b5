"""CPU companion of test_config_matrix_gpu.py: what dd_create accepts and refuses, and the premises of the GPU test.

The rule ("Configuration matrix"): a dd_config either passes dd_create and then matches the
float64 oracle at the parity bars (the GPU test), or dd_create returns DD_ERR_INVALID with a message naming the field,
before the blob is parsed and before any device call. The rejections run here on a machine without a GPU, as
test_host.test_abi_errors_without_gpu_work does: the default config with one field changed and an 8-byte blob that is
no weight blob. A refused field's message names the field; an accepted value gets as far as the blob and fails on
that.

Premises of the GPU test, per case of config_matrix_util.CASES: the state dict, the inputs and the schema agree on
shapes; the fp32 oracle is within half of every bar of the float64 oracle on the test's own scenes (the bars leave
room for the GPU's rounding); and the cases are not degenerate - permuting the LiDAR channels of the input moves the
trajectory by more than 100 x the waypoint bar, at 33 and 64 modes a scene selects another mode than 0, and the start
of the denoising at trunc_timestep = 999 has clamped coordinates.
"""
import ctypes

import numpy as np
import pytest

import config_matrix_util as C
from test_parity_gpu import AGENT_TOL, HEADING_TOL, MODE_TOL, TAP_TOL, WAYPOINT_L2_TOL

BARS = dict(waypoint=WAYPOINT_L2_TOL, heading=HEADING_TOL, mode=MODE_TOL, agent=AGENT_TOL, tap=TAP_TOL)
DUMMY_BLOB = b"XXXX\0\0\0\0"

REJECTED = [("lidar_arch", 50), ("lidar_arch", 18), ("image_arch", 18), ("lidar_channels", 0), ("lidar_channels", 5),
            ("num_poses", 4), ("num_poses", 9), ("num_poses", 16), ("num_modes", 0), ("num_modes", -1),
            ("num_modes", C.MAX_MODES + 1), ("trunc_timestep", -1), ("trunc_timestep", 1000), ("step_span", 0),
            ("step_span", 1001)]
ACCEPTED = [("lidar_channels", 1), ("lidar_channels", 2), ("lidar_channels", 3), ("lidar_channels", 4),
            ("num_modes", 1), ("num_modes", C.MAX_MODES), ("trunc_timestep", 0), ("trunc_timestep", 999),
            ("step_span", 1), ("step_span", 1000), ("image_arch", 50)]
FIELDS = sorted({f for f, _ in REJECTED})


def _create(field, value):
    """dd_create of the default config with one field changed on the dummy blob: (return code, message)."""
    from diffusiondrive_amd import _lib
    lib = _lib.load()
    cfg = _lib.DDConfig()
    lib.dd_default_config(ctypes.byref(cfg))
    setattr(cfg, field, value)
    h = ctypes.c_void_p()
    rc = lib.dd_create(ctypes.byref(cfg), DUMMY_BLOB, len(DUMMY_BLOB), 0, ctypes.byref(h))
    assert not h.value
    return rc, lib.dd_last_error().decode()


@pytest.mark.parametrize("field,value", REJECTED, ids=[f"{f}={v}" for f, v in REJECTED])
def test_dd_create_rejects(field, value):
    """DD_ERR_INVALID with the field's name and the value in the message; nothing about the blob, which is not read."""
    rc, msg = _create(field, value)
    assert rc == -1, (rc, msg)
    assert field in msg and str(value) in msg, msg
    assert [f for f in FIELDS if f in msg] == [field], msg


@pytest.mark.parametrize("field,value", ACCEPTED, ids=[f"{f}={v}" for f, v in ACCEPTED])
def test_dd_create_accepts(field, value):
    """An accepted value passes the validation: the dummy blob then fails as a blob, and the message names no config
    field."""
    rc, msg = _create(field, value)
    assert rc == -1, (rc, msg)
    assert "blob" in msg.lower() or "DDW1" in msg, msg
    assert not [f for f in FIELDS if f in msg], msg


def test_default_config_is_accepted():
    from diffusiondrive_amd import _lib
    lib = _lib.load()
    cfg = _lib.DDConfig()
    lib.dd_default_config(ctypes.byref(cfg))
    h = ctypes.c_void_p()
    assert lib.dd_create(ctypes.byref(cfg), DUMMY_BLOB, len(DUMMY_BLOB), 0, ctypes.byref(h)) == -1
    msg = lib.dd_last_error().decode()
    assert ("blob" in msg.lower() or "DDW1" in msg) and not [f for f in FIELDS if f in msg], msg


def test_python_side_refuses_what_dd_create_refuses():
    """state_dict_schema emits no schema for another pose count (its anchor encoder would stay 512 wide), and
    make_dd_config refuses a ResNet-50 LiDAR trunk and an unknown image trunk before the library is asked."""
    from diffusiondrive_amd.config import TrajectorySampling, TransfuserConfig
    from diffusiondrive_amd.model import make_dd_config
    from diffusiondrive_amd.schema import state_dict_schema
    from diffusiondrive_amd.weights import seeded_state_dict
    for horizon in (2.0, 4.5, 8.0):  # 4, 9 and 16 poses
        cfg = TransfuserConfig(trajectory_sampling=TrajectorySampling(time_horizon=horizon))
        assert cfg.trajectory_sampling.num_poses != 8
        with pytest.raises(ValueError, match="num_poses"):
            state_dict_schema(cfg)
        with pytest.raises(ValueError, match="num_poses"):
            seeded_state_dict(cfg, 0)
    with pytest.raises(ValueError, match="lidar_architecture"):
        make_dd_config(TransfuserConfig(lidar_architecture="resnet50"))
    with pytest.raises(ValueError, match="image_architecture"):
        make_dd_config(TransfuserConfig(image_architecture="resnet18"))
    c = make_dd_config(TransfuserConfig(image_architecture="resnet50", use_ground_plane=True, lidar_seq_len=2))
    assert (c.image_arch, c.lidar_arch, c.lidar_channels, c.num_poses) == (50, 34, 4, 8)


# --------------------------------------------------------------------------- premises of the GPU test
@pytest.mark.parametrize("case", list(C.CASES))
def test_case_shapes_agree(case):
    """The case's state dict passes the strict key / shape check of its config, and its inputs, timesteps and targets
    have the shapes the forward asks for."""
    from diffusiondrive_amd.model import check_state_dict
    cfg = C.case_config(case)
    sd = C.case_state_dict(case)
    assert check_state_dict(sd, cfg) == ([], [])
    inp, t, tg = C.case_inputs(case)
    Q = cfg.num_modes
    assert inp["camera_feature"].shape == (C.BATCH, 3, 256, 1024)
    assert inp["lidar_feature"].shape == (C.BATCH, cfg.lidar_in_channels, 256, 256)
    assert inp["status_feature"].shape == (C.BATCH, 8) and inp["noise"].shape == (C.BATCH, Q, 8, 2)
    assert sd["_trajectory_head.plan_anchor"].shape == (Q, 8, 2)
    assert sd["_backbone.lidar_encoder.conv1.weight"].shape == (64, cfg.lidar_in_channels, 7, 7)
    assert t.shape == (C.BATCH,) and tg.shape == (C.BATCH, 8, 3)
    steps, schedule = C.case_steps(case)
    assert 1 <= steps <= (1000 if schedule == "vanilla" else cfg.step_span)
    roll = C.roll_of(case)
    assert len(roll) == steps and roll[-1] == 0 and all(0 <= k <= 999 for k in roll)


def test_the_rolls_are_the_ones_the_cases_are_there_for():
    """steps3 / steps7 round where truncation gives another timestep, trunc999_span1000 rolls 750 .. 0, steps20 visits
    every timestep of the span and vanilla3's ratio does not divide 1000."""
    assert C.roll_of("steps3") == [13, 7, 0] and [int(s * 20 / 3) for s in range(3)][::-1] == [13, 6, 0]
    assert C.roll_of("steps7") == [17, 14, 11, 9, 6, 3, 0]
    assert [int(s * 20 / 7) for s in range(7)][::-1] != C.roll_of("steps7")
    assert C.roll_of("steps20") == list(range(19, -1, -1))
    assert C.roll_of("trunc999_span1000") == [750, 500, 250, 0]
    assert C.roll_of("trunc0_span1") == [0]
    assert C.roll_of("vanilla3") == [666, 333, 0] and C.roll_of("vanilla1") == [0]


_TRUNKS = {}


def _trunk(case, dtype):
    """The oracle before the trajectory head, once per (trunk, dtype)."""
    key = (C.trunk_key(case), dtype)
    if key not in _TRUNKS:
        _TRUNKS[key] = C.oracle_trunk(C.case_state_dict(case), C.case_inputs(case)[0], C.case_config(case), dtype)
    return _TRUNKS[key]


@pytest.mark.parametrize("case", list(C.CASES))
def test_fp32_oracle_is_within_half_of_every_bar(case):
    """The fp32 oracle against the float64 oracle on the case's own scenes, every output and tap at every (step, layer)
    the case runs: at most half of its bar, so the bars the GPU test holds leave room for the GPU's own rounding. A
    condition on the inputs: a case that misses it gets other scenes, not another bar."""
    cfg, sd, (inp, _, _) = C.case_config(case), C.case_state_dict(case), C.case_inputs(case)
    steps, schedule = C.case_steps(case)
    r64 = C.oracle_case(sd, inp, cfg, steps, schedule, np.float64, _trunk(case, np.float64))
    r32 = C.oracle_case(sd, inp, cfg, steps, schedule, np.float32, _trunk(case, np.float32))
    errs = C.errors(r32, r64)
    print(f"== config matrix premise {case}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert {f"{k}_s{s}l{l}" for s, l in C.step_layers(case) for k in ("gs", "reg", "cls")} <= set(errs)
    for k, v in errs.items():
        assert v <= 0.5 * C.bar_of(k, BARS), (case, k, v, C.bar_of(k, BARS))
    if case in ("modes33", "modes64"):
        # the argmax is taken: a kernel that always returned mode 0 would differ
        sel = r64["poses_cls"].argmax(-1)
        assert (sel != 0).any(), sel
    if case == "trunc999_span1000":
        img = C.start_image(sd, inp, cfg)
        assert (np.abs(img) > 1.0).any()


@pytest.mark.parametrize("case", C.LIDAR_CASES)
def test_lidar_channels_matter(case):
    """Reading the LiDAR channels in another order (the first channel moved to the end) moves the fp32 oracle's
    trajectory by more than 100 x the waypoint bar: a stem that swapped, dropped or repeated a channel cannot pass."""
    cfg, sd, (inp, _, _) = C.case_config(case), C.case_state_dict(case), C.case_inputs(case)
    steps, schedule = C.case_steps(case)
    ref = C.oracle_case(sd, inp, cfg, steps, schedule, np.float32, _trunk(case, np.float32))
    perm = dict(inp, lidar_feature=np.ascontiguousarray(np.roll(inp["lidar_feature"], -1, axis=1)))
    assert not np.array_equal(perm["lidar_feature"], inp["lidar_feature"])
    got = C.oracle_case(sd, perm, cfg, steps, schedule, np.float32)
    d = (got["trajectory"][..., :2].astype(np.float64) - ref["trajectory"][..., :2]).reshape(C.BATCH, -1)
    l2 = np.sqrt((d ** 2).sum(-1))
    print(f"== config matrix premise {case}: LiDAR channels rolled, waypoint L2 per scene {l2}")
    assert l2.max() > 100 * WAYPOINT_L2_TOL, l2
