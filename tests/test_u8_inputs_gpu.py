"""uint8 camera / LiDAR features read in place by the stems (dd_inputs, dd_forward_in and its siblings) on the GPU.

Both features are byte-valued by construction (camera k / 255, LiDAR min(c, hist_max) / hist_max). In every test the
float inputs are made from the bytes by ``t.float().div(255)`` and ``(c.clamp(max=hm).double() / hm).float()``; the float
path then computes today's result and ``torch.equal`` is the bar: the stems see identical fp32 values, so no tolerance
applies anywhere."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HM = 5  # TransfuserConfig.hist_max_per_pixel


def _bytes(B, C=1, seed=0):
    """B scenes of feature bytes: a camera image (B, 256, 1024, 3) over all 256 values, sparse LiDAR counts
    (B, C, 256, 256) in 0..9 (values above every hist_max used here, so the clip is exercised)."""
    g = torch.Generator().manual_seed(1000 + seed)
    cam = torch.randint(0, 256, (B, 256, 1024, 3), generator=g, dtype=torch.uint8)
    cam.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    lid = torch.randint(0, 10, (B, C, 256, 256), generator=g, dtype=torch.uint8)
    lid = lid * (torch.rand(lid.shape, generator=g) < 0.15).to(torch.uint8)
    st = torch.randn(B, 8, generator=g)
    nz = torch.randn(B, 20, 8, 2, generator=g)
    return cam, lid, st, nz


def _widen_cam(cam):
    return cam.permute(0, 3, 1, 2).float().div(255).contiguous()


def _widen_lid(lid, hm=HM):
    return (lid.clamp(max=hm).double() / hm).float()


def _feats(cam, lid, st, cam_u8=True, lid_u8=True, hm=HM):
    return {"camera_feature": (cam if cam_u8 else _widen_cam(cam)).to(DEV),
            "lidar_feature": (lid if lid_u8 else _widen_lid(lid, hm)).to(DEV), "status_feature": st.to(DEV)}


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, (list, tuple)):
            assert all(torch.equal(x, y) for x, y in zip(va, vb)), k
        elif isinstance(va, dict):
            assert all(torch.equal(va[n], vb[n]) for n in va), k
        else:
            assert torch.equal(va, vb), k


@pytest.fixture(scope="module")
def model(gpu, seeded_sd):
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    yield m
    m.close()


@pytest.fixture(scope="module")
def two():
    return _bytes(2)


# ---------------------------------------------------------------------------------------------- 1. the stem op
def _luts(hm):
    k = torch.arange(256)
    return k.float().div(255), (k.clamp(max=hm).double() / hm).float()


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("layout,B,C,H,W,hm,one", [
    ("hwc", 2, 3, 37, 53, 0, False),     # odd row bytes, odd image stride, tiles over every edge, batch stride % 4 != 0
    ("planar", 2, 1, 40, 40, 5, False),
    ("planar", 2, 1, 40, 40, 3, True),   # the opt-in one-channel kernel form
    ("planar", 2, 2, 37, 53, 3, False),
    ("planar", 2, 3, 40, 40, 3, False),
    ("hwc", 1, 3, 27, 40, 0, False),     # one input patch: its halo lies wholly outside the map
    ("planar", 1, 1, 27, 40, 5, False),
])
def test_stem_op_bits(gpu, monkeypatch, layout, B, C, H, W, hm, one, prec):
    """dd_op_stem_pool_u8 on the bytes equals dd_op_stem_pool_nchw on the widened tensor bit for bit."""
    from diffusiondrive_amd import _lib
    monkeypatch.setenv("DDMI_STEM1", "1" if one else "0")
    g = torch.Generator().manual_seed(7 * H + W + C)
    cam_lut, lid_lut = _luts(hm or 5)
    if layout == "hwc":
        x = torch.randint(0, 256, (B, H, W, C), generator=g, dtype=torch.uint8)
        x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
        lut = cam_lut
        wide = lut[x.long()].permute(0, 3, 1, 2).contiguous()
        assert torch.equal(wide, x.permute(0, 3, 1, 2).float().div(255))
    else:
        x = torch.randint(0, 9, (B, C, H, W), generator=g, dtype=torch.uint8)  # counts above hist_max present
        lut = lid_lut
        wide = lut[x.long()].contiguous()
        assert torch.equal(wide, (x.clamp(max=hm).double() / hm).float()) and int(x.max()) > hm
    w = (torch.rand(64, 7, 7, 4, generator=g) - 0.5) * (2.0 / np.sqrt(49 * C))
    w[..., C:] = 0.0
    b = torch.rand(64, generator=g) - 0.5
    hs, ws = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    hp, wp = (hs + 2 - 3) // 2 + 1, (ws + 2 - 3) // 2 + 1
    # the uint8 tensor one byte into its allocation: no alignment is assumed of the bytes
    raw = torch.empty(x.numel() + 1, dtype=torch.uint8, device=DEV)
    raw[1:] = x.reshape(-1).to(DEV)
    xd, wd, bd, ld, fd = raw[1:], w.to(DEV), b.to(DEV), lut.to(DEV), wide.to(DEV)
    out_u = torch.full((B, hp, wp, 64), float("nan"), device=DEV)
    out_f = torch.full((B, hp, wp, 64), float("nan"), device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _lib.check(gpu.dd_op_stem_pool_nchw(fd.data_ptr(), B, C, H, W, wd.data_ptr(), bd.data_ptr(), out_f.data_ptr(), prec,
                                        flags.data_ptr(), None), gpu, op=True)
    _lib.check(gpu.dd_op_stem_pool_u8(xd.data_ptr(), 0 if layout == "hwc" else 1, B, C, H, W, ld.data_ptr(),
                                      wd.data_ptr(), bd.data_ptr(), out_u.data_ptr(), prec, flags.data_ptr(), None),
               gpu, op=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_f).all()) and float(out_f.abs().max()) > 0
    assert torch.equal(out_u, out_f)
    assert int(flags.item()) == 0


# ---------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("mode", ["f16x3", "bf16", "fp32"])
def test_forward_equals_float_path(model, two, mode):
    """forward on uint8 features == forward on the widened floats for every output, in every gemm mode; so does the
    mixed call (uint8 camera, float LiDAR) and safe=True."""
    cam, lid, st, nz = two
    model.set_gemm_mode(mode)
    try:
        ref = model.forward(_feats(cam, lid, st, False, False), noise=nz, heads=True, modes=True)
        out = model.forward(_feats(cam, lid, st), noise=nz, heads=True, modes=True)
        mixed = model.forward(_feats(cam, lid, st, True, False), noise=nz, heads=True, modes=True)
        mixed2 = model.forward(_feats(cam, lid, st, False, True), noise=nz, heads=True, modes=True)
        safe = model.forward(_feats(cam, lid, st), noise=nz, heads=True, modes=True, safe=True)
        torch.cuda.synchronize()
    finally:
        model.set_gemm_mode("f16x3")
    assert model.numerics_flags() == 0
    assert sorted(ref) == ["agent_labels", "agent_states", "bev_semantic_map", "poses_cls", "poses_reg", "trajectory"]
    assert bool(torch.isfinite(ref["trajectory"]).all())
    for o in (out, mixed, mixed2, safe):
        _same(o, ref)


# ---------------------------------------------------------------------------------------------- 3. replay
def test_replay_follows_the_callers_buffers(model, two):
    """One handle, two uint8 batches at different addresses: the captured program reads the second call's buffers;
    float and uint8 calls alternate on the handle, one program per (shape, kinds), kernel nodes only."""
    m = model.clone()
    try:
        cam1, lid1, st1, nz1 = two
        cam2, lid2, st2, nz2 = _bytes(2, seed=1)
        u1, u2 = _feats(cam1, lid1, st1), _feats(cam2, lid2, st2)
        f1, f2 = _feats(cam1, lid1, st1, False, False), _feats(cam2, lid2, st2, False, False)
        assert u1["camera_feature"].data_ptr() != u2["camera_feature"].data_ptr()
        m.forward(u1, noise=nz1)                       # eager
        a1 = m.forward(u1, noise=nz1)                  # captured
        assert m.graph_info()["programs"] == 1
        a2 = m.forward(u2, noise=nz2)                  # replayed on the other buffers
        m.forward(f1, noise=nz1)
        r1 = m.forward(f1, noise=nz1)
        r2 = m.forward(f2, noise=nz2)
        info = m.graph_info()
        assert info["programs"] == 2 and info["other_nodes"] == 0 and info["multi_stream_execs"] == 0, info
        b2 = m.forward(u2, noise=nz2)                  # a uint8 call after float calls: its own program again
        c1 = m.forward(f1, noise=nz1)
        torch.cuda.synchronize()
        assert m.graph_info()["programs"] == 2
        assert not torch.equal(r1["trajectory"], r2["trajectory"])
        _same(a1, r1)
        _same(a2, r2)
        _same(b2, r2)
        _same(c1, r1)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- 4. byte strides
@pytest.fixture(scope="module")
def chunk_model(gpu, seeded_sd):
    """A handle whose forwards run in chunks of at most 4 scenes (DDMI_MAX_CHUNK is read at dd_create)."""
    from diffusiondrive_amd.model import DiffusionDriveModel
    mp = pytest.MonkeyPatch()
    mp.setenv("DDMI_MAX_CHUNK", "4")
    try:
        m = DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3")
    finally:
        mp.undo()
    yield m
    m.close()


def test_uneven_chunks(chunk_model):
    """B = 5 under a chunk limit of 4 runs as 3 + 2 scenes: the second chunk starts 3 scenes of BYTES into the uint8
    tensors. Five distinct scenes, so a chunk read at the wrong offset shows."""
    cam, lid, st, nz = _bytes(5, seed=2)
    ref = chunk_model.forward(_feats(cam, lid, st, False, False), noise=nz, heads=True, modes=True)
    out = chunk_model.forward(_feats(cam, lid, st), noise=nz, heads=True, modes=True)
    mixed = chunk_model.forward(_feats(cam, lid, st, False, True), noise=nz, heads=True, modes=True)
    torch.cuda.synchronize()
    assert len({tuple(t.flatten().tolist()) for t in ref["trajectory"]}) == 5
    _same(out, ref)
    _same(mixed, ref)


def test_samples_and_train(chunk_model, two):
    """forward_samples (B = 2, S = 3: head passes of one scene under the chunk limit) and forward_train with targets
    on uint8 features equal their float calls bit for bit."""
    cam, lid, st, _ = two
    g = torch.Generator().manual_seed(5)
    nz = torch.randn(2, 3, 20, 8, 2, generator=g)
    ref = chunk_model.forward_samples(_feats(cam, lid, st, False, False), 3, noise=nz, heads=True, modes=True, best=True)
    out = chunk_model.forward_samples(_feats(cam, lid, st), 3, noise=nz, heads=True, modes=True, best=True)
    torch.cuda.synchronize()
    _same(out, ref)
    tn = torch.randn(2, 20, 8, 2, generator=g)
    ts = torch.tensor([3, 41])
    tg = {"trajectory": torch.randn(2, 8, 3, generator=g)}
    ref = chunk_model.forward_train(_feats(cam, lid, st, False, False), tg, timesteps=ts, noise=tn)
    out = chunk_model.forward_train(_feats(cam, lid, st), tg, timesteps=ts, noise=tn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref["trajectory_loss"]))
    _same(out, ref)


# ---------------------------------------------------------------------------------------------- 5. hist_max
def test_hist_max_follows_the_call(model, two):
    """hist_max 5, then 3, then 5 again on one handle: the LiDAR table is rewritten ahead of the forward that needs
    it, and each call equals the float path at its own hist_max."""
    cam, lid, st, nz = two
    cfg0 = model.config
    res = {}
    try:
        for i, hm in enumerate((5, 3, 5)):
            model.config = dataclasses.replace(cfg0, hist_max_per_pixel=hm)
            res[i] = (model.forward(_feats(cam, lid, st, hm=hm), noise=nz, heads=True),
                      model.forward(_feats(cam, lid, st, False, False, hm=hm), noise=nz, heads=True))
        torch.cuda.synchronize()
    finally:
        model.config = cfg0
    for out, ref in res.values():
        _same(out, ref)
    assert not torch.equal(res[0][1]["trajectory"], res[1][1]["trajectory"])
    _same(res[2][0], res[0][1])


# ---------------------------------------------------------------------------------------------- 6. builders
def test_builders_write_the_bytes(model):
    """dd_build_camera_u8 / dd_build_lidar_u8: widened (and the camera permuted) they equal the float builders'
    outputs, and a forward fed with them equals a forward fed with the float features."""
    from diffusiondrive_amd.features import camera_features, lidar_features
    cfg = model.config
    r = np.random.default_rng(3)
    imgs = [tuple(r.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(3))]
    cam_f = camera_features(imgs, cfg, 0)
    cam_u = camera_features(imgs, cfg, 0, dtype=torch.uint8)
    assert cam_u.dtype == torch.uint8 and tuple(cam_u.shape) == (1, 256, 1024, 3)
    # widened on the CPU: torch's GPU division by a scalar multiplies by the reciprocal, which is not k / 255.f
    assert torch.equal(_widen_cam(cam_u.cpu()), cam_f.cpu())
    # a cloud that piles points up: counts far above hist_max, in-range and out-of-range points, bins shared by words
    xy = np.concatenate([r.uniform(-32, 32, (2, 4000)), np.repeat(r.uniform(-33, 33, (2, 300)), 9, axis=1)], axis=1)
    pts = [np.concatenate([xy, r.uniform(-1, 3, (1, xy.shape[1]))]).astype(np.float32)]
    lid_f = lidar_features(pts, cfg, 0)
    lid_u = lidar_features(pts, cfg, 0, dtype=torch.uint8)
    assert lid_u.dtype == torch.uint8 and tuple(lid_u.shape) == tuple(lid_f.shape)
    assert int(lid_u.max()) == HM and int((lid_u == 1).sum()) > 0 and int((lid_u == 0).sum()) > 0
    assert torch.equal(_widen_lid(lid_u.cpu()), lid_f.cpu())
    with pytest.raises(ValueError, match="dtype"):
        camera_features(imgs, cfg, 0, dtype=torch.float16)
    g = torch.Generator().manual_seed(9)
    st, nz = torch.randn(1, 8, generator=g).to(DEV), torch.randn(1, 20, 8, 2, generator=g)
    ref = model.forward({"camera_feature": cam_f, "lidar_feature": lid_f, "status_feature": st}, noise=nz, heads=True)
    out = model.forward({"camera_feature": cam_u, "lidar_feature": lid_u, "status_feature": st}, noise=nz, heads=True)
    torch.cuda.synchronize()
    _same(out, ref)


# ---------------------------------------------------------------------------------------------- 7. errors
def test_bad_descriptors_are_refused(gpu, model, two):
    """Both or neither pointer of a sensor, hist_max 0 / 256: DD_ERR_INVALID with the field named, nothing launched;
    the handle then runs a valid forward. A wrong-shaped uint8 tensor is a ValueError in Python."""
    from diffusiondrive_amd import _lib
    cam, lid, st, nz = two
    u = _feats(cam, lid, st)
    f = _feats(cam, lid, st, False, False)
    nzd = nz.to(DEV)
    traj = torch.zeros(2, 8, 3, device=DEV)
    outs = _lib.DDOutputs()
    outs.trajectory = traj.data_ptr()

    def call(**kw):
        ins = _lib.DDInputs()
        ins.status, ins.noise = u["status_feature"].data_ptr(), nzd.data_ptr()
        for k, v in kw.items():
            setattr(ins, k, v)
        rc = gpu.dd_forward_in(model.handle, ctypes.byref(ins), 2, 2, ctypes.byref(outs), None)
        return rc, gpu.dd_last_error().decode()

    cu, cf = u["camera_feature"].data_ptr(), f["camera_feature"].data_ptr()
    lu, lf = u["lidar_feature"].data_ptr(), f["lidar_feature"].data_ptr()
    torch.cuda.synchronize()
    for kw, field in [(dict(camera_u8=cu, camera_f32=cf, lidar_f32=lf), "camera_u8"),
                      (dict(lidar_f32=lf), "camera_f32"),
                      (dict(camera_u8=cu, lidar_u8=lu, lidar_f32=lf, lidar_hist_max=5), "lidar_u8"),
                      (dict(camera_u8=cu), "lidar_f32"),
                      (dict(camera_u8=cu, lidar_u8=lu, lidar_hist_max=0), "lidar_hist_max"),
                      (dict(camera_f32=cf, lidar_u8=lu, lidar_hist_max=256), "lidar_hist_max")]:
        rc, msg = call(**kw)
        assert rc == -1 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert float(traj.abs().max()) == 0.0  # nothing ran
    rc, msg = call(camera_u8=cu, lidar_u8=lu, lidar_hist_max=5)
    assert rc == 0, msg
    ref = model.forward(f, noise=nz)
    torch.cuda.synchronize()
    assert torch.equal(traj, ref["trajectory"])
    for bad in (cam.permute(0, 3, 1, 2).contiguous(), cam[:, :, :, :2].contiguous(), cam[:, :128].contiguous()):
        with pytest.raises(ValueError, match="uint8 camera_feature"):
            model.forward({**u, "camera_feature": bad.to(DEV)}, noise=nz)
    with pytest.raises(ValueError, match="lidar_feature"):
        model.forward({**u, "lidar_feature": lid[:, :, :128].contiguous().to(DEV)}, noise=nz)


# ---------------------------------------------------------------------------------------------- 8. four channels
def test_four_lidar_channels_transposing_route(gpu):
    """lidar_channels = 4 (the NHWC4 transposing route in every mode, elementwise.hip's uint8 passes): B = 1, f16x3,
    equals the float path."""
    from diffusiondrive_amd.config import TransfuserConfig
    from diffusiondrive_amd.model import DiffusionDriveModel
    from diffusiondrive_amd.weights import seeded_state_dict
    cfg = TransfuserConfig(lidar_seq_len=4)
    assert cfg.lidar_in_channels == 4
    m = DiffusionDriveModel(cfg, seeded_state_dict(cfg, 0), device=0, gemm="f16x3")
    try:
        cam, lid, st, nz = _bytes(1, C=4, seed=4)
        ref = m.forward(_feats(cam, lid, st, False, False), noise=nz, heads=True, modes=True)
        out = m.forward(_feats(cam, lid, st), noise=nz, heads=True, modes=True)
        out2 = m.forward(_feats(cam, lid, st), noise=nz, heads=True, modes=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ref["trajectory"]).all())
        _same(out, ref)
        _same(out2, ref)
    finally:
        m.close()
