"""Every kind of forward call interleaved on one handle, with refused calls between them.

A call (plain, with heads, S samples, best, training without / with targets, uint8 inputs) is one value that travels
down the forward path as an argument: nothing of it may stay on the handle. So whatever ran before, and whether it ran
or was refused, the plain forward of the same inputs returns the same bits, and every kind owns exactly one captured
program per chunk size. The handle is built under DDMI_MAX_CHUNK=2, so the B = 3 calls run as uneven chunks of 2 + 1
and an S = 2 chunk of two scenes takes two head passes."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, Q, P = 3, 20, 8
HM = 5  # TransfuserConfig.hist_max_per_pixel


def _chunked(make):
    """``make()`` with DDMI_MAX_CHUNK=2 set (read at dd_create)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("DDMI_MAX_CHUNK", "2")
    try:
        return make()
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def handle(gpu, seeded_sd):
    from diffusiondrive_amd.model import DiffusionDriveModel
    m = _chunked(lambda: DiffusionDriveModel(state_dict=seeded_sd, device=0, gemm="f16x3"))
    yield m
    m.close()


@pytest.fixture(scope="module")
def scenes():
    """Three distinct seeded scenes as feature bytes, the float features those bytes stand for (the float and the
    uint8 calls then see the same values), and every kind's other inputs."""
    g = torch.Generator().manual_seed(4242)
    cam = torch.randint(0, 256, (B, 256, 1024, 3), generator=g, dtype=torch.uint8)
    lid = torch.randint(0, 10, (B, 1, 256, 256), generator=g, dtype=torch.uint8)
    lid = lid * (torch.rand(lid.shape, generator=g) < 0.15).to(torch.uint8)
    st = torch.randn(B, 8, generator=g).to(DEV)
    camf = cam.permute(0, 3, 1, 2).float().div(255).contiguous().to(DEV)
    lidf = (lid.clamp(max=HM).double() / HM).float().to(DEV)
    feats = lambda c, l: {"camera_feature": c, "lidar_feature": l, "status_feature": st}  # noqa: E731
    return {"f32": feats(camf, lidf), "cam_u8": feats(cam.to(DEV), lidf), "u8": feats(cam.to(DEV), lid.to(DEV)),
            "noise": torch.randn(B, Q, P, 2, generator=g).to(DEV),
            "noise_s2": torch.randn(B, 2, Q, P, 2, generator=g).to(DEV),
            "timesteps": torch.tensor([3, 17, 49]),
            "target": {"trajectory": torch.randn(B, P, 3, generator=g).to(DEV)}}


def _cut(x, n):
    """The first n scenes of a feature dict, a target dict or a tensor."""
    return {k: v[:n] for k, v in x.items()} if isinstance(x, dict) else x[:n]


def test_a_kind_leaves_nothing_behind(handle, scenes):
    """After every other kind of call, and after every refused call, the plain float forward equals the baseline
    bit for bit on every output."""
    from diffusiondrive_amd import _lib
    m, f32, nz = handle, scenes["f32"], scenes["noise"]
    plain = lambda: m.forward(f32, noise=nz, heads=True, modes=True)  # noqa: E731
    m.numerics_flags(clear=True)
    first, base = plain(), plain()  # eager, then the captured program
    assert len(base) == 6 and all(torch.equal(first[k], base[k]) for k in base)

    def refused_samples():
        with pytest.raises(_lib.DDMIError, match="max_chunk = 2"):
            m.forward_samples(f32, 3)

    def refused_descriptor():
        ins, outs = _lib.DDInputs(), _lib.DDOutputs()
        ins.camera_f32, ins.camera_u8 = f32["camera_feature"].data_ptr(), scenes["u8"]["camera_feature"].data_ptr()
        ins.lidar_f32, ins.status = f32["lidar_feature"].data_ptr(), f32["status_feature"].data_ptr()
        ins.noise, outs.trajectory = nz.data_ptr(), torch.empty(B, P, 3, device=DEV).data_ptr()
        rc = m.lib.dd_forward_in(m.handle, ctypes.byref(ins), B, 2, ctypes.byref(outs),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"camera_u8" in m.lib.dd_last_error(), (rc, m.lib.dd_last_error())

    def refused_timestep():
        with pytest.raises(ValueError, match="timesteps must lie in"):
            m.forward_train(f32, scenes["target"], timesteps=torch.tensor([3, 1000, 49]), noise=nz, safe=False)

    steps = [
        ("samples S=2", lambda: m.forward_samples(f32, 2, noise=scenes["noise_s2"], modes=True, best=True)),
        ("train with targets", lambda: m.forward_train(f32, scenes["target"], timesteps=scenes["timesteps"], noise=nz,
                                                       safe=False)),
        ("train without targets", lambda: m.forward_train(f32, None, timesteps=scenes["timesteps"], noise=nz,
                                                          safe=False)),
        ("uint8 features", lambda: m.forward(scenes["u8"], noise=nz)),
        ("refused S=3", refused_samples),
        ("refused descriptor", refused_descriptor),
        ("refused timestep", refused_timestep),
    ]
    for name, step in steps:
        step()
        again = plain()
        for k in base:
            assert torch.equal(again[k], base[k]), (name, k)
    torch.cuda.synchronize()
    assert m.numerics_flags() == 0
    info = m.graph_info()
    assert info["other_nodes"] == 0 and info["multi_stream_execs"] == 0, info


def test_one_program_per_kind(handle, scenes):
    """Each kind adds exactly one captured program; forward_samples(S=1) without best shares the plain one.

    The count is per chunk size, so the calls here take the first two scenes (one chunk under max_chunk = 2). A kind's
    first call runs eagerly and may allocate buffers, which empties the cache: every kind therefore runs once up front,
    and the counted calls allocate nothing. The cache also drops everything once it holds more than 8 programs; to stay
    clear of that limit this test clones the handle at its start (an empty cache of its own, also under
    DDMI_MAX_CHUNK=2) rather than ordering calls around what the other test left: the 8 kinds then reach 8 programs
    and never more."""
    m = _chunked(handle.clone)
    n = 2
    f32, cam_u8, u8 = (_cut(scenes[k], n) for k in ("f32", "cam_u8", "u8"))
    nz, nz2, tt, tg = (_cut(scenes[k], n) for k in ("noise", "noise_s2", "timesteps", "target"))
    kinds = [
        ("plain", lambda: m.forward(f32, noise=nz)),
        ("plain + heads", lambda: m.forward(f32, noise=nz, heads=True)),
        ("S=2", lambda: m.forward_samples(f32, 2, noise=nz2)),
        ("S=2 + best", lambda: m.forward_samples(f32, 2, noise=nz2, best=True)),
        ("train without target", lambda: m.forward_train(f32, None, timesteps=tt, noise=nz, heads=False, safe=False)),
        ("train with target", lambda: m.forward_train(f32, tg, timesteps=tt, noise=nz, heads=False, safe=False)),
        ("uint8 camera", lambda: m.forward(cam_u8, noise=nz)),
        ("uint8 camera + uint8 LiDAR", lambda: m.forward(u8, noise=nz)),
    ]
    try:
        for _, call in kinds:
            call()
        count = m.graph_info()["programs"]
        for name, call in kinds:
            call()
            call()
            count += 1
            assert m.graph_info()["programs"] == count, name
            if name == "plain":
                m.forward_samples(f32, 1, noise=nz[:, None])
                m.forward_samples(f32, 1, noise=nz[:, None])
                assert m.graph_info()["programs"] == count, "S=1 shares the plain program"
        assert count <= 8
        torch.cuda.synchronize()
    finally:
        m.close()
