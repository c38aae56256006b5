"""conv_x6's F(2,3) walk on the device, reached with DDMI_X6_WALK=2 at the smallest shapes that can break it.

Every element against float64 with the per-element bound rho_w D + T (+ the rowrange floor) of x6_walk_emul.py - rho_w
from the CPU emulation, never from the device -, on dense operands and once more with strided out / res views inside
poisoned guards; the route (dd_op_last_kernel, dd_op_last_walk) of every launch; and the fp16 range: a pair of finite
activations whose sum leaves fp16 raises DD_NUM_F16_OVERFLOW_BIT.
"""
import pytest
import torch

import f16x3_emul as E
import x6_walk_emul as WE
from guard_util import POISON, dense_strides
from test_op_views_gpu import G_in, G_out, gv, launch, twice
from test_ops_gpu import DEV, g, nans, ok, rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
ENV = {"DDMI_X6_WALK": "2", "DDMI_X3_SPLIT": "1"}
# (B, H, W, Cin, Cout), relu, res, the form
SHAPES = [
    ((1, 16, 16, 32, 128), False, False, "conv_x6<16,16,128,4,2>"),   # one chunk: the prologue is the whole K loop
    ((1, 20, 20, 96, 132), True, False, "conv_x6<16,16,128,4,2>"),    # ragged tiles, ragged Cout
    ((2, 8, 40, 128, 192), True, True, "conv_x6<8,32,128,4,2>"),      # the 8 x 32 form, residual
    ((1, 17, 19, 64, 128), False, False, "conv_x6<16,16,128,4,2>"),   # odd H and W: a pair straddles the edge
    ((1, 20, 20, 96, 36), True, False, "conv_x6<16,16,64,4,2>"),      # the BN = 64 form, ragged Cout
    ((2, 17, 33, 128, 64), False, True, "conv_x6<16,16,64,4,2>"),     # ... full Cout, odd W across three tiles
]
FAMILIES = ("uniform", "chanscale12", "rowrange")
IDS = ["x".join(map(str, s[0])) for s in SHAPES]


def _case(shape, relu, res, family):
    B, H, W, Cin, Cout = shape
    return WE.walk_case((B, H, W, Cin, Cout, 3, 1, 1, relu, res), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape,relu,res,route", SHAPES, ids=IDS)
def test_walk_bound(gpu, monkeypatch, shape, relu, res, route, family):
    B, H, W, Cin, Cout = shape
    wc = _case(shape, relu, res, family)
    c = wc.case
    assert wc.rho <= E.RHO_MAX, wc.rho
    for key, val in ENV.items():
        monkeypatch.setenv(key, val)
    out = nans(B, H, W, Cout, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, win, bin_ = g(c.x.permute(0, 2, 3, 1)), g(c.w.permute(0, 2, 3, 1)), g(c.b)
    rin = g(c.r.permute(0, 2, 3, 1)) if res else None
    ok(gpu.dd_op_conv2d_x3(xin.data_ptr(), B, H, W, Cin, win.data_ptr(), bin_.data_ptr(),
                           rin.data_ptr() if res else None, out.data_ptr(), Cout, 3, 3, 1, 1, int(relu), 0,
                           flags.data_ptr(), None), gpu)
    assert gpu.dd_op_last_kernel().decode() == route
    assert gpu.dd_op_last_walk().decode() == "f23"
    assert int(flags.item()) == 0
    got = out.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    ratio = wc.ratio(got)
    print(f"== x6 walk {shape} {family}: rho_w {wc.rho:.3e} gpu ratio {ratio:.3f}")
    assert ratio <= 1.0, (shape, family, ratio)


@pytest.mark.parametrize("shape,relu,res,route", SHAPES, ids=IDS)
def test_walk_on_strided_views_inside_guards(gpu, monkeypatch, shape, relu, res, route):
    """The same launches with out (and res) as channel windows of wider maps, every operand inside poisoned guards: the
    NaN run and the 3e38 run agree to the bit with no flag, no guard or gap word of the output changes, the body meets
    the bound, and it is bit-identical to the dense launch."""
    B, H, W, Cin, Cout = shape
    wc = _case(shape, relu, True, "uniform")   # always with a residual here
    c = wc.case
    for key, val in ENV.items():
        monkeypatch.setenv(key, val)
    wd, bd = g(c.w.permute(0, 2, 3, 1)).reshape(Cout, -1), g(c.b)
    ldo, ldr = Cout + 12, Cout + 4

    def run(poison):
        X = G_in(c.x.permute(0, 2, 3, 1), dense_strides((B, H, W, Cin)), poison)
        R = G_in(c.r.permute(0, 2, 3, 1), (H * W * ldr, W * ldr, ldr, 1), poison)
        O = G_out((B, H, W, Cout), (H * W * ldo, W * ldo, ldo, 1))
        ran = launch(gpu, 1, gv(X), wd, gv(O), N=B, H=H, W=W, Cin=Cin, Cout=Cout, k=3, s=1, p=1, res=gv(R), bias=bd,
                     relu=relu)
        ran.walk = gpu.dd_op_last_walk().decode()
        ran.bodies["out"] = O.check()
        return ran

    ran = twice(run)
    assert ran.route == route and ran.walk == "f23"
    got = ran.bodies["out"].cpu().permute(0, 3, 1, 2)
    ratio = wc.ratio(got)
    assert ratio <= 1.0, (shape, ratio)
    dense = nans(B, H, W, Cout, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    xin, rin = g(c.x.permute(0, 2, 3, 1)), g(c.r.permute(0, 2, 3, 1))
    ok(gpu.dd_op_conv2d_x3(xin.data_ptr(), B, H, W, Cin, wd.data_ptr(), bd.data_ptr(), rin.data_ptr(),
                           dense.data_ptr(), Cout, 3, 3, 1, 1, int(relu), 0, flags.data_ptr(), None), gpu)
    assert gpu.dd_op_last_walk().decode() == "f23"
    assert torch.equal(dense.view(torch.int32), ran.bodies["out"].contiguous().view(torch.int32))


def test_walk_switch_off_gives_the_direct_launch(gpu, monkeypatch):
    """DDMI_X6_WALK=0 (and the default at this size: no small shape is routed) run the direct walk."""
    (B, H, W, Cin, Cout), relu, res, _ = SHAPES[1]
    c = _case((B, H, W, Cin, Cout), relu, res, "uniform").case
    xin, win, bin_ = g(c.x.permute(0, 2, 3, 1)), g(c.w.permute(0, 2, 3, 1)), g(c.b)
    for val in ("0", None):
        monkeypatch.delenv("DDMI_X6_WALK", raising=False)
        if val is not None:
            monkeypatch.setenv("DDMI_X6_WALK", val)
        out = nans(B, H, W, Cout, device=DEV)
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        ok(gpu.dd_op_conv2d_x3(xin.data_ptr(), B, H, W, Cin, win.data_ptr(), bin_.data_ptr(), None, out.data_ptr(),
                               Cout, 3, 3, 1, 1, int(relu), 0, flags.data_ptr(), None), gpu)
        assert gpu.dd_op_last_kernel().decode() == "conv_x6<8,8,64,2,2>"
        assert gpu.dd_op_last_walk().decode() == ""
        assert int(flags.item()) == 0


def test_walk_flags_a_pair_sum_beyond_fp16(gpu, monkeypatch):
    """Two neighbouring activations of 40000 are fp16 numbers, their sum V1 = d1 + d2 = 80000 is not: the walk raises
    DD_NUM_F16_OVERFLOW_BIT (the direct walk, which never adds activations, does not). Finite inputs only."""
    x = rnd(1, 32, 16, 16, seed=15)
    x[0, 5, 7, 8] = 40000.0
    x[0, 5, 7, 9] = 40000.0
    w = rnd(128, 32, 3, 3, seed=16)
    xin, win = g(x.permute(0, 2, 3, 1)), g(w.permute(0, 2, 3, 1))
    got = {}
    for walk in ("2", "0"):
        monkeypatch.setenv("DDMI_X6_WALK", walk)
        out = nans(1, 16, 16, 128, device=DEV)
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        ok(gpu.dd_op_conv2d_x3(xin.data_ptr(), 1, 16, 16, 32, win.data_ptr(), None, None, out.data_ptr(), 128, 3, 3, 1,
                               1, 0, 0, flags.data_ptr(), None), gpu)
        got[walk] = (int(flags.item()), gpu.dd_op_last_walk().decode())
    assert got["2"] == (1, "f23"), got
    assert got["0"] == (0, ""), got
