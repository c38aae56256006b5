"""conv_x6's F(2,3) walk on the CPU (x6_walk_emul.py): rho_w and the emulation's share of the bound on every family,
and the whole oracle with every routable conv in the walk's arithmetic.

Measured here: the walk emulation's max (err - T)+ / D is 3.3e-8 - 6.7e-8 over the cases (0 on the chanscale families,
where T covers it; the direct emulation reads the same class), below plain fp32's 5.1e-8 - 1.1e-7, so rho_w = 2.0e-7 -
4.3e-7 <= RHO_MAX and the emulation sits at 0.13 - 0.46 of its bound; the emulated-walk oracle at B = 2 reads 0.125 /
0.244 / 0.135 / 0.175 of the tightest bar (query_out) on the seeded, rescaled, rescaled_var and rescaled_signed dicts
(direct f16x3: 0.13 / 0.26 / 0.15 / 0.18).
"""
import numpy as np
import pytest
import torch

import batch_sweep_util as U
import f16x3_cases as C
import f16x3_emul as E
import rescale_util as R
import x6_walk_emul as WE
from test_f16x3_bound import _worst


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name,shape", WE.CPU_SHAPES, ids=[c[0] for c in WE.CPU_SHAPES])
def test_walk_emulation_meets_half_its_bound(name, shape, family):
    """rho_w = 4 max(emulation, plain fp32) <= RHO_MAX, and the emulation (fp32 accumulation in k16 steps, after ReLU)
    is within half of rho_w D + T (+ the rowrange floor) on every element; the other half is for the device's
    summation order."""
    wc = WE.walk_case(shape, family)
    assert wc.rho == 4 * max(wc.rho_emul, wc.rho_fp32)
    ratio = wc.ratio(wc.emul())
    print(f"{name} {family}: rho_w {wc.rho:.3e} (walk emulation {wc.rho_emul:.2e}, fp32 {wc.rho_fp32:.2e}; direct rho "
          f"{wc.case.rho:.3e}) emulation / bound {ratio:.3f}")
    assert wc.rho <= E.RHO_MAX, (name, family, wc.rho)
    assert ratio <= 0.5, (name, family, ratio)


def test_walk_equals_the_direct_conv_in_float64():
    """The transform itself: with float64 accumulation and unsplit-exact inputs (small integers) the walk is the
    convolution, odd W and the map's edges included."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (2, 32, 5, 7), generator=gen).float()
    w = torch.randint(-4, 5, (8, 32, 3, 3), generator=gen).float() * 2.0   # even taps: U1, U2 stay integers
    ref = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
    got = WE.conv_walk_emul(x, w, acc=torch.float64)
    assert torch.equal(got.double(), ref)


@pytest.fixture(scope="module")
def inputs():
    from diffusiondrive_amd.weights import synthetic_inputs
    return synthetic_inputs(2, 7)


@pytest.mark.parametrize("variant", ["seeded"] + list(R.VARIANTS))
def test_emulated_walk_oracle_stays_inside_half_of_every_bar(seeded_sd, inputs, variant):
    """The oracle at B = 2 with every 3 x 3 / stride 1 conv of Cin >= 128 in the walk's arithmetic (48 convs, a
    superset of what the forward routes), the rest in direct f16x3, against the float64 oracle on the same dict: within
    half of every bar."""
    sd = seeded_sd if variant == "seeded" else R.VARIANTS[variant](seeded_sd)
    ref = U.oracle_run(sd, inputs)
    with WE.emulated_walk_oracle() as replaced:
        em = U.oracle_run(sd, inputs, dtype=np.float32)
    assert len(set(replaced)) == 48, len(set(replaced))
    e, name, frac = _worst(em, ref)
    print(f"{variant} emulated walk vs float64: worst {name} {e[name]:.3e} = {frac:.3f} of its bar")
    assert frac <= 0.5, (variant, name, e[name])
