"""CPU companion of test_decoder_edges_gpu.py: the premises of its doctored cases, shown on the CPU oracle.

- the oracle runs end to end in float64 (float64 state dict and inputs) and agrees with its fp32 self within the
  parity bars: the float64 run is the yardstick a case's bar is derived from if the fp32 bars do not hold;
- the "A" cases reach what they claim (every layer-1 tap off the map, an exact 20-way cls tie, ...);
- every "B" edit puts the activation that enters its f16x3 site beyond the fp16 range, and the seeded dict does not.
"""
import numpy as np
import pytest
import torch

from decoder_edge_util import (BATCH, CASES, F16_MAX, OVERFLOW_SITES, make_case, make_overflow_sd,
                               record_oracle_activations)
from golden_util import golden_files, load, waypoint_l2

# the bars of tests/test_parity_gpu.py (that module is GPU-marked as a whole, so the CPU suite restates nothing and
# imports them)
from test_parity_gpu import MODE_TOL, WAYPOINT_L2_TOL


def _run(sd, inp, dtype=np.float32, heads=False):
    from oracle.model import OracleModel, Taps
    sd = {k: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in sd.items()}
    taps = Taps()
    out = OracleModel(sd).forward(*(np.asarray(inp[k]).astype(dtype) for k in
                                    ("camera_feature", "lidar_feature", "status_feature", "noise")),
                                  taps=taps, heads=heads)
    return out, taps


def test_float64_oracle_agrees_with_fp32_on_a_golden_batch(seeded_sd):
    """A float64 state dict and float64 inputs run the whole oracle in float64 (no fp32 constant left in the DDIM
    schedule, the sine / timestep embeddings); on the smallest golden batch the fp32 oracle stays within the parity
    bars of it: the trajectory within WAYPOINT_L2_TOL, every per-(step, layer) reg / cls within MODE_TOL, the BEV
    aggregate within MODE_TOL of its scale."""
    from diffusiondrive_amd.weights import synthetic_inputs
    g = min((load(p) for p in golden_files()), key=lambda g_: int(g_["batch"]))
    inp = synthetic_inputs(int(g["batch"]), int(g["seed"]))
    o32, t32 = _run(seeded_sd, inp, np.float32)
    o64, t64 = _run(seeded_sd, inp, np.float64)
    assert o32["trajectory"].dtype == torch.float32
    assert o64["trajectory"].dtype == torch.float64
    for k, v in t64.items():
        assert v.dtype == torch.float64, k
    assert waypoint_l2(o32["trajectory"].numpy(), o64["trajectory"].numpy()) <= WAYPOINT_L2_TOL
    for s in range(2):
        for l in range(2):
            for k in ("reg", "cls"):
                n = f"{k}_s{s}l{l}"
                assert float((t32[n].double() - t64[n]).abs().max()) <= MODE_TOL, n
            n = f"gs_s{s}l{l}"
            assert float((t32[n].double() - t64[n]).abs().max()) <= MODE_TOL * max(1.0, float(t64[n].abs().max())), n


@pytest.fixture(scope="module")
def case_taps(seeded_sd):
    cache = {}

    def get(name):
        if name not in cache:
            sd, inp = make_case(seeded_sd, name)
            cache[name] = (sd, inp) + _run(sd, inp)
        return cache[name]
    return get


def test_cases_are_the_documented_ones():
    assert CASES == ("clamp_noise", "offmap_l1", "tied_cls", "equal_modes") and BATCH == 2


def test_clamp_noise_reaches_corners_and_mixes_taps(case_taps):
    """The clamp of the DDIM start is active in both scenes (the synthetic anchors already reach past the normalised
    range), and with its noise x 40 scene 1 clamps about half of its coordinates: points at the upper x bound
    (x = 55.7: off the 64 x 64 map, its taps zero-padded) next to points on the map within the scene, points at the
    y bounds (26 / -20: on the map), and duplicate points. Scene 0 stays on the map."""
    from diffusiondrive_amd.config import TransfuserConfig
    from oracle.model import DDIM, denorm_odo, norm_odo
    sd, inp, _, _ = case_taps("clamp_noise")
    anchor = torch.as_tensor(sd["_trajectory_head.plan_anchor"])[None]
    img = DDIM().add_noise(norm_odo(anchor), torch.as_tensor(inp["noise"]), TransfuserConfig().trunc_timestep)
    assert (img[0].abs() > 1).any() and float((img[1].abs() > 1).float().mean()) > 0.4
    pts = denorm_odo(img.clamp(-1, 1))
    x0 = pts[0, ..., 0].numpy()
    x1, y1 = pts[1, ..., 0].numpy(), pts[1, ..., 1].numpy()
    assert float(x0.max()) < 31  # scene 0: every tap row inside the map
    assert np.isclose(x1.max(), 55.7, atol=1e-4) and np.isclose(x1.min(), -1.2, atol=1e-4)
    assert np.isclose(y1.max(), 26.0, atol=1e-4) and np.isclose(y1.min(), -20.0, atol=1e-4)
    assert (x1 > 32).sum() >= 20 and (x1 < 31).sum() >= 20  # off the map and on it within the scene
    uniq = len(np.unique(pts[1].reshape(-1, 2).numpy(), axis=0))
    assert uniq < 160 - 20, uniq  # duplicate points (the corners)


def test_offmap_l1_pads_every_layer1_tap(case_taps):
    _, _, out, taps = case_taps("offmap_l1")
    for s in range(2):
        assert float(taps[f"reg_s{s}l0"][..., 0].min()) > 33.0  # tap rows y0, y0 + 1 >= 64
        assert not taps[f"gs_s{s}l1"].any()
    x = taps["reg_s1l1"][..., 0]
    assert float(x.min()) > -10 and float(x.max()) < 64
    assert torch.isfinite(out["trajectory"]).all()


def test_tied_cls_is_an_exact_tie(case_taps):
    _, _, out, taps = case_taps("tied_cls")
    cls = taps["cls_s1l1"]
    assert (cls == cls[:, :1]).all()
    assert (cls.argmax(-1) == 0).all()
    assert torch.equal(out["trajectory"], taps["reg_s1l1"][:, 0])


def test_equal_modes_feeds_identical_rows(case_taps):
    sd, inp, _, taps = case_taps("equal_modes")
    assert (sd["_trajectory_head.plan_anchor"] == sd["_trajectory_head.plan_anchor"][7]).all()
    assert (inp["noise"] == inp["noise"][:, :1]).all()
    # identical inputs per mode: the oracle's rows agree to rounding (its BLAS may order rows' sums differently)
    reg = taps["reg_s1l1"]
    assert float((reg - reg[:, :1]).abs().max()) <= 1e-4


@pytest.fixture(scope="module")
def seeded_activations(seeded_sd):
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = synthetic_inputs(1, 7)
    with record_oracle_activations({}) as rec:
        _run(seeded_sd, inp)
    return rec


@pytest.mark.parametrize("site", sorted(OVERFLOW_SITES))
def test_overflow_edit_exceeds_fp16_at_its_site(seeded_sd, seeded_activations, site):
    """The edit's activation entering the named f16x3 site is beyond 65504 on the oracle (which stays finite in
    fp32); on the seeded dict the same activation is inside the fp16 range."""
    from diffusiondrive_amd.weights import synthetic_inputs
    probe = OVERFLOW_SITES[site][3:]
    assert probe in seeded_activations, probe
    assert seeded_activations[probe] < F16_MAX, (site, seeded_activations[probe])
    with record_oracle_activations({}) as rec:
        out, _ = _run(make_overflow_sd(seeded_sd, site), synthetic_inputs(1, 7))
    assert rec[probe] > F16_MAX, (site, rec[probe])
    assert np.isfinite(rec[probe])
    print(f"{site}: |activation| entering the site {seeded_activations[probe]:.3e} -> {rec[probe]:.3e}, "
          f"trajectory finite: {bool(torch.isfinite(out['trajectory']).all())}")


def test_gathered_tap_helper_accepts_a_correct_dedup_and_rejects_wrong_ones():
    """check_gathered_taps (the dedup check of the GPU tests) against tables built here by a plain per-tap loop: a
    correct dedup passes - also a scene with no live tap - and a wrong slot, count, row order or row value fails."""
    from decoder_edge_util import check_gathered_taps
    Bn, Q, P, HB, C = 3, 20, 8, 64, 4
    cap = Q * P * 4
    rng = np.random.default_rng(5)
    pts = rng.uniform(-40, 40, (Bn, Q * P, 2)).astype(np.float32)
    pts[1, :, 0] += 80  # scene 1: every tap off the map
    pts[2, :8] = pts[2, 8:16]  # duplicate points
    dense = rng.normal(size=(Bn * HB * HB, C))
    rows = np.full(Bn * cap, -1, np.int32)
    slots = np.full(Bn * cap, -1, np.int32)
    counts = np.zeros(Bn, np.int32)
    for b in range(Bn):
        taps = []
        for u in range(Q * P):
            x, y = float(pts[b, u, 0]), float(pts[b, u, 1])
            iy, ix = ((x / 32 + 1) * HB - 1) / 2, ((y / 32 + 1) * HB - 1) / 2  # exact in float64 for float32 points
            y0, x0 = int(np.floor(iy)), int(np.floor(ix))
            for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
                taps.append((b * HB + yy) * HB + xx if 0 <= yy < HB and 0 <= xx < HB else -1)
        uniq = sorted(set(t for t in taps if t >= 0))
        counts[b] = len(uniq)
        rows[b * cap:b * cap + len(uniq)] = uniq
        where = {p_: b * cap + i for i, p_ in enumerate(uniq)}
        slots[b * cap:(b + 1) * cap] = [where.get(t, -1) for t in taps]
    vals = np.zeros((Bn * cap, C))
    vals[rows >= 0] = dense[rows[rows >= 0]]
    args = dict(B=Bn, tol=1e-12, Q=Q, P=P, HB=HB)
    padded, live, err = check_gathered_taps(pts, rows, slots, counts, vals, dense, **args)
    assert padded >= cap and live > 0 and err == 0 and counts[1] == 0

    def broken(**kw):
        a = dict(rows=rows.copy(), slots=slots.copy(), counts=counts.copy(), vals=vals.copy())
        for k, f in kw.items():
            f(a[k])
        with pytest.raises(AssertionError):
            check_gathered_taps(pts, a["rows"], a["slots"], a["counts"], a["vals"], dense, **args)

    first_live = int(np.argmax(slots >= 0))
    broken(slots=lambda s: s.__setitem__(first_live, s[first_live] + 1))
    broken(slots=lambda s: s.__setitem__(first_live, -1))
    broken(counts=lambda c: c.__setitem__(0, c[0] - 1))
    broken(counts=lambda c: c.__setitem__(1, 1))
    broken(rows=lambda r: r.__setitem__(slice(0, 2), r[1::-1].copy()))
    broken(rows=lambda r: r.__setitem__(cap + 3, 5))  # a row in the scene without a live tap
    broken(vals=lambda v: v.__setitem__((0, 0), v[0, 0] + 1e-3))
