"""Shared pieces of the batch-sweep tests (test_batch_sweep_gpu.py, its CPU companion test_batch_sweep.py) and of
tools/route_census.py: the sweep's batches, the replica builder (a batch of B scenes made of a few distinct scenes
repeated), the degenerate input batch, the float64 oracle run, the reduction of a profiling log ($DDMI_LAUNCH_LOG) to
the set of routes a forward took, and the committed census of those sets (tests/golden/forward_routes.json)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROUTES_PATH = os.path.join(HERE, "golden", "forward_routes.json")
MAX_BATCH = 129  # the census covers 1 .. MAX_BATCH (129 = the first batch the default 128-scene chunking splits)

# The batches of the GPU sweep. SWEEP is the floor, chosen from the dispatchers before the census: the route classes
# no other test holds to a ground truth (2..3, 32, 33..51, 52..63, 128), odd batches ragged against the 64 / 128 /
# 256-row tiles, both sides of the decoder's 32 | 33 group boundary and of the GPT GEMMs'
# M >= 16384 switch (51 | 52), and the chunked 129 (65 + 64). The census (20 route sets over 1 .. 129) showed that
# only B = 1 takes routes these do not reach (test_batch_sweep.py proves on the CPU that the list reaches every route);
# beside it, one odd batch of five more sets the list did not visit (8..12, 25..31, 34..50, 65..82, 103..127), 20
# batches in all. Odd on purpose: the GPT scales have 320 tokens per scene (2.5 tiles of 128 rows), so only an odd
# batch leaves the 128- and 256-row GEMM tiles ragged - conv_x3<128,128>, which the GPT GEMMs take from 103 to 128,
# has a partial tile at 111 and at none of the even batches. The three sets left (16, 64, 102) consist of routes met
# at other batches; B = 16 and 64 are held to a ground truth by test_parity_gpu.py.
SWEEP = [2, 3, 5, 7, 13, 24, 32, 33, 51, 52, 63, 100, 128, 129]
SWEEP_ADDED = [1, 11, 29, 41, 75, 111]
SWEEP_ALL = sorted(SWEEP + SWEEP_ADDED)
FP32_SWEEP = [3, 33, 129]

N_DISTINCT = 5      # period of the replicas: coprime to the 2- / 4-workgroup groupings and to every tile size
SCENE_SEED = 79     # synthetic_inputs seed of the distinct scenes (used by no other test)
CHUNK_SEED = 89     # the 7 scenes of the uneven-chunk case
DEGENERATE_SEED = 83
INPUT_KEYS = ("camera_feature", "lidar_feature", "status_feature", "noise")

Q, P = 20, 8
SL = [(s, l) for s in range(2) for l in range(2)]


# --------------------------------------------------------------------------- replicas
def replica_index(B, n=N_DISTINCT):
    """Distinct scene of every scene of a batch of B: scene i is distinct scene i % n."""
    return np.arange(B) % n


def first_occurrence(idx):
    """For a slice ``idx`` of replica_index (a chunk's scenes): the position in the slice of the first scene with the
    same distinct scene, per scene."""
    idx = np.asarray(idx)
    first = {}
    for i, d in enumerate(idx.tolist()):
        first.setdefault(d, i)
    return np.array([first[d] for d in idx.tolist()], dtype=np.int64)


def build_replicas(distinct, B):
    """The batch of B scenes from the distinct scenes' inputs (every array of ``distinct`` indexed on axis 0)."""
    idx = replica_index(B, len(distinct["status_feature"]))
    return {k: np.ascontiguousarray(np.asarray(distinct[k])[idx]) for k in INPUT_KEYS}


def chunk_ranges(B, max_chunk=128):
    """The (first scene, scenes) of the chunks a forward of B scenes runs as (Model::forward)."""
    nch = (B + max_chunk - 1) // max_chunk
    chunk = (B + nch - 1) // nch
    return [(b0, min(chunk, B - b0)) for b0 in range(0, B, chunk)]


# --------------------------------------------------------------------------- degenerate inputs
DEGENERATE = ("as drawn", "LiDAR all zero", "camera all zero", "camera and LiDAR all 1.0",
              "camera, LiDAR and status all zero", "velocity (40, -12), acceleration (-9, 9)")


def degenerate_inputs():
    """B = 6 from synthetic_inputs(6, 83): one scene per entry of DEGENERATE (an empty point cloud, a black frame, a
    saturated frame and histogram, everything zero, a fast hard-braking ego)."""
    from diffusiondrive_amd.weights import synthetic_inputs
    inp = {k: np.array(v, copy=True) for k, v in synthetic_inputs(6, DEGENERATE_SEED).items()}
    cam, lid, st = inp["camera_feature"], inp["lidar_feature"], inp["status_feature"]
    lid[1] = 0.0
    cam[2] = 0.0
    cam[3] = 1.0
    lid[3] = 1.0
    cam[4] = 0.0
    lid[4] = 0.0
    st[4] = 0.0
    st[5, 4:6] = (40.0, -12.0)
    st[5, 6:8] = (-9.0, 9.0)
    return inp


# --------------------------------------------------------------------------- oracle
def oracle_run(sd, inp, dtype=np.float64, heads=True):
    """One oracle forward in ``dtype`` (state dict and inputs cast to it) with its taps; returns the reference arrays
    by the names the GPU side uses, taps in the device's NHWC layout."""
    from oracle.model import OracleModel, Taps
    sd = {k: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in sd.items()}
    taps = Taps()
    out = OracleModel(sd).forward(*(np.asarray(inp[k]).astype(dtype) for k in INPUT_KEYS), taps=taps, heads=heads)
    B = out["trajectory"].shape[0]
    ref = {k: v.numpy() for k, v in out.items()}
    ref["img_l4"] = taps["img_l4"].permute(0, 2, 3, 1).contiguous().numpy()
    ref["p3"] = taps["p3"].permute(0, 2, 3, 1).contiguous().numpy()
    ref["bev_feature"] = taps["bev_feature"].permute(0, 2, 3, 1).contiguous().numpy()
    ref["keyval"] = taps["keyval"].numpy()
    ref["cross_bev"] = taps["cross_bev"].permute(0, 2, 3, 1).reshape(B, -1, taps["cross_bev"].shape[1]).numpy()
    ref["query_out"] = taps["query_out"].numpy()
    for s, l in SL:
        for k in ("gs", "reg", "cls"):
            ref[f"{k}_s{s}l{l}"] = taps[f"{k}_s{s}l{l}"].numpy()
    return ref


OUTPUT_NAMES = ("trajectory", "poses_reg", "poses_cls", "bev_semantic_map", "agent_states", "agent_labels")
ORACLE_TAPS = ("img_l4", "p3", "bev_feature", "keyval", "cross_bev", "query_out") + tuple(f"gs_s{s}l{l}" for s, l in SL)
MODE_TAPS = tuple(f"{k}_s{s}l{l}" for s, l in SL for k in ("reg", "cls"))


def errors(got, ref):
    """Largest error per quantity of ``got`` (name -> array, scenes on axis 0) against ``ref`` (the same scenes): the
    waypoint L2 (max over scenes) and the heading of the trajectory, absolute on the mode / agent outputs, relative to
    max(1, max |ref|) on bev_semantic_map and the taps. Only the names present in ``got``."""
    e = {}
    for k, v in got.items():
        g, r = np.asarray(v, np.float64), np.asarray(ref[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k == "trajectory":
            d = (g[..., :2] - r[..., :2]).reshape(g.shape[0], -1)
            e["waypoint_l2"] = float(np.sqrt((d ** 2).sum(-1)).max())
            e["heading"] = float(np.abs(g[..., 2] - r[..., 2]).max())
        elif k in ("poses_reg", "poses_cls", "agent_states", "agent_labels") or k in MODE_TAPS:
            e[k] = float(np.abs(g - r).max())
        else:
            e[k] = float(np.abs(g - r).max() / max(1.0, np.abs(r).max()))
    return e


def bar_of(name, bars):
    """The bar of an ``errors`` entry; ``bars`` = dict(waypoint=, heading=, mode=, agent=, tap=)."""
    if name == "waypoint_l2":
        return bars["waypoint"]
    if name == "heading":
        return bars["heading"]
    if name.startswith("agent"):
        return bars["agent"]
    if name in ("poses_reg", "poses_cls") or name in MODE_TAPS:
        return bars["mode"]
    return bars["tap"]


# --------------------------------------------------------------------------- routes
def read_launch_log(path):
    """(kernel name, detail) of every line of a profiling log."""
    out = []
    with open(path) as f:
        for line in f:
            name, detail = line.rstrip("\n").split("\t")[:2]
            out.append((name, detail))
    return out


def route_string(name, detail):
    """One launch as a batch-independent string: "<kernel> N= K= k= s= HW= -> cfg / groups / form". M= scales with the
    batch and is dropped; so do the rows of a GEMM (a k = 1 conv on an H x 1 "image"), written HW=rows."""
    keep, choice = [], []
    for tok in detail.split():
        key = tok.split("=", 1)[0]
        if key in ("cfg", "groups", "form"):
            choice.append(tok if key != "cfg" else tok[4:])
        elif key in ("N", "K", "k", "s"):
            keep.append(tok)
        elif key == "HW":
            keep.append("HW=rows" if tok.endswith("x1") else tok)
    s = " ".join([name] + keep)
    return s + (" -> " + " ".join(choice) if choice else "")


def route_set(entries):
    return sorted({route_string(n, d) for n, d in entries})


def groups_of(entries, kernel):
    """The groups= values of the launches of ``kernel`` ("decoder" / "tfdec") in a log."""
    return sorted({int(tok[7:]) for n, d in entries if n == kernel for tok in d.split() if tok.startswith("groups=")})


def ranges_of(sets):
    """{B: route set} over consecutive batches -> [{"from", "to", "routes"}] of maximal runs with an identical set."""
    out = []
    for b in sorted(sets):
        if out and out[-1]["to"] == b - 1 and out[-1]["routes"] == sets[b]:
            out[-1]["to"] = b
        else:
            out.append({"from": b, "to": b, "routes": sets[b]})
    return out


def load_routes(path=ROUTES_PATH):
    with open(path) as f:
        return json.load(f)


def routes_at(ranges, B):
    for r in ranges:
        if r["from"] <= B <= r["to"]:
            return r["routes"]
    raise KeyError(B)
