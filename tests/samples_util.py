"""Shared pieces of the trajectory-samples tests (test_samples.py on the CPU, test_samples_gpu.py on the GPU):
dd_forward_samples runs S decoder scenes per perception scene, decoder scene d = b * S + s. The oracle is per scene, so
its truth for a samples forward is one oracle forward of the batch in which scene b is repeated once per noise, with
that noise (``oracle_batch``); the draw-block rule of the device noise is restated here (``block_window``)."""
import numpy as np

import batch_sweep_util as U

Q, P = U.Q, U.P
MAX_SAMPLES = 32          # DD_MAX_SAMPLES (include/ddmi.h)
PAIR_SEED = 131           # synthetic_inputs seed of the two scenes of the distinct-pairs case (used by no other test)
GROUP_SEED = 137          # the three scenes of the group-boundary shapes
MODES6_SEED = 139         # the two scenes of the unfused-chain case
VANILLA_SEED = 149        # the scene of the vanilla-schedule case
SHARD_SEED = 151          # the four scenes of the device-noise cases
NOISE_SEED = 157          # seed of the (B, S, Q, P, 2) start noises


def sample_noise(B, S, q=Q, seed=NOISE_SEED):
    """Seeded start noises (B, S, q, P, 2), float32."""
    return np.random.default_rng(seed).standard_normal((B, S, q, P, 2)).astype(np.float32)


def oracle_batch(scenes, noise):
    """The oracle's batch for a samples forward: scene b repeated once per noise[b, s], scene-major (row b * S + s),
    by batch_sweep_util.INPUT_KEYS. ``scenes``: camera / LiDAR / status of B scenes, ``noise``: (B, S, Q, P, 2)."""
    B, S = noise.shape[:2]
    rep = np.repeat(np.arange(B), S)
    out = {k: np.ascontiguousarray(np.asarray(scenes[k])[rep]) for k in U.INPUT_KEYS[:3]}
    out["noise"] = np.ascontiguousarray(noise.reshape((B * S,) + noise.shape[2:]))
    return out


def block_window(position, b, S, s, block=Q * P * 2):
    """(first normal, count) of the draw block that sample s of the call's scene b takes when the handle's stream
    stands at block ``position``: block position + b * S + s, a block = Q * P * 2 normals."""
    return (position + b * S + s) * block, block


def head_passes(n, S, max_chunk=128):
    """The (first scene, scenes) of the trajectory-head passes over a chunk of n scenes: consecutive equal ranges of at
    most max_chunk // S scenes (Model::forward_body)."""
    per_max = max(1, max_chunk // S)
    npass = (n + per_max - 1) // per_max
    per = (n + npass - 1) // npass
    return [(b0, min(per, n - b0)) for b0 in range(0, n, per)]


def decoder_groups(D):
    """Workgroups per decoder scene of decoder_mk at D decoder scenes (the dispatcher's documented rule)."""
    return 4 if D * 4 <= 64 else 2 if D * 2 <= 64 else 1
