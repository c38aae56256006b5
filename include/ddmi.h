/* ddmi — MI355X-native DiffusionDrive planner hot path: C ABI.
 *
 * The boundary the reference's agent API would bind for its inference forward. Every entry
 * point takes plain pointers and sizes (device pointers for tensors, hipStream_t passed as
 * void*), returns 0 on success or a negative code, and records a message for dd_last_error().
 * No torch types cross this boundary. Reference interfaces each entry replaces:
 *
 *   dd_create   <- TransfuserAgent.__init__ + initialize()        transfuser_agent.py:38-57,94-106
 *                  (V2TransfuserModel construction, strict state_dict load with the
 *                  `agent.` / `_transfuser_model.` prefixes already stripped by the caller)
 *   dd_forward  <- TransfuserAgent.forward -> V2TransfuserModel.forward (eval)
 *                                                                  transfuser_agent.py:120-125,
 *                                                                  transfuser_model_v2.py:98-162,578-641
 *   dd_forward_ex  same, with the full output dict (bev_semantic_map, agent_states, agent_labels,
 *                  all-mode poses) of transfuser_model_v2.py:144-162,165-205
 *   dd_forward_samples  S draws of the same forward's trajectory distribution per scene (S start noises through
 *                  TrajectoryHead.forward_test, transfuser_model_v2.py:578-641) over ONE pass of everything before
 *                  the head; the reference would run its whole forward once per draw
 *   dd_forward_in / dd_forward_samples_in / dd_forward_train_in  the same three forwards with the inputs in a
 *                  dd_inputs descriptor, which also takes the camera / LiDAR features as the uint8 values they are
 *                  made from (no reference counterpart: the reference widens them to float on the CPU,
 *                  transfuser_features.py:57-138)
 *   dd_destroy  <- agent teardown (no reference counterpart; frees device memory)
 *   dd_simulate_proposals  <- PDMSimulator.simulate_proposals      pdm_planner/simulation/pdm_simulator.py:32-79
 *                  (BatchLQRTracker.track_trajectory, batch_lqr.py:134-464; the profile fits of
 *                  batch_lqr_utils.py:59-249; BatchKinematicBicycleModel.propagate_state,
 *                  batch_kinematic_bicycle.py:76-185), the first stage of the PDM score (pdm_score.py:83-140)
 *   dd_simulate  <- transform_trajectory + get_trajectory_as_array (pdm_score.py:24-80) on the planner's 8 poses,
 *                  then the same simulation
 *   dd_comfort   <- ego_is_comfortable                          pdm_planner/scoring/pdm_comfort_metrics.py:313-336
 *                  (the six comfort flags of the simulated states, and optionally the six filtered signals)
 *   dd_ego_areas <- PDMScorer._calculate_ego_area, _calculate_drivable_area_compliance and
 *                  _calculate_driving_direction_compliance      pdm_planner/scoring/pdm_scorer.py:240-291,351-396
 *                  (the three map flags of every simulated state and the two scores that need nothing else)
 *   dd_collisions <- PDMScorer._calculate_no_at_fault_collision, get_collision_type and _calculate_ttc
 *                  pdm_scorer.py:293-349,414-498, pdm_scorer_utils.py:13-65
 *   dd_progress  <- PDMScorer._calculate_progress               pdm_scorer.py:398-412
 *   dd_pdm_aggregate <- PDMScorer._aggregate_scores             pdm_scorer.py:156-183
 *   dd_proposals <- PDMGenerator.generate_proposals             pdm_planner/proposal/pdm_generator.py:68-95,185-366
 *                   with BatchIDMPolicy.propagate (proposal/batch_idm_policy.py:102-168) and PDMPath.interpolate /
 *                   substring (utils/pdm_path.py:67-105)
 *   dd_pdm_select <- np.argmax(proposal_scores)                 pdm_planner/abstract_pdm_closed_planner.py
 *
 * Threading: a handle is bound to one device and is not re-entrant; concurrent calls on one
 * handle must be serialised by the caller (the reference runs one agent per worker process,
 * run_pdm_score.py:56-57). Different handles are independent.
 */
#ifndef DDMI_H_
#define DDMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_ABI_VERSION 1

#define DD_OK 0
#define DD_ERR_INVALID -1   /* bad argument / shape / missing or mis-shaped weight */
#define DD_ERR_RUNTIME -2   /* HIP runtime failure */

typedef struct dd_handle dd_handle;

#define DD_MAX_MODES 128    /* largest dd_config.num_modes */

/* Mirrors the TransfuserConfig fields the hot path reads (transfuser_config.py:10-149). Each field lists its default
 * and the values dd_create accepts; any other value returns DD_ERR_INVALID with the field's name in dd_last_error(),
 * before the weight blob is parsed and before any device call. Every accepted value is held to the float64 oracle
 * (tests/test_config_matrix_gpu.py; DESIGN.md section 5, "Configuration matrix"). */
typedef struct dd_config {
  int abi_version;     /* DD_ABI_VERSION */
  int image_arch;      /* 34 = resnet34 (default), 50 = resnet50 (nuScenes-style config C4); nothing else */
  int lidar_arch;      /* 34 only (the BEV tokens read a 512-channel LiDAR layer-4 map) */
  int cam_h, cam_w;    /* 256, 1024 only */
  int lidar_h, lidar_w;/* 256, 256 only */
  int lidar_channels;  /* 1 (use_ground_plane = False); 1..4 = lidar_seq_len x (2 if use_ground_plane else 1) */
  int num_modes;       /* 20 anchors; 1..DD_MAX_MODES (20 runs the decoder megakernel, any other count the unfused
                          chain of the same layers) */
  int num_poses;       /* 8 only (plan_anchor_encoder.0 is 8 x 64 wide) */
  int trunc_timestep;  /* 8  (transfuser_model_v2.py:594); 0..999, an index into the 1000 alphas_cumprod */
  int step_span;       /* 20 (transfuser_model_v2.py:585); 1..1000, and a truncated forward takes steps <= step_span */
} dd_config;

/* Optional outputs of dd_forward_ex (device pointers; NULL = not requested). */
typedef struct dd_outputs {
  float* trajectory;       /* B x P x 3  [x, y, heading]  (required) */
  float* poses_reg;        /* B x Q x P x 3, last step / last layer */
  float* poses_cls;        /* B x Q */
  float* bev_semantic_map; /* B x 7 x (lidar_h/2) x lidar_w, NCHW */
  float* agent_states;     /* B x 30 x 5 */
  float* agent_labels;     /* B x 30 */
} dd_outputs;

/* Outputs of dd_forward_samples (device pointers; NULL = not requested). */
#define DD_MAX_SAMPLES 32   /* largest S of dd_forward_samples */
typedef struct dd_sample_outputs {
  float* trajectory;       /* B x S x P x 3: each sample's argmax mode (required) */
  float* poses_reg;        /* B x S x Q x P x 3, last step / last layer */
  float* poses_cls;        /* B x S x Q */
  float* best_trajectory;  /* B x P x 3: the candidate with the largest cls logit over all S*Q of the scene */
  int*   best_index;       /* B: s * Q + q of that candidate (first maximum on ties, as the per-sample argmax) */
  float* bev_semantic_map; /* per scene, exactly as dd_outputs */
  float* agent_states;
  float* agent_labels;
} dd_sample_outputs;

/* Outputs of dd_forward_train (device pointers; NULL = not requested). */
typedef struct dd_train_outputs {
  float* trajectory;       /* B x P x 3: the last layer's argmax mode (required) */
  float* poses_reg[2];     /* per decoder layer: B x Q x P x 3 */
  float* poses_cls[2];     /* per decoder layer: B x Q */
  float* loss;             /* 3 floats: trajectory_loss_0, trajectory_loss_1, trajectory_loss (needs targets) */
  float* bev_semantic_map; /* B x 7 x (lidar_h/2) x lidar_w, NCHW */
  float* agent_states;     /* B x 30 x 5 */
  float* agent_labels;     /* B x 30 */
} dd_train_outputs;

/* Inputs of dd_forward_in / dd_forward_samples_in / dd_forward_train_in (device pointers). Both sensor features are
 * byte-valued by construction, and either may be passed as the bytes instead of the floats - independently of the
 * other; the fused stems then widen the bytes in their patch load (exactly: the stems see the same fp32 values, so
 * the result is bit-identical to the float call's) and the feature never exists as floats in memory:
 *   camera_f32  (B, 3, cam_h, cam_w) fp32 NCHW, or
 *   camera_u8   (B, cam_h, cam_w, 3) uint8 HWC - the resized image as cv2 / NAVSIM hold it before ToTensor
 *               (transfuser_features.py:57-77); byte k stands for float(k) / 255.0f (correctly rounded: torch's
 *               uint8 -> .float().div(255), and what dd_build_camera writes);
 *   lidar_f32   (B, C, lidar_h, lidar_w) fp32, or
 *   lidar_u8    (B, C, lidar_h, lidar_w) uint8 histogram counts, planar like the float tensor; byte c stands for
 *               (float)((double)min(c, lidar_hist_max) / (double)lidar_hist_max) (transfuser_features.py:133-137;
 *               counts above lidar_hist_max are clipped, so raw or clipped counts give the same result);
 *   lidar_hist_max  1..255, read only with lidar_u8 (the reference's hist_max_per_pixel, 5); may change from call
 *               to call on one handle.
 * Exactly one pointer per sensor: both or neither set, or a lidar_hist_max outside 1..255 with lidar_u8, returns
 * DD_ERR_INVALID before any device work with the field's name in dd_last_error(). No alignment is required of the
 * uint8 tensors. A uint8 call and a float call at the same shape are two captured programs of the handle; either
 * may follow the other. */
typedef struct dd_inputs {
  const float* camera_f32;
  const uint8_t* camera_u8;
  const float* lidar_f32;
  const uint8_t* lidar_u8;
  int lidar_hist_max;
  const float* status;     /* B x 8, as dd_forward_ex */
  const float* noise;      /* as the float entry point's noise (nullable where that one's is) */
} dd_inputs;

/* Fill *cfg with the reference defaults. */
void dd_default_config(dd_config* cfg);

/* Parse a DDW1 weight blob (diffusiondrive_amd/weights.py:pack_blob; reference state_dict key
 * schema without the `_transfuser_model.` prefix), fold BatchNorm, re-layout for the kernels and
 * upload to `device`. Missing or mis-shaped keys are an error (strict load). */
int dd_create(const dd_config* cfg, const void* weights_blob, size_t blob_bytes, int device, dd_handle** out);

/* One eval forward of B scenes. Inputs are device pointers in the reference layouts:
 * camera (B,3,cam_h,cam_w), lidar (B,C,lidar_h,lidar_w), status (B,8), noise (B,Q,P,2)
 * (the DDIM start noise the reference draws with torch.randn, transfuser_model_v2.py:593).
 * noise may be NULL: the handle then draws it on the device (Philox4x32-10 keyed by dd_set_seed's seed,
 * Box-Muller; scene s of the handle's stream since the last dd_set_seed takes draws [s*Q*P*2, (s+1)*Q*P*2)).
 * That draw is N(0,1) but NOT bit-equal to torch.randn's CPU stream: pass the noise explicitly to reproduce
 * a reference run. Any B >= 1 (more than 128 scenes run as equal chunks of at most 128, same results).
 * steps = number of truncated DDIM steps (2 in the reference). out_modes / out_cls may be NULL. */
int dd_forward(dd_handle* h, const float* camera, const float* lidar, const float* status, const float* noise,
               int B, int steps, float* out_traj, float* out_modes, float* out_cls, void* stream);

int dd_forward_ex(dd_handle* h, const float* camera, const float* lidar, const float* status, const float* noise,
                  int B, int steps, const dd_outputs* outs, void* stream);

/* dd_forward_ex with the inputs in a descriptor (fp32 or uint8 features, dd_inputs above). dd_forward_ex is this call
 * with camera_f32 / lidar_f32 set. */
int dd_forward_in(dd_handle* h, const dd_inputs* in, int B, int steps, const dd_outputs* outs, void* stream);

/* S trajectory samples per scene from one perception pass. The planner is a diffusion model: one start noise draws
 * one trajectory from its output distribution, and everything before the trajectory head (trunks, GPT fusion, FPN,
 * bev_proj, the tf decoder and its hoists, the optional heads: ~93 % of a forward) does not depend on the noise. This
 * entry runs that part once for the B scenes and the head (TrajectoryHead.forward_test, transfuser_model_v2.py:578-641)
 * over D = B * S decoder scenes, decoder scene d = b * S + s reading scene b's cross-BEV map, agent K / V and ego row.
 * The reference has no counterpart: it would call V2TransfuserModel.forward S times (best-of-N under an external
 * scorer, mode-diversity metrics, plan uncertainty). noise (B,S,Q,P,2): sample s of scene b is dd_forward's result for
 * scene b with noise[b][s]. S in 1..DD_MAX_SAMPLES and at most the handle's chunk limit (128, $DDMI_MAX_CHUNK), else
 * DD_ERR_INVALID before any device work; any B >= 1: scenes run in dd_forward's chunks (the backbone at the chunk's
 * full batch) and the head in passes of at most chunk-limit decoder scenes. Every gemm mode, schedule and accepted
 * num_modes; S = 1 is dd_forward_ex launch for launch. noise may be NULL: sample s of the call's scene b then takes
 * draw block position + b * S + s of the handle's stream (a block = Q*P*2 normals; dd_forward consumes one block per
 * scene, this call B * S), see dd_set_seed_at. best_trajectory / best_index: one more small launch picks each
 * scene's best candidate over its S*Q (only when one of the two is requested). */
int dd_forward_samples(dd_handle* h, const float* camera, const float* lidar, const float* status,
                       const float* noise /* B x S x Q x P x 2, or NULL */, int B, int S, int steps,
                       const dd_sample_outputs* outs, void* stream);

/* dd_forward_samples with the inputs in a descriptor (in->noise: B x S x Q x P x 2, or NULL). */
int dd_forward_samples_in(dd_handle* h, const dd_inputs* in, int B, int S, int steps, const dd_sample_outputs* outs,
                          void* stream);

/* The training-mode trajectory head over the eval-mode network, as a loss evaluator: replaces
 * V2TransfuserModel.forward(features, targets) with TrajectoryHead.forward_train (transfuser_model_v2.py:520-576) and
 * LossComputer (modules/multimodal_loss.py:119-168). forward_train's two random draws are inputs: timesteps (B
 * int32 in [0, 1000); the reference draws torch.randint(0, 50)) and noise (B,Q,P,2, torch.randn). The head noises the
 * normalised plan anchors per scene (diffusers add_noise), clamps, runs ONE pass of both decoder layers with each
 * scene's own time embedding, and returns every layer's poses; with target_traj (B,P,3) it also returns the
 * layers' losses cls_weight * focal + reg_weight * L1 (the reference's trajectory_cls_weight 10 / reg_weight 8) and
 * their sum. Every submodule is in eval mode (dropout off, BatchNorm running statistics). Any B >= 1 (chunks of at
 * most 128; the loss is reduced over the whole batch). */
int dd_forward_train(dd_handle* h, const float* camera, const float* lidar, const float* status, const float* noise,
                     const int* timesteps, const float* target_traj, int B, float cls_weight, float reg_weight,
                     const dd_train_outputs* outs, void* stream);
/* dd_forward_train with the inputs in a descriptor (in->noise required). */
int dd_forward_train_in(dd_handle* h, const dd_inputs* in, const int* timesteps, const float* target_traj, int B,
                        float cls_weight, float reg_weight, const dd_train_outputs* outs, void* stream);
/* The BEV-semantic term of the training loss, transfuser_loss.py:28-29 (F.cross_entropy(bev_semantic_map,
 * target.long()), mean over every pixel): logits (B,C,H,W) NCHW and target (B,H,W) uint8 class ids in device memory,
 * work = dd_bev_semantic_loss_work(B, H, W) floats of device scratch, loss = one device float. Deterministic (fixed
 * reduction order). */
int dd_bev_semantic_loss(const float* logits, const unsigned char* target, int B, int C, int H, int W, float* work,
                         float* loss, void* stream);
size_t dd_bev_semantic_loss_work(int B, int H, int W);

int dd_destroy(dd_handle* h);

/* Seed of the device noise draw (noise == NULL in dd_forward) and restart of its stream at scene 0. Default
 * seed 0. No reference counterpart (the reference draws on the CPU, transfuser_model_v2.py:593). */
int dd_set_seed(dd_handle* h, unsigned long long seed);
/* The same, with the stream positioned at global scene index first_scene: rank r of a scene-sharded job that
 * passes first_scene = r * (scenes per rank) draws exactly the noise of those scenes in an unsharded run.
 * first_scene is a DRAW-BLOCK index (a block = the Q*P*2 normals of one decoder scene): dd_forward consumes one
 * block per scene, so for it blocks are scenes; dd_forward_samples consumes S per scene, so a sharded samples run
 * passes first_scene * S. */
int dd_set_seed_at(dd_handle* h, unsigned long long seed, unsigned long long first_scene);

/* Last error message of the calling thread ("" if none). */
const char* dd_last_error(void);

/* ---- instrumentation (bench / tests) ---------------------------------------------------- */
/* Enable per-kernel HIP-event timing (disables graph replay while on). */
int dd_set_profiling(dd_handle* h, int enable);
int dd_reset_stats(dd_handle* h);
/* Accumulated stats of one kernel class ("conv_gemm", "layernorm", ...): total device ms,
 * launches and algorithmic FLOPs (conv_gemm) since the last reset. Synchronises pending events. */
int dd_kernel_stats(dd_handle* h, const char* kernel, double* total_ms, long long* launches, double* flops);
/* Algorithmic HBM bytes of the same launches (conv / GEMM classes: input map, output, residual and weight
 * image each counted once; "stem_pool": the input at its element size - 4 B per fp32 element, 1 B per uint8
 * element - the pooled map and the weight image; 0 for the other classes). */
int dd_kernel_bytes(dd_handle* h, const char* kernel, double* bytes);
/* Enable / disable hipGraph capture + replay of the forward (default on). */
int dd_set_graph(dd_handle* h, int enable);
/* Streams of the captured forward: 2 (default; $DDMI_STREAMS=0 at dd_create gives 1) = the LiDAR trunk, the tf
 * decoder and the optional heads on the handle's second stream beside the rest. The forward is captured as a program
 * of SINGLE-stream graph segments (one per run of launches between fork / join points) replayed on the two streams
 * with event records / waits between the segment launches: no graph exec has internal branch streams (the HIP runtime
 * of ROCm 7.2 faults launching a multi-stream graph whose branch streams share the launch stream's hardware queue:
 * DESIGN.md section 4, Handle lifetime). 1 = everything in order on one stream, and a forward called on a non-default
 * stream runs on that stream itself (no hand-off through the handle's own stream): the batches-in-flight mode, N such
 * handles driven from N caller streams keep N forwards in flight on one device, one hardware queue each
 * (diffusiondrive_amd/model.py InFlightPlanner); such a handle runs the decoder's value_proj without its K split (less
 * work on a shared device; $DDMI_VPROJ_SPLITS overrides). No reference counterpart (the reference runs one eager
 * forward at a time). */
int dd_set_streams(dd_handle* h, int n);
/* The handle's current stream count (1 or 2, as dd_set_streams sets it): lets a caller that switches a handle to
 * single-stream for batches in flight restore what it found (diffusiondrive_amd/runner.py). */
int dd_get_streams(dd_handle* h, int* n);
/* The captured forwards the handle holds: programs (one per shape / mode), their single-stream graph segments in all,
 * and segments whose graph has parallel branches (more than one root node: a multi-stream exec; 0 by construction). */
int dd_graph_info(dd_handle* h, int* programs, int* segments, int* multi_stream_execs);
/* Node types of those captured segments: kernel nodes, and every other node (memset / memcpy / event nodes). The
 * forward captures kernel nodes only - input staging copies run on the stream ahead of the replay, outside any graph
 * - so other_nodes is 0 (tfdec_mk4: a memset node zeroing a megakernel's counters was not seen by the
 * kernel's memory-side atomics in graph replays). */
int dd_graph_nodes(dd_handle* h, int* kernel_nodes, int* other_nodes);
/* GEMM arithmetic of every conv / linear of the path:
 *   DD_GEMM_FP32   fp32-input MFMA (v_mfma_f32_32x32x2_f32), an exact fp32 fma chain;
 *   DD_GEMM_F16X3  3-product fp16 split on f16 MFMA (conv_x3.hip): each fp32 operand becomes
 *                  hi + lo fp16, products ah*bh + ah*bl + al*bh accumulate in fp32 - fp32-class
 *                  accuracy (<= ~3*2^-22 relative per product) at 5.3x the fp32 MFMA rate.
 *   DD_GEMM_BF16   one bf16 product per MAC (operands rounded to bf16, fp32 accumulation) in the
 *                  backbone (trunks + GPT fusion), f16x3 after it (FPN, BEV tokens, decoders, heads):
 *                  the REDUCED-precision mode of the bf16 configs (BASELINE configs C2-bf16 / C4),
 *                  held to no worse than the reference's own bf16 autocast (0.06-0.08 m).
 * Default DD_GEMM_FP32, or $DDMI_GEMM=fp32|f16x3|bf16 at dd_create. Attention scores: fp32 MFMA in DD_GEMM_FP32;
 * in DD_GEMM_F16X3 the GPT attention takes f16x3's three products and the tf-decoder megakernel a three-way fp16
 * split with six products (down to 2^-22); DD_GEMM_BF16 keeps the six-product scores in the GPT attention too
 * (DESIGN.md section 5). */
#define DD_GEMM_FP32 0
#define DD_GEMM_F16X3 1
#define DD_GEMM_BF16 2
int dd_set_gemm_mode(dd_handle* h, int mode);
int dd_get_gemm_mode(dd_handle* h, int* mode);
/* Denoising schedule of the trajectory head:
 *   DD_SCHED_TRUNCATED  the reference (transfuser_model_v2.py:578-641): anchors noised to t = 8,
 *                       steps over round(arange(steps) * 20 / steps)[::-1], DDIM prev = t - 1;
 *   DD_SCHED_VANILLA    ablation C5 (no reference counterpart): x_T = noise, diffusers "leading"
 *                       set_timesteps(steps) over 1000 train steps, prev = t - 1000 / steps. */
#define DD_SCHED_TRUNCATED 0
#define DD_SCHED_VANILLA 1
int dd_set_schedule(dd_handle* h, int schedule);
/* Numerics flags raised by kernels since the last clear (synchronises the handle's stream):
 * bit 0 (DD_NUM_F16_OVERFLOW_BIT) = an activation reached |x| >= 65504 under DD_GEMM_F16X3, so that
 * forward's result is not trustworthy (re-run it in DD_GEMM_FP32); bit 1 (DD_NUM_SYNC_TIMEOUT_BIT) = the
 * tf-decoder megakernel's inter-workgroup wait gave up (never on a healthy device; same remedy); bit 2
 * (DD_NUM_SYNC_STATE_BIT) = a megakernel's inter-workgroup counter (tf decoder groups, decoder query groups) held a
 * value no healthy launch leaves there, so the waits it guards passed or failed wrongly (same remedy).
 * clear != 0 resets them, and after bit 1 or 2 also re-zeroes the inter-workgroup counters. */
#define DD_NUM_F16_OVERFLOW_BIT 1u
#define DD_NUM_SYNC_TIMEOUT_BIT 2u
#define DD_NUM_SYNC_STATE_BIT 4u
int dd_numerics_flags(dd_handle* h, unsigned* flags, int clear);
/* Copy a named internal buffer (e.g. "p3", "keyval", "cross_bev", "reg_s0l1") of the last
 * forward into dst (device pointer), at most `count` floats; *actual = buffer length. */
int dd_tap(dd_handle* h, const char* name, float* dst, size_t count, size_t* actual, void* stream);

/* ---- candidate simulation (the first stage of NAVSIM's PDM score, on the GPU) ------------------ */
/* The PDM score (navsim/evaluate/pdm_score.py:83-140) never scores a planner's waypoints: it interpolates them to a
 * 41-state proposal at 0.1 s and runs PDMSimulator.simulate_proposals - an LQR tracker closed over a kinematic bicycle
 * model for 40 steps - and computes every sub-score from the simulated states. These entries run that simulation for N
 * candidates (dd_forward_samples draws up to 32 x 20 per scene) without a handle, in float64 throughout as the
 * reference does, deterministically (no atomics; two calls on the same input are bit-equal). Of the sub-scores, comfort
 * is in scope (dd_comfort below: it needs nothing but the states), and so are drivable-area and driving-direction
 * compliance (dd_ego_areas below: the states and the scene's map polygons); collision and TTC (dd_collisions: the
 * tracked objects as well), progress (dd_progress: the centerline) and the aggregation (dd_pdm_aggregate) follow. */
typedef struct dd_sim_params {
  double wheel_base;                /* 3.089 m (nuPlan's get_pacifica_parameters) */
  double dt;                        /* 0.1 s: the proposal's sampling interval and the tracker's discretisation; the
                                       bicycle model steps int(dt * 1e6) us read back as time_us * 1e-6
                                       (pdm_simulator.py:56,62), one ulp below 0.1 */
  int tracking_horizon;             /* 10 steps (batch_lqr.py:68); 2..40 */
  double q_lon, r_lon;              /* 10, 1 (batch_lqr.py:63-64) */
  double q_lat[3], r_lat;           /* {1, 10, 0}, 1 (batch_lqr.py:65-66) */
  double jerk_penalty;              /* 1e-4 (batch_lqr.py:69) */
  double curvature_rate_penalty;    /* 1e-2 (batch_lqr.py:70) */
  double initial_curvature_penalty; /* 1e-10 (batch_lqr_utils.py:14) */
  double stopping_gain;             /* 0.5 (batch_lqr.py:71) */
  double stopping_velocity;         /* 0.2 m/s (batch_lqr.py:72) */
  double max_steering_angle;        /* pi / 3 (batch_kinematic_bicycle.py:37) */
  double accel_time_constant;       /* 0.2 s (batch_kinematic_bicycle.py:38) */
  double steering_time_constant;    /* 0.05 s (batch_kinematic_bicycle.py:39) */
} dd_sim_params;
/* Fill *p with the reference defaults listed above. */
void dd_default_sim_params(dd_sim_params* p);
/* Device scratch of one call over N candidates, in doubles (the velocity fit's factor, each candidate's velocity and
 * curvature profiles, dd_simulate's proposals). The calls allocate nothing. */
size_t dd_simulate_work(int N);
/* The simulator proper (pdm_simulator.py:32-79). proposals: device double (N, 41, 3) [x, y, heading] at 0.1 s;
 * ego_states: device double (G, 11) in the StateIndex order of pdm_enums.py:4-17 (x, y, heading, velocity x / y,
 * acceleration x / y, steering angle, steering rate, angular velocity, angular acceleration), G = N / per_group:
 * candidate n starts from ego_states[n / per_group] (per_group = 20 x S for dd_forward_samples' poses_reg); work:
 * dd_simulate_work(N) device doubles; out_states: device double (N, 41, 11), state 0 = the start state, the heading
 * in [-pi, pi) (nuPlan's principal_value). Per candidate: the least-squares velocity / acceleration fit with the
 * jerk regulariser exactly as batch_lqr_utils.py:59-70 builds it (NOT a difference matrix: the second slice
 * assignment overwrites the first), the curvature / curvature-rate fit (a 40 x 40 SPD solve per candidate, Cholesky
 * where the reference multiplies by a pseudo-inverse), then 40 steps of tracker command (the stopping P controller
 * where both the reference and the current velocity are <= stopping_velocity, else the one-step longitudinal LQR and
 * the tracking_horizon-step lateral LQR) and bicycle update. DD_ERR_INVALID before any device work, with the argument
 * or field named in dd_last_error(): N <= 0, per_group <= 0, N % per_group != 0, a null pointer, dt, wheel_base or a
 * penalty (jerk, curvature rate, initial curvature) <= 0, tracking_horizon outside 2..40. */
int dd_simulate_proposals(const double* proposals, const double* ego_states, int N, int per_group,
                          const dd_sim_params* params, double* work, double* out_states, void* stream);
/* The same from the planner's own output: traj = device float (N, num_poses, 3) in the ego frame, exactly the
 * trajectory / poses_reg tensors the forwards write (any leading shape flattened to N), read in place. The proposal is
 * built on the device first, restating transform_trajectory + get_trajectory_as_array (pdm_score.py:24-80) on the
 * exact 0.1 s grid: knot 0 is the start state's rear-axle pose, knot k = 1..8 is ego o pose_k (x0 + cos(h0) x -
 * sin(h0) y, y0 + sin(h0) x + cos(h0) y, h0 + h); x and y are linear between knots at weights j / 5; the heading is
 * unwrapped along the knots (np.unwrap), then linear. The reference evaluates nuPlan's InterpolatedTrajectory at
 * absolute timestamps truncated to whole microseconds, which moves a sample by <= 1 us of travel; this grid is exact.
 * num_poses must be 8 (poses at 0.5 s: the only num_poses dd_create accepts), else DD_ERR_INVALID. */
int dd_simulate(const float* traj, int num_poses, const double* ego_states, int N, int per_group,
                const dd_sim_params* params, double* work, double* out_states, void* stream);

/* ---- comfort metrics of simulated states (ego_is_comfortable, pdm_comfort_metrics.py:313-336, on the GPU) ------ */
/* The bounds are the module constants of pdm_comfort_metrics.py:11-28. A bound of exactly 0 (either sign) means NO
 * bound on that side: the reference's _within_bound tests the bound's truthiness (`min_bound if min_bound else -inf`,
 * :216-217), and dd_comfort keeps that. The symmetric bounds are used as (-b, +b). */
typedef struct dd_comfort_params {
  double dt;                 /* 0.1 s between states; delta = mean(diff(arange(41) * dt)) as the reference forms it */
  double min_lon_accel;      /* -4.05 m/s^2 */
  double max_lon_accel;      /*  2.40 m/s^2 */
  double max_abs_lat_accel;  /*  4.89 m/s^2 */
  double max_abs_mag_jerk;   /*  8.37 m/s^3 */
  double max_abs_lon_jerk;   /*  4.13 m/s^3 */
  double max_abs_yaw_accel;  /*  1.93 rad/s^2 */
  double max_abs_yaw_rate;   /*  0.95 rad/s */
} dd_comfort_params;
/* Fill *p with the reference's values listed above. */
void dd_default_comfort_params(dd_comfort_params* p);
/* states: device double (N, 41, 11) in StateIndex order, exactly what dd_simulate / dd_simulate_proposals write (read
 * in place: heading = column 2, acceleration x / y = columns 5 / 6). out_flags: device uint8 (N, 6), 1 = every sample
 * of the signal satisfies lo < v < hi (false on NaN), in the reference's order; out_signals: device double (N, 6, 41)
 * or NULL, the six signals the flags are taken from, each np.round(., 8) = rint(v * 1e8) / 1e8:
 *   0 lon acceleration  savgol(ax, window 41, order 2)                                   (min_lon_accel, max_lon_accel)
 *   1 lat acceleration  savgol(ay, window 41, order 2)                                   +-max_abs_lat_accel
 *   2 jerk magnitude    savgol(round(savgol(hypot(ax, ay), window 8, order 2)), window 41, order 2, deriv 1, delta)
 *                                                                                        +-max_abs_mag_jerk
 *   3 lon jerk          the same with ax in place of the hypot                           +-max_abs_lon_jerk
 *   4 yaw acceleration  savgol(unwrap(heading), window 5, order 3, deriv 2, delta)       +-max_abs_yaw_accel
 *   5 yaw rate          savgol(unwrap(heading), window 5, order 2, deriv 1, delta)       +-max_abs_yaw_rate
 * as the reference really computes them: the yaw signals use window 5 whatever window_length says (:110-136 never
 * passes it on), the jerk signals pre-smooth with the EVEN window 8 (:98; scipy fits the quadratic half a sample off
 * the grid: output i reads samples i-3..i+4) and round before differentiating, savgol_filter runs in mode "interp"
 * (the first and last window / 2 outputs come from the polynomial fitted to the first / last window samples; with
 * window 41 every output is one fit of the whole series), and unwrap is _phase_unwrap (:139-157): heading - 2 pi
 * cumsum(rint(diff(heading) / 2 pi)), ties to even. A non-finite input sample makes every output it reaches
 * non-finite and the flags that read them 0; nothing is raised. One launch on `stream`; the call allocates nothing,
 * copies nothing and does not synchronise. DD_ERR_INVALID before any device work, with the argument or field named
 * in dd_last_error(): N <= 0, null states / params / out_flags, dt <= 0 or non-finite, a NaN bound, a lower bound >=
 * its upper bound when both are non-zero (a negative symmetric bound, or min_lon_accel >= max_lon_accel). */
int dd_comfort(const double* states, int N, const dd_comfort_params* params, uint8_t* out_flags, double* out_signals,
               void* stream);

/* ---- map compliance of simulated states (PDMScorer._calculate_ego_area, pdm_scorer.py:240-291, and the two scores
 * taken from it alone: drivable-area compliance :351-358 and driving-direction compliance :360-396, on the GPU) ---- */
/* The vehicle figures are formed in double the way nuPlan's VehicleParameters forms them from get_pacifica_parameters'
 * front length 4.049, rear length 1.127 and width 2.297: length = front + rear, half_length = length / 2, half_width =
 * width / 2, rear_axle_to_center = |length / 2 - rear|. Those three figures, like dd_sim_params.wheel_base, are quoted
 * from memory of nuPlan, which is not part of this tree: they are parameters so that a caller who holds the real
 * VehicleParameters passes its own. */
typedef struct dd_area_params {
  double half_length;          /* 2.588 m */
  double half_width;           /* 1.1485 m */
  double rear_axle_to_center;  /* 1.461 m */
  double dt;                   /* 0.1 s between states (proposal_sampling.interval_length) */
  double driving_direction_horizon;               /* 1.0 s; the window holds int(horizon / dt) + 1 samples */
  double driving_direction_compliance_threshold;  /* 2.0 m: below it the driving-direction score is 1 */
  double driving_direction_violation_threshold;   /* 6.0 m: below it 0.5, else 0 */
} dd_area_params;
/* Fill *p with the values listed above. */
void dd_default_area_params(dd_area_params* p);
/* The drivable-area maps of G scenes as flat device arrays. A ring is a run of vertices whose closing edge, last to
 * first, is implied; a repeated closing vertex (as shapely stores it) is a harmless zero-length edge. A polygon is one
 * or more rings under the even-odd rule (the exterior first, then the holes: any order gives the same answer). The
 * rings of a polygon, the polygons of a scene and the scenes follow each other in the arrays. The offset arrays are
 * read on the device and are TRUSTED, not validated: every offset array must start at 0 and never decrease, ring_off
 * must end at the vertex count, poly_ring_off at the ring count, scene_poly_off at num_polys, and every ring must
 * have at least 3 vertices, all finite. diffusiondrive_amd.simulate.pack_drivable_maps guarantees that. */
typedef struct dd_drivable_maps {
  const double* verts;            /* device double (V, 2): x, y */
  const int32_t* ring_off;        /* device int32 (R + 1): ring r = vertices ring_off[r] .. ring_off[r + 1] - 1 */
  const int32_t* poly_ring_off;   /* device int32 (P + 1): polygon p = rings poly_ring_off[p] .. poly_ring_off[p+1]-1 */
  const uint8_t* poly_kind;       /* device uint8 (P): bit 0 lane class (LANE, LANE_CONNECTOR); bit 1 drivable class
                                     (ROADBLOCK, INTERSECTION, DRIVABLE_AREA, CARPARK_AREA); bit 2 on route (the
                                     polygon's token is in route_lane_ids), read only together with bit 0 */
  const int32_t* scene_poly_off;  /* device int32 (G + 1): scene g = polygons scene_poly_off[g] .. [g + 1] - 1; a scene
                                     may have none */
  int num_polys;                  /* P, the host's copy of scene_poly_off[G]; with P = 0 the first four may be NULL */
} dd_drivable_maps;
/* Device scratch of one call over maps of P polygons, in doubles: the closed bounding box of every polygon, which the
 * call's first small launch fills. Never 0, so that the scratch pointer of an all-empty map is still a pointer. */
size_t dd_ego_areas_work(int P);
/* states: device double (N, 41, 11) in StateIndex order, exactly what dd_simulate / dd_simulate_proposals write, read
 * in place (x, y, heading = columns 0..2, the rear-axle pose). Candidate n is scored on the map of scene n / per_group,
 * as in dd_simulate; G must be N / per_group. Per state the five points of state_array_to_coords_array
 * (pdm_array_representation.py:142-181) in BBCoordsIndex order - front-left, rear-left, rear-right, front-right,
 * center; center = (x, y) + rear_axle_to_center (cos h, sin h), corner = center + (lat cos(h + pi/2) + lon cos h,
 * lat sin(h + pi/2) + lon sin h) with the cosine of the rounded sum, as translate_lon_and_lat forms it - are tested
 * against every polygon of the scene. A point is in a polygon when it lies in its interior (shapely's contains): a
 * point on an edge or a vertex is outside, a point in a hole is outside; a point with a NaN coordinate is outside
 * everything. The test is a crossing count over coordinate differences (no product of absolute coordinates), exact on
 * an edge wherever the two products are exact and otherwise right for every point further from an edge than the
 * rounding of one product of two differences.
 *   out_areas: device uint8 (N, 41, 3) in EgoAreaIndex order:
 *     0 multiple lanes  more than one lane-class polygon holds at least one corner and none holds all four
 *     1 non-drivable    fewer than four corners lie in the union of the drivable-class polygons (per corner: the four
 *                       may lie in four polygons; lane-class polygons do not count)
 *     2 oncoming        the CENTER (not the rear axle) is in no lane-class polygon that is on route
 *   out_scores: device double (N, 2): [drivable-area compliance: 0 if any state is non-drivable, else 1;
 *     driving-direction compliance: 1 if m < compliance_threshold, 0.5 if m < violation_threshold, else 0 (a NaN m
 *     gives 0)], m = max_t sum(p[max(0, t - h) .. t]), h = int(horizon / dt) (eleven samples by default), p[0] = 0,
 *     p[t] = |center[t] - center[t - 1]| where the oncoming flag AT t is set, else 0
 *   out_progress: device double (N) or NULL: m
 *   out_coords: device double (N, 41, 5, 2) or NULL: the five points
 * With an empty map every state is non-drivable and oncoming and never in multiple lanes. Two launches on `stream`
 * (the bounding boxes, then the scoring: one candidate per wavefront, a polygon skipped where none of its points lies
 * in the polygon's closed bounding box); the call allocates nothing, copies nothing, does not synchronise and uses no
 * atomics: two calls on the same input are bit-equal. DD_ERR_INVALID before any device work, with the argument or
 * field named in dd_last_error(): N <= 0, per_group <= 0, N % per_group != 0, G != N / per_group, null states / maps /
 * params / work / out_areas / out_scores / maps->scene_poly_off, maps->num_polys < 0 or a null map array with
 * num_polys > 0, a length or dt that is not positive and finite, a threshold that is NaN or negative,
 * compliance_threshold > violation_threshold, a NaN horizon or int(horizon / dt) (truncated towards zero, as Python's
 * int) outside 0..40. */
int dd_ego_areas(const double* states, int N, int per_group, const dd_drivable_maps* maps, int G,
                 const dd_area_params* params, double* work, uint8_t* out_areas, double* out_scores,
                 double* out_progress, double* out_coords, void* stream);

/* ---- the rest of the PDM score: no-at-fault collision and time-to-collision (PDMScorer._calculate_no_at_fault_collision
 * :293-349 with get_collision_type, pdm_scorer_utils.py:13-65, and _calculate_ttc :414-498), progress along the
 * centerline (:398-412) and the aggregation (_aggregate_scores :156-183), on the GPU ---- */
/* The weights and thresholds of PDMScorerConfig (:36-58), get_collision_type's stopped-speed default, and the two angle
 * bounds of nuPlan's is_agent_ahead / is_agent_behind (observation/idm/utils.py), which are quoted from memory of
 * nuPlan - it is not part of this tree - and are parameters for that reason:
 *   angle = arccos(dot((cos h, sin h), (track - ego) / |track - ego|)); ahead: angle < ahead_angle; behind: angle >
 *   behind_angle; a zero-length vector, or a dot product rounded past 1, gives NaN and both are false.
 * The TTC look-ahead steps are fixed at {0, 3, 6, 9} (np.arange(0, 10, 3), :426). */
typedef struct dd_score_params {
  double progress_weight;                    /* 5 */
  double ttc_weight;                         /* 5 */
  double comfortable_weight;                 /* 2 */
  double driving_direction_weight;           /* 0 */
  double progress_distance_threshold;        /* 5.0 m */
  double ttc_stopped_speed_threshold;        /* 5e-3 m/s: below it a state takes no part in TTC */
  double collision_stopped_speed_threshold;  /* 5e-2 m/s: at or below it the ego is stopped (STOPPED_EGO) */
  double ahead_angle;                        /* deg2rad(30) */
  double behind_angle;                       /* deg2rad(150) */
} dd_score_params;
/* Fill *p with the values listed above. */
void dd_default_score_params(dd_score_params* p);
/* The tracked objects of G scenes as flat device arrays, track-major. A track is one object over T_obs occupancy maps;
 * it need not exist at every time (valid), and a NaN box never stands for absence. Every valid box must be finite and
 * CONVEX (nuPlan's oriented boxes are rectangles), corners in the order front-left, rear-left, rear-right, front-right
 * (either orientation). Tracks whose token contains "red_light" and tracks in collided_track_ids are skipped by both
 * metrics unconditionally and are not packed at all. The arrays are TRUSTED, not validated:
 * diffusiondrive_amd.simulate.pack_observations guarantees them. */
typedef struct dd_observations {
  const double* boxes;             /* device double (K, T_obs, 4, 2) */
  const uint8_t* valid;            /* device uint8 (K, T_obs): 1 where the track is in occupancy map t */
  const double* heading;           /* device double (K): unique_objects[token].box.center.heading (the first appearance):
                                      the reference's track state carries it, the angle rule as quoted reads only the
                                      centroid, and dd_collisions does not read it */
  const uint8_t* flags;            /* device uint8 (K): bit 0 stopped (is_track_stopped: not an Agent, or speed <= 5e-2),
                                      bit 1 agent type (VEHICLE, PEDESTRIAN, BICYCLE: an at-fault hit scores 0, else 0.5) */
  const int32_t* scene_track_off;  /* device int32 (G + 1): scene g = tracks scene_track_off[g] .. [g + 1] - 1 */
  int num_tracks;                  /* K, the host's copy of scene_track_off[G]; with K = 0 the first four may be NULL */
  int num_times;                   /* T_obs >= 50: TTC reads map t + 9 for t up to 40 */
} dd_observations;
/* The centerlines of G scenes: scene g's polyline is vertices scene_off[g] .. scene_off[g + 1] - 1, at least 2, all
 * finite (TRUSTED; simulate.pack_centerlines guarantees it). */
typedef struct dd_centerlines {
  const double* verts;        /* device double (V, 2) */
  const int32_t* scene_off;   /* device int32 (G + 1) */
  int num_verts;              /* V, the host's copy of scene_off[G]; at least 2 G */
} dd_centerlines;
/* Device scratch of dd_collisions over K tracks, in doubles (each track's bounding box over its valid times). Never 0. */
size_t dd_collisions_work(int K);
/* states (N, 41, 11) and areas (N, 41, 3) exactly as dd_simulate and dd_ego_areas write them; candidate n meets the
 * tracks of scene n / per_group. intersections: the polygons of layer INTERSECTION only (pack_drivable_maps(...,
 * layers=("INTERSECTION",)); poly_kind is not read; a scene may have none). The ego quad is the four corners of
 * dd_ego_areas; the TTC quads are those corners + (cos h, sin h) * hypot(vx, vy) * (double(k) * dt), k = 0, 3, 6, 9,
 * tested against map t + k. Two quads intersect when they share a point (closed: touching counts), by a separating-
 * axis test over differences against an ego corner; a quad with a non-finite corner intersects nothing (this
 * project's rule: shapely raises or answers per GEOS build). The centroid is the area centroid (the corner mean for a
 * zero-area box). Per (candidate, track) only the first hit decides:
 *   collision: the first t with an intersection. speed <= collision_stopped_speed_threshold: not at fault; else a
 *     stopped track: at fault; else the track's centroid at t (with `heading`) behind the rear-axle pose: not at fault;
 *     else the segment front-left - front-right intersects the box: at fault; else (lateral) at fault iff areas[n, t]
 *     has multiple-lanes or non-drivable set. At fault: no_collision = min(., agent ? 0 : 0.5), time index min(., t).
 *   TTC: the first (t, k) in lexicographic order with an intersection and NOT speed[t] < ttc_stopped_speed_threshold.
 *     Infraction (ttc = 0, time index min(., t)) iff the centroid at t + k is ahead, or it is not behind and either
 *     flag is set at t or the rear-axle point (x, y) is strictly inside an INTERSECTION polygon (the containment rule
 *     of dd_ego_areas).
 * Outputs, device double (N) each: no_collision in {1, 0.5, 0}, collision_time_idx (inf if none), ttc in {1, 0},
 * ttc_time_idx (inf if none). Two launches on `stream` (the tracks' bounding boxes, then one candidate per
 * wavefront); no allocation, copy, synchronisation or atomics: two calls are bit-equal. DD_ERR_INVALID before any
 * device work, naming the argument or field in dd_last_error(): N <= 0, per_group <= 0, N % per_group != 0, G != N /
 * per_group, a null states / areas / obs / intersections / area_params / score_params / work / output, null
 * scene_track_off or scene_poly_off, num_tracks < 0 or a null observation array with num_tracks > 0, num_times < 50,
 * num_polys < 0 or a null polygon array with num_polys > 0, a vehicle length or dt that is not positive and finite, a
 * dd_score_params field that is non-finite or negative, a zero weight sum, ahead_angle > behind_angle. */
int dd_collisions(const double* states, const uint8_t* areas, int N, int per_group, const dd_observations* obs,
                  const dd_drivable_maps* intersections, int G, const dd_area_params* area_params,
                  const dd_score_params* score_params, double* work, double* out_no_collision,
                  double* out_collision_time_idx, double* out_ttc, double* out_ttc_time_idx, void* stream);
/* raw progress (N): max(project(center[40]) - project(center[0]), 0) along scene n / per_group's centerline, the center
 * as in dd_ego_areas. project is shapely's LineString.project as GEOS is remembered to do it (it cannot be run here):
 * the nearest segment, the FIRST on a tie, the parameter clamped to [0, 1], the lengths of the segments before it
 * summed in order plus the partial length; differences against the segment's start. A NaN center gives NaN. One
 * launch, one thread per candidate. DD_ERR_INVALID: the counts as above, null states / lines / params / out, null
 * lines->verts / scene_off, num_verts < 2 G, a non-positive or non-finite rear_axle_to_center. */
int dd_progress(const double* states, int N, int per_group, const dd_centerlines* lines, int G,
                const dd_area_params* area_params, double* out_raw_progress, void* stream);
/* _aggregate_scores. Inputs device double (N) but comfort, device uint8 (N, 6) as dd_comfort writes it. multi =
 * no_collision * drivable_area; p = raw_progress * multi; pmax = the NaN-keeping max (np.max) of p over the per_group
 * candidates of the scene (score_proposals' rule), or with progress_reference (device double (G), else NULL) pmax_n =
 * np.max([progress_reference[n / per_group], p_n]) (pdm_score.py:99-130 scores the pair [PDM-closed, prediction]: the
 * reference value is the PDM-closed trajectory's raw * multi). progress = p / pmax if pmax >
 * progress_distance_threshold, else 1 where multi != 0 and 0 where multi == 0 (a NaN pmax takes this branch). score =
 * multi * ((((w_p progress + w_t ttc) + w_c all(comfort)) + w_d driving_direction) / (((w_p + w_t) + w_c) + w_d)).
 * One launch, one workgroup per scene, no atomics. DD_ERR_INVALID: the counts, a null input / params / output, a
 * dd_score_params field that is non-finite or negative, a zero weight sum. */
int dd_pdm_aggregate(const double* no_collision, const double* drivable_area, const double* driving_direction,
                     const double* raw_progress, const double* ttc, const uint8_t* comfort, int N, int per_group,
                     const dd_score_params* score_params, const double* progress_reference, double* out_score,
                     double* out_progress, void* stream);

/* ---- PDM-Closed's proposal generation (PDMGenerator.generate_proposals, pdm_generator.py:68-95,185-366, with
 * BatchIDMPolicy.propagate, batch_idm_policy.py:102-168, and PDMPath.interpolate / substring, pdm_path.py:67-105) on
 * the GPU: the stage in front of dd_simulate_proposals ---- */
/* The lateral paths of G scenes, the same number per scene, as flat device arrays; path q = scene q / paths_per_scene,
 * lateral index q % paths_per_scene. TRUSTED, not validated (diffusiondrive_amd.simulate.pack_paths guarantees it):
 * path_off starts at 0, never decreases and ends at num_verts; every path has at least 2 vertices, all finite, a
 * progress that starts at 0, never decreases and ends above 1e-5. */
typedef struct dd_paths {
  const double* verts;        /* device double (V, 3): x, y, heading UNWRAPPED along the path (np.unwrap) */
  const double* progress;     /* device double (V): calculate_progress of each path (its cumulative length from 0) */
  const int32_t* path_off;    /* device int32 (G * paths_per_scene + 1) */
  int paths_per_scene;        /* P >= 1 */
  int num_verts;              /* V, the host's copy of path_off[G P] */
} dd_paths;
/* What the generator reads of the observation: the tracks of dd_observations (the tokens in collided_track_ids
 * dropped, the red-light tokens NOT among them) with a speed per track, and the scenes' stop polygons - the red-light
 * lane connectors, static over time, simple rings of at least 3 vertices whose closing edge is implied - in
 * dd_drivable_maps' layout without the polygon level. Object index within a scene: the tracks in order, then the
 * rings. TRUSTED (simulate.pack_lead_objects guarantees it). */
typedef struct dd_lead_objects {
  const double* boxes;             /* device double (K, T_obs, 4, 2) */
  const uint8_t* valid;            /* device uint8 (K, T_obs) */
  const double* heading;           /* device double (K): unique_objects[token].center.heading */
  const double* speed;             /* device double (K): velocity.magnitude(); 0 for an object that is no nuPlan Agent */
  const int32_t* scene_track_off;  /* device int32 (G + 1) */
  int num_tracks;                  /* K; with K = 0 the first four may be NULL */
  int num_times;                   /* T_obs >= 41: the update at time index 40 reads occupancy map 40 */
  const double* stop_verts;        /* device double (Vs, 2) */
  const int32_t* ring_off;         /* device int32 (R + 1): ring r = vertices ring_off[r] .. ring_off[r + 1] - 1 */
  const int32_t* scene_ring_off;   /* device int32 (G + 1): scene g = rings scene_ring_off[g] .. [g + 1] - 1 */
  int num_rings;                   /* R; with R = 0 stop_verts and ring_off may be NULL */
} dd_lead_objects;
/* BatchIDMPolicy's parameters as metric_cache_processor.py:44-59 sets them (one value for all policies: the policies
 * differ by their target velocity alone), the exponent propagate hard-codes, the generator's update rate and the
 * number of poses of the TRAJECTORY sampling the corridor's length is taken from (50, not the 40 of the proposals).
 * The vehicle's width and length are dd_area_params' half_width and half_length. */
typedef struct dd_idm_params {
  double min_gap_to_lead_agent;   /* 1.0 m */
  double headway_time;            /* 1.5 s */
  double accel_max;               /* 1.5 m/s^2 */
  double decel_max;               /* 3.0 m/s^2 (positive) */
  double dt;                      /* 0.1 s */
  int acceleration_exponent;      /* 10 */
  int leading_agent_update_rate;  /* 2: the leader is searched at time indices that are multiples of it */
  int corridor_poses;             /* 50 */
} dd_idm_params;
void dd_default_idm_params(dd_idm_params* p);
/* Device scratch of dd_proposals in doubles for G scenes of P paths, K tracks and R rings in all. Never 0. */
size_t dd_proposals_work(int G, int P, int K, int R);
/* ego_states: device double (G, 11) in StateIndex order (rear-axle x, y = columns 0, 1 and velocity x = column 3 are
 * read). targets: device double (G, L): the target velocity of policy l in scene g (speed_limit_fraction * speed limit,
 * or the fallback, as BatchIDMPolicy.update forms it), TRUSTED on the device; targets_host: NULL, or a host copy of
 * the same G L values, which is then checked (a device array cannot be without a copy). L <= 64.
 *   out_proposals: device double (G P L, 41, 3), x, y, heading: lateral-major in PDMProposalManager's order, proposal
 *     n = scene n / (P L), path (n / L) % P, policy n % L: what dd_simulate_proposals takes with per_group = P L
 *   out_idm: device double (N, 41, 2) or NULL: progress, velocity
 *   out_lead: device double (N, 41, 3) or NULL: the leader's progress, velocity, rear length
 *   out_lead_index: device int32 (N, 41) or NULL: the object index within the scene (tracks, then rings: K_scene +
 *     ring), -1 for free driving and for time indices 0 and below the first update
 * The rules (DESIGN.md section 18 has them at length):
 *   start: progress = project(rear axle) on the path (dd_progress's rule); state 0 = interpolate(progress); the IDM
 *     state is (progress, velocity x).
 *   interpolate(d): d clipped to [1e-5, length]; scipy's linear interp1d over the cumulative progress (searchsorted,
 *     the index clipped to [1, V - 1], slope * (d - x_lo) + y_lo); heading arctan2(sin, cos); a NaN becomes 0.
 *   corridor, once per (scene, path): the VERTICES whose progress lies in [progress, progress + |max target| *
 *     corridor_poses * dt] (both clipped to [0, length]; the interpolated ends are not added); with one or none inside,
 *     shapely's substring as remembered: the two interpolated ends and the vertices strictly between, one point when the
 *     ends coincide. Buffered by half_width with square caps as the EXACT offset region (this project's rule: GEOS,
 *     which cannot be asked here, inscribes polygons in the arcs, at most r (1 - cos(pi / 64)) inside them): a rectangle
 *     per segment of positive length, the first and last lengthened by r; a closed disc at every interior point; one
 *     point gives a disc. Intersection is closed.
 *   leader, at time indices t that are multiples of the update rate (other rows copy the row before; rows before the
 *     first update are zero, as the reference's array): among the objects valid at t that meet the corridor and whose
 *     centroid (area centroid at t) projects strictly ahead of the proposal's progress at t - 1, the nearest to the ego
 *     quad at state t - 1 (dd_ego_areas' corners; 0 where they intersect, else the least distance between the
 *     boundaries, on coordinates relative to the quad's first corner), the first in object order on a tie. Row =
 *     (progress[t - 1] + distance, speed * cos(normalize(heading - ego heading)) for a track, .). With nothing ahead:
 *     (path length, ., half_length). The reference fills one scratch row for the proposals of a path in policy order
 *     and never clears it: a value marked '.' is what an earlier proposal of the same path wrote at the same t, 0 if
 *     none did (a leader after a free-driving proposal keeps rear length half_length; a ring after a track keeps the
 *     track's velocity).
 *   IDM: s* = (min_gap + v headway) + v (v - v_lead) / (2 sqrt(accel decel)); s_a = max((x_lead - x) - l_r, min_gap);
 *     a = clip(accel ((1 - (v / target)^exponent) - (s* / s_a)^2), -decel, accel); x += dt v; v += dt a.
 * Three launches on `stream` (setup per path; corridor membership per (path, update time); one wavefront per path
 * walking its L proposals); no allocation, copy, synchronisation or atomics: two calls are bit-equal. DD_ERR_INVALID
 * before any device work, naming the argument or field in dd_last_error(): G <= 0, L outside 1..64, a null paths /
 * objects / ego_states / targets / idm_params / area_params / work / out_proposals, paths_per_scene <= 0, null path
 * arrays, num_verts < 2 G P, num_tracks or num_rings negative, a null array that a positive count needs, null
 * scene_track_off / scene_ring_off, num_times < 41, an IDM or vehicle figure that is not positive and finite, an
 * exponent, update rate or corridor_poses that is not positive, an update rate above 40, a targets_host entry that is
 * not positive and finite, work_doubles below dd_proposals_work(G, P, K, R). */
int dd_proposals(const dd_paths* paths, const dd_lead_objects* objects, const double* ego_states,
                 const double* targets, const double* targets_host, int G, int L, const dd_idm_params* idm_params,
                 const dd_area_params* area_params, double* work, size_t work_doubles, double* out_proposals,
                 double* out_idm, double* out_lead, int32_t* out_lead_index, void* stream);
/* The pick of PDM-Closed: per scene np.argmax of its per_group scores (the first maximum; a NaN counts as the
 * maximum), that candidate's states (N, 41, 11) -> out_states (G, 41, 11) and its raw_progress * (no_collision *
 * drivable_area) -> out_reference (G): the progress_reference dd_pdm_aggregate takes. One launch, one wavefront per
 * scene. DD_ERR_INVALID: N <= 0, per_group <= 0, N % per_group != 0, a null argument. */
int dd_pdm_select(const double* score, const double* raw_progress, const double* no_collision,
                  const double* drivable_area, const double* states, int N, int per_group, int32_t* out_index,
                  double* out_states, double* out_reference, void* stream);

/* ---- PDM's forecasted observation from raw detections (PDMObservation.update, pdm_observation.py:105-205, with
 * PDMObjectManager, pdm_object_manager.py) on the GPU: the stage in front of dd_proposals and dd_collisions ---- */
/* The detections of G scenes as flat device arrays, scene g = rows scene_det_off[g] .. [g + 1] - 1. TRUSTED, not
 * validated (diffusiondrive_amd.simulate.pack_detections guarantees it): scene_det_off starts at 0, never decreases
 * and ends at num_dets; every row whose type is 0..3 is finite with a positive length and width. */
#define DD_DET_VEHICLE 0
#define DD_DET_PEDESTRIAN 1
#define DD_DET_BICYCLE 2
#define DD_DET_STATIC 3     /* every tracked object type that is not in nuPlan's AGENT_TYPES */
#define DD_DET_SKIP 255     /* TrackedObjectType.EGO, or a row to pass over; so is every value of 4..254 */
typedef struct dd_detections {
  const double* boxes;             /* device double (D, 7): center x, y, heading, length, width, velocity x, y */
  const uint8_t* type;             /* device uint8 (D): DD_DET_* */
  const int32_t* scene_det_off;    /* device int32 (G + 1) */
  const uint8_t* collided_in;      /* device uint8 (D) or NULL: non-zero = the track is in collided_track_ids (the
                                      collided_out of the call before); it must not be the call's collided_out */
  int num_dets;                    /* D, the host's copy of scene_det_off[G]; with D = 0 the first two may be NULL */
} dd_detections;
typedef struct dd_observe_params {
  double map_radius;     /* 100 m (metric_cache_processor.py:46); 0 = no radius filter (`self._map_radius and ...`) */
  double dt;             /* 0.1 s (the sampling's interval_length) */
  int num_samples;       /* 50: _observation_samples */
  int sample_res;        /* 2: observation_sample_res; T_obs = num_samples + sample_res */
  int max_vehicles;      /* 50 (MAX_DYNAMIC_OBJECTS) */
  int max_pedestrians;   /* 25 */
  int max_bicycles;      /* 10 */
  int max_static;        /* 50 (MAX_STATIC_OBJECTS) */
  double stopped_speed;  /* 5e-2 m/s: at or below it an agent counts as stopped (dd_observations.flags bit 0) */
} dd_observe_params;
/* Fill *p with the values listed above. */
void dd_default_observe_params(dd_observe_params* p);
/* Device scratch of dd_observe over D detections, in doubles (per slot the box at t = 0, its displacement per second
 * and whether it is valid). Never 0. */
size_t dd_observe_work(int D);
/* ego_states: device double (G, 11) in StateIndex order (the rear-axle x, y, heading are read). The rules:
 *   ego center = rear axle + rear_axle_to_center (cos h, sin h); the ego quad is dd_ego_areas' four corners there.
 *   dropped: a type outside 0..3, a row with collided_in set, and - unless map_radius is 0 - a row with
 *     hypot(ego center - center) > map_radius. nuPlan's Point2D.distance_to is quoted from memory as that hypot;
 *     nuPlan is not part of this tree.
 *   corners of a row: center + (lat cos(h + pi/2) + lon cos h, lat sin(h + pi/2) + lon sin h), lon = +-length / 2,
 *     lat = +-width / 2, in the order front-left, rear-left, rear-right, front-right: the formula dd_ego_areas uses for
 *     nuPlan's translate_longitudinally_and_laterally (the cosine of the rounded sum, not -sin h), which
 *     OrientedBox.all_corners is remembered to call.
 *   agents (types 0..2; pdm_object_manager.py:62-79): velocity_angle = atan2(vy, vx); the agent drives forward iff
 *     |normalize(h - velocity_angle)| < pi / 2, normalize(a) = atan2(sin a, cos a); track_heading = h, or
 *     normalize(h + pi) when it does not; dxy = (cos, sin)(track_heading) * hypot(vx, vy): a reversing agent is forecast
 *     backwards along its own axis, never along its velocity. A static object has dxy = 0.
 *   selection per class (static; vehicles; pedestrians; bicycles): ascending ((cx - px)^2 + (cy - py)^2)^0.5 to the
 *     ego center, the first `cap` kept; a tie goes to the lower detection index (the reference's np.argsort is an
 *     unstable introsort: its order on a tie is not defined).
 *   slots: scene g's tracks are slots scene_det_off[g] .. [g + 1] - 1, so K = D and scene_track_off = scene_det_off,
 *     and no count returns to the host. Within the scene, in the reference's token order (static + dynamic,
 *     pdm_observation.py:186, which decides dd_proposals' tie rule and out_lead_index): the kept static objects by
 *     distance, the kept vehicles, pedestrians, bicycles, then every dropped row in detection order. A dropped row is a
 *     track that is valid at no time; dd_collisions and dd_proposals honour `valid`.
 *   boxes[k, t] = corners + (double(sample_res (t / sample_res)) dt) dxy, t = 0 .. T_obs - 1: what observation[t]
 *     returns through _global_to_local_idcs (map t / sample_res, forecast to sample_res (t / sample_res) dt).
 *   newly collided: a kept track whose box at t = 0 meets the ego quad (dd_collisions' closed separating-axis test on
 *     differences against the ego quad's first corner). It counted toward its cap - the reference appends the token
 *     after the maps are built - and is invalid at every time, because the scorer and the generator skip
 *     collided_track_ids. out_collided[d] = collided_in[d] | newly collided, in detection order.
 * Outputs, which fill a dd_observations and a dd_lead_objects that share boxes, valid and heading:
 *   out_boxes: device double (K, T_obs, 4, 2), 16-byte aligned; zero where the track is not valid
 *   out_valid: device uint8 (K, T_obs)
 *   out_heading: device double (K): the row's own heading (unique_objects[token].center.heading)
 *   out_speed: device double (K): hypot(vx, vy), 0 for a type outside 0..2
 *   out_flags: device uint8 (K): bit 0 stopped (no agent, or speed <= stopped_speed), bit 1 agent (types 0..2)
 *   out_order: device int32 (K): the detection index (0 .. D - 1) each slot holds
 *   out_collided: device uint8 (D)
 * Two launches on `stream` (one workgroup per scene ranks by counting within the class over LDS chunks of 256 rows, so
 * any D works, and writes the slots' t = 0 boxes to `work`; then one thread per corner of the output writes the
 * forecast in whole cache lines); none with D = 0. No allocation, copy, synchronisation or atomics: two calls are
 * bit-equal. DD_ERR_INVALID before any device work, naming the argument or field in dd_last_error(): G <= 0, num_dets
 * < 0, a null det / ego_states / params / area_params / scene_det_off, with num_dets > 0 a null boxes / type / work /
 * output or an out_boxes that is not 16-byte aligned, collided_in == out_collided, sample_res outside 1..num_samples,
 * num_samples + sample_res < 50, (num_samples + sample_res) * num_dets * 8 >= 2^31 (the packers' limit), a negative cap, a dt,
 * map_radius, stopped_speed or vehicle figure (half_length, half_width, rear_axle_to_center) that is negative or
 * non-finite. */
int dd_observe(const dd_detections* det, const double* ego_states, int G, const dd_observe_params* params,
               const dd_area_params* area_params, double* work, double* out_boxes, uint8_t* out_valid,
               double* out_heading, double* out_speed, uint8_t* out_flags, int32_t* out_order, uint8_t* out_collided,
               void* stream);
/* Detections from the planner's own agent head, read in place: agent_states device float (B, A, 5), the ego-frame x,
 * y, heading, length, width of transfuser_features.py:192-204; agent_labels device float (B, A) logits; ego_states
 * device double (B, 11). Writes a dd_detections of D = A B rows: out_boxes (D, 7), out_type (D), out_scene_det_off
 * (B + 1) = A b. Row (b, a), every value widened to double first: center = (x0 + (cos(h0) x - sin(h0) y), y0 +
 * (sin(h0) x + cos(h0) y)), heading = h0 + h, velocity 0, type VEHICLE where logit > threshold (0 is the callback's
 * sigmoid() > 0.5), length and width are positive and all six values are finite; any other row is all zeros with type
 * DD_DET_SKIP. The reference has no counterpart: this is the project's rule. A zero-velocity agent is flagged stopped
 * and forecast in place. One launch. DD_ERR_INVALID: B <= 0, A <= 0, A B >= 2^31, a null argument, a NaN threshold. */
int dd_detections_from_agents(const float* agent_states, const float* agent_labels, const double* ego_states, int B,
                              int A, float threshold, double* out_boxes, uint8_t* out_type,
                              int32_t* out_scene_det_off, void* stream);

/* ---- input feature builder (TransfuserFeatureBuilder.compute_features on the GPU) ---------- */
/* Camera feature (transfuser_features.py:57-77): crop + stitch + cv2 INTER_LINEAR resize +
 * ToTensor. cams: device uint8, B scenes x 3 images (cam_l0, cam_f0, cam_r0) x src_h x src_w x 3
 * (HWC, as NAVSIM loads them); out: device float (B, 3, out_h, out_w). The stitched image must
 * down-scale by one even integer factor (NAVSIM: 1080x1920 cameras -> 4096x1024 -> 1024x256). */
int dd_build_camera(const uint8_t* cams, int B, int src_h, int src_w, float* out, int out_h, int out_w,
                    void* stream);
/* LiDAR feature (transfuser_features.py:79-138): np.histogramdd splat of the points with
 * z < max_height (split at split_height; channels = 2 for use_ground_plane: [below, above], 1:
 * [above]) over resolution^2 bins of [range_lo, range_hi] m, clip at hist_max, / hist_max.
 * xyz: device float, per scene b the planar rows x, y, z of its N_b points (= NAVSIM
 * lidar_pc[:3], contiguous) starting at element 3 * offsets[b]; offsets: device int64 [B + 1]
 * (offsets[0] = 0); max_points = max_b N_b (launch sizing); out: device float (B, channels, res, res). */
int dd_build_lidar(const float* xyz, const int64_t* offsets, int B, int channels, float* out, int resolution,
                   float range_lo, float range_hi, int pixels_per_meter, float max_height, float split_height,
                   int hist_max, long long max_points, void* stream);

/* The same two features as bytes, for dd_inputs.camera_u8 / lidar_u8 (same arguments as the float forms): out =
 * device uint8 (B, out_h, out_w, 3) HWC, the resized image itself ((s + 2) >> 2 of the four taps; the float form is
 * this / 255), and device uint8 (B, channels, res, res) = min(count, hist_max) (hist_max in 1..255; the float form
 * is this / hist_max; out 4-byte aligned). */
int dd_build_camera_u8(const uint8_t* cams, int B, int src_h, int src_w, uint8_t* out, int out_h, int out_w,
                       void* stream);
int dd_build_lidar_u8(const float* xyz, const int64_t* offsets, int B, int channels, uint8_t* out, int resolution,
                      float range_lo, float range_hi, int pixels_per_meter, float max_height, float split_height,
                      int hist_max, long long max_points, void* stream);

/* ---- single-op entry points (parity tests of individual kernels) ---------------------------- */
/* Last error message of a dd_op_* call on the calling thread. */
const char* dd_op_last_error(void);
/* Kernel and tile configuration of the calling thread's last conv / GEMM launch (dd_op_* or forward), e.g.
 * "conv_x6<8,32,128,4,2>": lets tests prove which route a shape took. */
const char* dd_op_last_kernel(void);
/* The K walk of that launch: "f23" (conv_x6's Winograd F(2,3) walk along W) or "" (the direct walk). */
const char* dd_op_last_walk(void);
/* The host's f16x3 / bf16 weight split (weights.cpp:prep_split) on host pointers, no device call: w fp32
 * [rows][K] -> hi, lo (fp16 bits) and b16 (bf16 bits), each [rows][ldh] with ldh = K rounded up to 8 (padding
 * zero), sinv[rows] = 1 / s_r, *ldh_out = ldh. Any output may be null. */
int dd_op_split_weights(const float* w, int rows, int K, uint16_t* hi, uint16_t* lo, uint16_t* b16, float* sinv,
                        int* ldh_out);
/* The megakernels' weight packing (decoder_mk.hip:pack_mk_weights) on host pointers, no device call: w fp32
 * [nout][nin], nin % 16 == 0, nout % 32 == 0 -> packed[nout * nin * 2] fp16 bits in MFMA-fragment order (block
 * (nt, ks) of 64 lanes x (8 hi, 8 lo), lane = col % 32 + 32 ((k % 16) / 8)), sinv[nout]. */
int dd_op_pack_mk_weights(const float* w, int nout, int nin, uint16_t* packed, float* sinv);
/* The decoder megakernel's GEMM core (decoder_mk.hip): out[32][N] = A[32][K] W^T + bias, A and W fp32 (W
 * [N][K] packed on the host into the MFMA-fragment f16x3 image), K % 256 == 0, N % 32 == 0; synchronous. */
int dd_op_mk_linear(const float* A, int K, const float* wgt, const float* bias, float* out, int N, void* stream);
/* Fused bev_proj (transfuser_model_v2.py:123-140 concat_cross_bev + bev_proj): out[B*H*W][256] =
 * LayerNorm(ReLU(bilinear(kvp [B][Hk][Wk][256]) + p3 wgt^T + bias)) with p3 rows of 64 channels at stride
 * p3_ld floats and wgt [256][64] = bev_proj.0's p3 columns; kvp = bev_proj.0's keyval columns applied to
 * the Hk x Wk keyval tokens. Synchronises the stream. */
int dd_op_bevproj(const float* p3, int64_t p3_ld, const float* kvp, const float* wgt, const float* bias,
                  const float* ln_g, const float* ln_b, float* out, int B, int H, int W, int Hk, int Wk, void* stream);
/* NHWC conv: in (B,H,W,Cin), wgt (Cout,KH,KW,Cin), optional bias (Cout), res (B,Ho,Wo,Cout). */
int dd_op_conv2d(const float* in, int B, int H, int W, int Cin, const float* wgt, const float* bias,
                 const float* res, float* out, int Cout, int KH, int KW, int stride, int pad, int relu, void* stream);
/* Same conv on the split-precision kernel (conv_x3.hip; weights prepared on the host as dd_create
 * does; synchronous): prec 0 = f16x3, 1 = bf16. flags (device unsigned, nullable) receives
 * DD_NUM_F16_OVERFLOW_BIT. */
int dd_op_conv2d_x3(const float* in, int B, int H, int W, int Cin, const float* wgt, const float* bias,
                    const float* res, float* out, int Cout, int KH, int KW, int stride, int pad, int relu, int prec,
                    unsigned* flags, void* stream);
/* Fused stem (replaces timm conv1 / bn1 / act1 / maxpool, transfuser_backbone.py:23-33,175-192): in (B,H,W,4)
 * NHWC, wgt (64,7,7,4) OHWI with BN folded, bias (64) -> out (B,Hp,Wp,64) = maxpool3x3/2(relu(conv7x7/2(in) +
 * bias)) on the f16x3 kernel (synchronous; weights split on the host as dd_create does). */
int dd_op_stem_pool_x3(const float* in, int B, int H, int W, const float* wgt, const float* bias, float* out,
                       unsigned* flags, void* stream);
/* The same with the arithmetic chosen: prec 0 = f16x3, 1 = bf16 (one bf16 product per MAC). */
int dd_op_stem_pool(const float* in, int B, int H, int W, const float* wgt, const float* bias, float* out, int prec,
                    unsigned* flags, void* stream);
/* The same on the reference's NCHW feature tensor of C = 1..3 channels read in place (wgt still (64,7,7,4), the
 * missing channels' taps unused) - the path dd_forward takes for the camera (C = 3) and the LiDAR histogram (C = 1,
 * which runs a one-channel kernel form: 4 k16 steps instead of 14). */
int dd_op_stem_pool_nchw(const float* in, int B, int C, int H, int W, const float* wgt, const float* bias, float* out,
                         int prec, unsigned* flags, void* stream);
/* The same on uint8 features read in place (the forms dd_forward_in takes): layout 0 = in is (B, H, W, 3) HWC
 * (C = 3), 1 = planar (B, C, H, W), C = 1..3; byte k stands for the fp32 value lut[k] (256 device floats). Equals
 * dd_op_stem_pool_nchw on the widened NCHW tensor bit for bit. */
int dd_op_stem_pool_u8(const uint8_t* in, int layout, int B, int C, int H, int W, const float* lut, const float* wgt,
                       const float* bias, float* out, int prec, unsigned* flags, void* stream);
/* C (M,N) = A (M,K) . W(N,K)^T [+ bias] [+ res (M,N)] [relu] */
int dd_op_gemm(const float* A, int M, int K, const float* W, const float* bias, const float* res, float* C, int N,
               int relu, void* stream);
/* Batched C_z (M,N) = A_z (M,K) . B_z, B_z (K,N) row-major (kn = 1) or (N,K) (kn = 0). */
int dd_op_gemm_batched(const float* A, const float* Bm, float* C, int batch, int M, int N, int K, int kn,
                       void* stream);
int dd_op_layernorm(const float* x, const float* res, int res_div, const float* g, const float* b,
                    const float* film_scale, const float* film_shift, float* y, int rows, int C, void* stream);
int dd_op_softmax_rows(float* x, int rows, int L, float scale, void* stream);
int dd_op_bilinear(const float* in, int B, int Hi, int Wi, int C, float* out, int Ho, int Wo, void* stream);
/* out += bilinear(in) (NHWC): the GPT-fusion upsample-add back into the trunks (transfuser_backbone.py:241-276,
 * F.interpolate(..., mode="bilinear", align_corners=False) then `+`) */
int dd_op_bilinear_add(const float* in, int B, int Hi, int Wi, int C, float* out, int Ho, int Wo, void* stream);
int dd_op_maxpool3x3s2(const float* in, int B, int H, int W, int C, float* out, void* stream);
int dd_op_avgpool(const float* in, int B, int H, int W, int C, int oh, int ow, float* out, void* stream);
int dd_op_bev_sample_attn(const float* logits, const float* pts, const float* value, float* out, int B, int Q,
                          int P, int Hv, int Wv, int C, void* stream);
int dd_op_mha_small(const float* q, const float* k, const float* v, float* out, int B, int Lq, int Lk, int nh,
                    int hd, void* stream);
/* Fused GPT self-attention core (replaces transfuser_backbone.py:386-410, SelfAttention.forward between
 * the qkv projections and `proj`): qkv (B,T,3C) packed q | k | v, y (B,T,C) =
 * softmax(q_h k_h^T / sqrt(C/heads)) v_h per (scene, head). prec 0: fp32 MFMA, T % 64 == 0 and
 * (T/4) % 8 == 0 (T <= 512), C/heads in {16, 32, 64, 128, 256, 512}; prec 1: f16x3 MFMA (the f16x3 mode:
 * scores on two-way fp16 splits, three products), prec 2: the same with three-way score splits and six products
 * (the bf16 mode's choice); both T % 32 == 0, T <= 1024, C/heads in {16, 32, 64, 128}. */
int dd_op_gpt_attention(const float* qkv, float* y, int B, int T, int C, int heads, int prec, void* stream);
/* The same over a query window: only rows [q_first, q_first + q_count) of every scene of y are computed and written
 * (whole blocks of 32 rows for prec 1 / 2, of 64 for prec 0), against all T keys in the full launch's tile order, so
 * those rows equal the full launch's bit for bit. waves > 0: the f16x3 form's waves per workgroup (micro-benchmarks;
 * 0 = the library's choice). */
int dd_op_gpt_attention_rows(const float* qkv, float* y, int B, int T, int C, int heads, int prec, int q_first,
                             int q_count, int waves, void* stream);
/* dd_op_layernorm (no residual, no FiLM) over `groups` groups of `group_rows` rows of C floats, the groups
 * group_stride floats apart in x and in y; rows between the groups are neither read nor written. */
int dd_op_layernorm_groups(const float* x, const float* g, const float* b, float* y, int groups, int group_rows,
                           long long group_stride, int C, void* stream);

/* ---- the same kernels on strided operand views (test support: the forms the forward launches, which the dense
 * entries above cannot express) */
/* (n, h, w, c) view with element strides: element (n, h, w, c) at p + n sn + h sh + w sw + c sc. p null: no operand.
 * The conv / GEMM operands have sc = 1. Row groups (a GEMM's A, C, res): sn = group stride, sh = row stride, sw = 0. */
typedef struct dd_op_view {
  float* p;
  int64_t sn, sh, sw, sc;
} dd_op_view;
/* One conv / GEMM launch, built as the forward builds it (views, then the K slice, the fused LayerNorm, the fused
 * pooling) and dispatched as dd_op_conv2d_x3 dispatches. A GEMM over G groups of R rows is the 1 x 1 conv with N = G,
 * H = R, W = 1. */
typedef struct dd_op_conv_desc {
  dd_op_view in, out, res; /* res optional, indexed by the output pixel (sn = 0: one image for every n) */
  int N, H, W, Cin;
  int KH, KW, stride, pad, Cout;
  const float* wgt; /* device fp32 [Cout][ldb], K order (kh, kw, ci) */
  int64_t ldb;      /* floats per weight row; > KH KW Cin only for a K slice */
  int k0;           /* K slice [k0, k0 + Cin) of the rows (1 x 1 only, k0 % 8 == 0) */
  const float* bias; /* optional */
  int relu;
  int mode; /* 0 = fp32 (conv_gemm), 1 = f16x3, 2 = bf16; 1 / 2 split the weight on the host as dd_create does */
  unsigned* flags;    /* device word receiving DD_NUM_* bits (modes 1 / 2; nullable) */
  int64_t route_rows; /* > 0: the dispatcher chooses the tile form for this many rows (a row subset of that GEMM) */
  float* ln_out; /* optional fused LayerNorm of the output rows (out's row layout), with ln_g / ln_b */
  const float* ln_g;
  const float* ln_b;
  dd_op_view pool_out; /* optional fused pool_p x pool_p mean of the output (+ pool_add, sn ignored: one for all n) */
  int pool_p;
  dd_op_view pool_add;
  int fused_ln;   /* out: 1 if the launch wrote ln_out (otherwise it is untouched) */
  int fused_pool; /* out: 1 if the launch wrote pool_out (otherwise it is untouched) */
} dd_op_conv_desc;
size_t dd_op_conv_desc_size(void);
/* Synchronous. The route taken is in dd_op_last_kernel. */
int dd_op_conv_view(dd_op_conv_desc* d, void* stream);
/* dd_op_layernorm with leading dimensions: row r of x / y at r ldx / r ldy, the residual row r / res_div at ldres;
 * film_div > 0: the FiLM vectors of row group r / film_div, film_ld floats apart (0: one pair for every row). */
int dd_op_layernorm_ld(const float* x, int64_t ldx, const float* res, int64_t ldres, int res_div, const float* g,
                       const float* b, const float* film_scale, const float* film_shift, int film_div,
                       int64_t film_ld, float* y, int64_t ldy, int rows, int C, void* stream);
/* dd_op_bilinear / dd_op_bilinear_add (accumulate = 1) on strided views. */
int dd_op_bilinear_view(const dd_op_view* in, int B, int Hi, int Wi, int C, const dd_op_view* out, int Ho, int Wo,
                        int accumulate, void* stream);
/* dd_op_mha_small with the launcher's own operand form: row i of scene b of q / out at b q_bstride + i ldq
 * (b o_bstride + i ldo), key / value row j of K / V batch b / kv_div at (b / kv_div) kv_bstride + j ldkv (k and v may
 * point into one interleaved buffer); kv_div consecutive scenes share one K / V batch (B % kv_div == 0). */
int dd_op_mha_small_view(const float* q, int64_t ldq, int64_t q_bstride, const float* k, const float* v, int64_t ldkv,
                         int64_t kv_bstride, float* out, int64_t ldo, int64_t o_bstride, int B, int Lq, int Lk, int nh,
                         int hd, int kv_div, void* stream);
/* dd_op_bev_sample_attn with `samples` consecutive scenes reading one value map (value holds B / samples maps) and the
 * two point scales: grid x = pts[..., 1] inv_max_x, grid y = pts[..., 0] inv_max_y. */
int dd_op_bev_sample_attn_s(const float* logits, const float* pts, const float* value, float* out, int B, int Q, int P,
                            int Hv, int Wv, int C, int samples, float inv_max_x, float inv_max_y, void* stream);
/* The tap tables of the gathered value_proj. slots null: rows[(ip) 4 + t] = the map pixel (image b / samples) tap t
 * of point ip reads, -1 where zero padding applies. slots given: the deduplicated form - rows[b Q P 4 + j] the j-th
 * distinct tap pixel of scene b in pixel order (-1 past its count), slots[ip 4 + t] the index into rows of the tap's
 * pixel (-1: padded). Returns 1 if launched, 0 if the dedup form refuses the shape (nothing written), < 0 on error. */
int dd_op_bev_taps(const float* pts, int* rows, int* slots, int B, int Q, int P, int Hv, int Wv, float inv_max_x,
                   float inv_max_y, int samples, void* stream);
/* The sampling on gathered rows: tap t of point ip reads vrows[slots[ip 4 + t]] (slots null: vrows[ip 4 + t]). */
int dd_op_bev_sample_attn_gathered(const float* logits, const float* pts, const float* vrows, const int* slots,
                                   float* out, int B, int Q, int P, int Hv, int Wv, int C, float inv_max_x,
                                   float inv_max_y, void* stream);
/* The capacity of value_proj's union-staged kernel: *umax_rows = the union rows one staging buffer holds, *range_keys
 * = the keys its bitmap spans. A 256-row tile whose union of 3 x 3 neighbourhoods exceeds the first, or whose
 * max key - min key + 131 exceeds the second, is computed by the gathered kernel instead. Host only. */
int dd_op_vproj_limits(int* umax_rows, int* range_keys);
/* The gathered value_proj (value_proj.hip, launch_vproj) on a caller's row table: out[b cap + l][256] =
 * ReLU(conv3x3(map) + bias) at pixel rows[b cap + l], l < counts[b]; rows past a group's count are not written.
 * map: nimg images (64, 64, 256) NHWC (nimg 0 = B); wgt: device fp32 (256, 3, 3, 256), K order (kh, kw, ci), split on
 * the host as dd_create does, its image rows lengthened by ldh_pad halfs (a multiple of 8; the padding holds NaNs);
 * rows: B * cap keys image * 4096 + pixel, distinct and ascending within a group, -1 past its count; counts: B.
 * union_stage 1: the union-staged kernel with K split usplit (1, 2, 4, 8), then the gathered kernel for the tiles
 * whose key range or union (above min(capacity, umax)) did not fit; 0: the gathered kernel for every tile.
 * The entry owns the scratch, as the forward holds it: fallback flags and arrival counters [tiles][2] zeroed
 * (tiles = ceil(B cap / 256)), split partials filled with the word part_fill. It runs the union launch, copies the
 * flags to fb_seen (host, [tiles][2], nullable: which (tile, half) pairs fell back), runs the fallback launch, then -
 * rows2 / counts2 / out2 given (all or none) - the whole form again on that second table with the same scratch, and
 * copies flags and counters to fb_after / ucnt_after (host, [tiles][2], nullable: all zero after a sound launch).
 * flags (device word, nullable) receives DD_NUM_* bits. Synchronous. DD_ERR_INVALID before any device work, with the
 * argument named in dd_op_last_error(): a null operand, B or cap < 1, a bad ldh_pad or union_stage; and after the
 * tables are read back: a count outside [0, cap] or a key outside the map. launch_vproj's own refusals (B > 256,
 * usplit, nimg > B, an operand not 16-byte aligned) return DD_ERR_RUNTIME before anything is launched. */
int dd_op_vproj(const float* map, const float* wgt, const float* bias, const int* rows, const int* counts, float* out,
                int B, int cap, int nimg, int union_stage, int usplit, int umax, int ldh_pad, unsigned part_fill,
                unsigned* flags, const int* rows2, const int* counts2, float* out2, unsigned* fb_seen,
                unsigned* fb_after, unsigned* ucnt_after, void* stream);
/* dd_op_avgpool into a strided (n, oh, ow, c) view, plus add[(y ow + x) C + c] (nullable; one table for every n). */
int dd_op_avgpool_view(const float* in, int B, int H, int W, int C, int oh, int ow, const dd_op_view* out,
                       const float* add, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDMI_H_ */
