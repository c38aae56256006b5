// Decoder-layer megakernel: one launch per (denoise step, decoder layer) for the whole batch, one
// 512-thread workgroup per scene (TrajectoryHead.forward_test, transfuser_model_v2.py:578-641, with
// CustomTransformerDecoderLayer :297-382 inside). The per-layer chain of the unfused path - about 20
// launches of 5-25 us (12 M = 1280 GEMMs, 5 LayerNorms, BEV sampling, agent MHA, finalize, DDIM) -
// becomes one launch whose phases are separated by workgroup barriers only: every row of the chain
// is a trajectory query of ONE scene, so no phase needs another workgroup's data.
//
// Per scene (20 queries; MFMA row tile 32, rows 20..31 zero):
//   [layer 0] points = denorm(clamp(x_t)); gen_sineembed_for_position (blocks.py:22-40) -> 512 / query;
//             plan_anchor_encoder Linear 512 -> 256, ReLU, LN, Linear 256 -> 256 (:459-462) = traj_feature
//   BEV attention (blocks.py:88-129): logits = Linear 256 -> 8 (fp32 VALU), softmax, 4-tap bilinear
//             gather of the gathered value_proj rows (slots), output_proj + residual
//   agent cross-attention: q projection, 8-head attention over the scene's 30 agent K / V (staged in
//             LDS), out_proj + residual, norm1; ego attention (hoisted: + ego row), norm2
//   FFN 256 -> 1024 -> 256 (four 256-wide hidden chunks, the second GEMM accumulating in registers),
//             norm3, FiLM (ModulationLayer, :259-294)
//   heads (:208-256): cls [Linear, ReLU, LN] x 2 -> Linear 256 -> 1; reg Linear-ReLU-Linear-ReLU ->
//             Linear 256 -> 24; reg[..., :2] += points, heading = tanh * pi (:376-380)
//   [layer 0] the BEV taps of layer 1 (its points = this layer's reg xy) deduplicated for the gathered
//             value_proj conv that runs between the two launches
//   [layer 1] DDIM step (eta 0, prediction 'sample', clip; diffusers semantics) and the taps of the next
//             step's layer 0; or, at the last step, the argmax mode selection (:637-641)
//
// Arithmetic: the 256-wide Linears are f16x3 on v_mfma_f32_32x32x16_f16 exactly as conv_x3 (weights
// pre-split with the same per-column power-of-two scale, stored in MFMA-fragment order so a wave's
// B fragment is one contiguous 2 KB read; activations split once when their producer writes them to
// LDS); the 8 / 1 / 24-wide heads, softmaxes, LayerNorms, attention, geometry and DDIM in fp32 VALU.
// Compiled with -ffp-contract=off like decoder.hip: the geometry / DDIM chains round like PyTorch.
//
// LDS (141 KB, one workgroup per CU): two fp32 [32][260] row buffers, two split [32][264] hi / lo
// A-operand buffers (together the K = 512 embedding operand, or the scene's agent K / V during the
// attention), small per-query state. Weights stream from L2 straight into the MFMA operand registers.
#include "decoder_mk.h"
#include "mk_core.h"

#include <algorithm>
#include <cmath>

namespace ddmi {

namespace {

constexpr int kQ = 20, kP = 8, kD = 256, kA = 30, kNH = 8, kHD = 32, kHV = 64, kFF = 1024;
constexpr int kQP = kQ * kP;
constexpr int OFF_T1 = 32 * FP * 4;
constexpr int OFF_SA = 2 * 32 * FP * 4;               // 66560
constexpr int SPLIT_BYTES = 32 * HP * 2;              // one hi or lo image, K = 256
constexpr int OFF_SB = OFF_SA + 2 * SPLIT_BYTES;      // 100352
constexpr int OFF_SMALL = OFF_SB + 2 * SPLIT_BYTES;   // 134144
// small per-query state (floats)
constexpr int S_W8 = 0;                 // [20][8] BEV point weights
constexpr int S_PTS = S_W8 + kQP;       // [160][2] points of this layer
constexpr int S_PN = S_PTS + 2 * kQP;   // [160][2] next points
constexpr int S_RR = S_PN + 2 * kQP;    // [20][24] reg head raw
constexpr int S_REG = S_RR + kQ * 24;   // [160][3] reg output
constexpr int S_CLS = S_REG + 3 * kQP;  // [20] cls logits
constexpr int S_SLOT = S_CLS + 32;      // [160] int4 tap slots of this (step, layer), staged at the start
constexpr int S_END = S_SLOT + 4 * kQP;
constexpr int LDS_BYTES = OFF_SMALL + S_END * 4;
static_assert(2 * 32 * HP2 * 2 <= 4 * SPLIT_BYTES, "K = 512 operand fits the two split buffers");
static_assert(kA * 2 * kD * 4 <= 4 * SPLIT_BYTES, "agent K / V fit the two split buffers");
static_assert(4096 * 4 + NT * 4 <= 32 * FP * 4, "dedup table fits a row buffer");
static_assert(kNH * kQ * 33 <= 32 * FP, "attention probabilities fit a row buffer");

__device__ inline float norm_x(float x) { return 2.f * (x + 1.2f) / 56.9f - 1.f; }
__device__ inline float norm_y(float y) { return 2.f * (y + 20.f) / 46.f - 1.f; }
__device__ inline float denorm_x(float x) { return (x + 1.f) / 2.f * 56.9f - 1.2f; }
__device__ inline float denorm_y(float y) { return (y + 1.f) / 2.f * 46.f - 20.f; }

// F.grid_sample bilinear geometry (align_corners=False) of a trajectory point (blocks.py:101-122),
// the arithmetic of decoder.hip's bev_tap_geometry
__device__ inline void tap_geom(float tx, float ty, int& x0, int& y0, float wt[4]) {
  const float gx = ty * (1.0f / 32.0f);  // grid x (width) <- trajectory y
  const float gy = tx * (1.0f / 32.0f);  // grid y (height) <- trajectory x
  const float ix = ((gx + 1.f) * (float)kHV - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)kHV - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  x0 = (int)fx;
  y0 = (int)fy;
  const int x1 = x0 + 1, y1 = y0 + 1;
  wt[0] = ((float)x1 - ix) * ((float)y1 - iy);
  wt[1] = (ix - (float)x0) * ((float)y1 - iy);
  wt[2] = ((float)x1 - ix) * (iy - (float)y0);
  wt[3] = (ix - (float)x0) * (iy - (float)y0);
}

// the scene's distinct tap pixels (pixel order) -> rows[b*cap ..], -1 past the count, the count -> counts[b]
// (the gathered value_proj compacts the scenes' rows with it); each tap's compact row -> slots
// (bev_tap_dedup_kernel's algorithm with the workgroup's threads). img = the map image the scene samples (its
// perception scene: b / samples); counts, slots and the compact row base stay per decoder scene b
__device__ void dedup_scene(const float* pts, int* table, int* scan, int b, int img, int* rows, int* slots,
                            int* counts) {
  const int tid = threadIdx.x, nt = blockDim.x;
  constexpr int HW = kHV * kHV, cap = kQP * 4;
  const int64_t base = (int64_t)b * cap;
  for (int e = tid; e < HW; e += nt) table[e] = 0;
  __syncthreads();
  for (int u = tid; u < kQP; u += nt) {
    int x0, y0;
    float wt[4];
    tap_geom(pts[2 * u], pts[2 * u + 1], x0, y0, wt);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
      if ((unsigned)yy < (unsigned)kHV && (unsigned)xx < (unsigned)kHV) table[yy * kHV + xx] = 1;
    }
  }
  __syncthreads();
  const int E = (HW + nt - 1) / nt;
  int cnt = 0;
  for (int e = tid * E; e < min(HW, tid * E + E); ++e) cnt += table[e];
  // exclusive prefix of the per-thread counts: inclusive wave scan by shuffles, then the wave totals
  const int lane = tid & 63, wv = tid >> 6, nw = (nt + 63) >> 6;
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) scan[wv] = inc;
  __syncthreads();
  int wbase = 0, total = 0;
  for (int w = 0; w < nw; ++w) {
    const int t = scan[w];
    if (w < wv) wbase += t;
    total += t;
  }
  __syncthreads();  // scan[] is free again (the caller's table + 4096 stays untouched otherwise)
  scan[tid] = wbase + inc;  // inclusive prefix, as the rest of the function expects
  int r = scan[tid] - cnt;
  for (int e = tid * E; e < min(HW, tid * E + E); ++e)
    if (table[e]) {
      table[e] = r;
      rows[base + r] = img * HW + e;
      ++r;
    }
  for (int j = total + tid; j < cap; j += nt) rows[base + j] = -1;
  if (tid == 0 && counts) counts[b] = total;
  __syncthreads();
  for (int u = tid; u < kQP; u += nt) {
    int x0, y0;
    float wt[4];
    tap_geom(pts[2 * u], pts[2 * u + 1], x0, y0, wt);
    int4 sl;
    auto slot = [&](int yy, int xx) {
      return ((unsigned)yy < (unsigned)kHV && (unsigned)xx < (unsigned)kHV) ? (int)(base + table[yy * kHV + xx]) : -1;
    };
    sl.x = slot(y0, x0);
    sl.y = slot(y0, x0 + 1);
    sl.z = slot(y0 + 1, x0);
    sl.w = slot(y0 + 1, x0 + 1);
    *reinterpret_cast<int4*>(slots + ((int64_t)b * kQP + u) * 4) = sl;
  }
}

// Hand-off of the query groups' results to the scene's last arriving group (MI355X_MICROARCH.md hand-off table, the
// "workgroup whose add came last" row): every published word is stored sc1 (write-through; the line leaves the
// writer's L2) and read back with sc1 loads, and every scene's published region starts on a 128-B line no other
// scene writes (reg_out 1920 B, the point buffers 1280 B per scene, cls through cls_x's 128-B slot), so no reader's
// L2 can hold a partial line another group rewrote within the launch.
__device__ inline void st_x(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline float ld_x(const float* p) {
  return __uint_as_float(
      __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// QG queries of one scene per workgroup (G = 20 / QG workgroups per scene, group gi takes queries gi QG ..): every
// phase is per query except the mode selection and the next taps' dedup, which the scene's last arriving group runs
template <int QG>
__global__ __launch_bounds__(NT, 1) void decoder_mk_kernel(MkArgs a) {
  constexpr int G = kQ / QG, QGP = QG * kP;
  static_assert(G * QG == kQ, "query groups");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* X1 = reinterpret_cast<float*>(lds);
  float* T1 = reinterpret_cast<float*>(lds + OFF_T1);
  char* SA = lds + OFF_SA;  // hi image; lo image at + SPLIT_BYTES
  char* SB = lds + OFF_SB;
  float* SM = reinterpret_cast<float*>(lds + OFF_SMALL);
  const float* __restrict__ dim_t = a.dim_t;
  const int b = blockIdx.x / G, gi = blockIdx.x % G, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int bp = b / a.samples;   // the perception scene (map image, agent K / V, ego row) of decoder scene b
  const int q0 = gi * QG;         // first query of the group in the scene
  const int row0 = b * kQ + q0;   // its global query row
  const int64_t pt0 = (int64_t)b * kQP + q0 * kP;  // its first (query, point) of the scene's
  const MkLayer& L = a.L;
  // diagnostic phase stamps (a separate build, DDMI_BUILD_VARIANT=stamps: -DDDMI_MK_STAMPS, and
  // MkArgs::stamps set by DDMI_MK_STAMPS=1): shader clock after each phase barrier. Compiled out of the
  // product library (the stamp stores cost registers).
#ifdef DDMI_MK_STAMPS
  __shared__ unsigned long long st_lds[40];
  if (tid < 40) st_lds[tid] = 0ull;
  auto stamp = [&](int k) {
    if (tid == 0) st_lds[k] = __builtin_amdgcn_s_memtime();
  };
#else
  auto stamp = [](int) {};
#endif
  stamp(0);
  const MkLin none{};
  Ring R;
  ring_fill(R, a.layer == 0 ? a.A.pa0 : L.outp, wave, 0);  // flies under the prologue
  int4* SLOT = reinterpret_cast<int4*>(SM + S_SLOT);
  for (int t = tid; t < QGP; t += NT) SLOT[t] = reinterpret_cast<const int4*>(a.slots)[pt0 + t];

  // ================================================================ layer 0: points, embedding, anchor encoder
  if (a.layer == 0) {
    for (int t = tid; t < QGP; t += NT) {
      const float* im = a.imgx + (pt0 + t) * 2;
      const float cx = fminf(fmaxf(im[0], -1.f), 1.f);
      const float cy = fminf(fmaxf(im[1], -1.f), 1.f);
      const float px = denorm_x(cx), py = denorm_y(cy);
      SM[S_PTS + 2 * t] = px;
      SM[S_PTS + 2 * t + 1] = py;
      a.pts[(pt0 + t) * 2] = px;
      a.pts[(pt0 + t) * 2 + 1] = py;
    }
    __syncthreads();
    stamp(1);
    // gen_sineembed_for_position: query q, point p, slot d -> column p * 64 + d of the K = 512 operand;
    // slots 2f and 2f + 1 share the angle (sin / cos); the padding queries' rows are zero
    char* EH = SA;  // [32][HP2] hi, then [32][HP2] lo
    for (int e = tid; e < QG * kP * 32; e += NT) {
      const int t = e >> 5, f = e & 31;  // t = q * P + p; f = coordinate half (y: 0..15, x: 16..31) x frequency
      const int q = t >> 3, p = t & 7;
      const float u = ((f < 16) ? SM[S_PTS + 2 * t + 1] : SM[S_PTS + 2 * t]) * 6.283185307179586f;
      const float ang = u / dim_t[f & 15];
      const int col = p * 64 + 2 * f;
      float sn, cs;
      sincosf(ang, &sn, &cs);  // one range reduction for the pair (the arguments reach ~380 rad)
      st_split(EH, HP2, q, col, sn);
      st_split(EH, HP2, q, col + 1, cs);
    }
    for (int e = tid; e < (32 - QG) * 512; e += NT) st_split(EH, HP2, QG + (e >> 9), e & 511, 0.f);
    __syncthreads();
    mk_f16 acc;
    zero_acc(acc);
    mk_gemm<32>(EH, EH + 32 * HP2 * 2, HP2, a.A.pa0, wave, 0, acc, 0, R, a.A.pa3, wave, 0);
    mk_epi<QG>(acc, a.A.pa0, wave, a.flags, [&](int row, int col, float v) { T1[row * FP + col] = fmaxf(v, 0.f); });
    __syncthreads();
    stamp(2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = wave + 8 * k;
      if (q >= QG) {  // padding rows (wave-uniform): zero operand rows, no LayerNorm
        st_split4(SA, HP, q, lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
        continue;
      }
      const float4 o = ln256(reinterpret_cast<const float4*>(T1 + q * FP)[lane], a.A.pa2g, a.A.pa2b, lane);
      st_split4(SA, HP, q, lane * 4, q < QG ? o : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    __syncthreads();
    stamp(3);
    zero_acc(acc);
    mk_gemm<16>(SA, SA + SPLIT_BYTES, HP, a.A.pa3, wave, 0, acc, 0, R, L.outp, wave, 0);
    mk_epi<QG>(acc, a.A.pa3, wave, a.flags, [&](int row, int col, float v) {
      if (row < QG) {
        X1[row * FP + col] = v;
        a.tfe[(int64_t)(row0 + row) * kD + col] = v;
      }
    });
  } else {
    for (int e = tid; e < QG * 64; e += NT) {
      const int q = e >> 6, c4 = (e & 63) * 4;
      *reinterpret_cast<float4*>(X1 + q * FP + c4) =
          *reinterpret_cast<const float4*>(a.tfe + (int64_t)(row0 + q) * kD + c4);
    }
    for (int t = tid; t < QGP; t += NT) {
      SM[S_PTS + 2 * t] = a.pts[(pt0 + t) * 2];
      SM[S_PTS + 2 * t + 1] = a.pts[(pt0 + t) * 2 + 1];
    }
  }
  __syncthreads();
  stamp(4);

  // ================================================================ GridSampleCrossBEVAttention
  // logits = attention_weights(query) (Linear 256 -> 8, fp32), softmax over the 8 points: the 8 weight
  // rows staged in LDS (SB is free here), a thread per (query, point) walking the two rows in LDS
  {
    float* AW = reinterpret_cast<float*>(SB);  // [8][FP]: padded rows, conflict-free across points
    for (int e = tid; e < kP * kD / 4; e += NT)
      *reinterpret_cast<float4*>(AW + (e >> 6) * FP + (e & 63) * 4) = reinterpret_cast<const float4*>(L.attw_w)[e];
    __syncthreads();
    if (tid < QGP) {
      const int q = tid >> 3, p = tid & 7;
      const float4* xr = reinterpret_cast<const float4*>(X1 + q * FP);
      const float4* wr = reinterpret_cast<const float4*>(AW + p * FP);
      float s0 = 0.f;
#pragma unroll 8
      for (int c = 0; c < kD / 4; ++c) {
        const float4 x = xr[c], w = wr[c];
        s0 += x.x * w.x;
        s0 += x.y * w.y;
        s0 += x.z * w.z;
        s0 += x.w * w.w;
      }
      SM[S_W8 + tid] = s0 + L.attw_b[p];
    }
    __syncthreads();
    if (tid < QG) {
      float* w = SM + S_W8 + tid * kP;
      float mx = -INFINITY;
      for (int p = 0; p < kP; ++p) mx = fmaxf(mx, w[p]);
      float e[kP], sm = 0.f;
      for (int p = 0; p < kP; ++p) {
        e[p] = expf(w[p] - mx);
        sm += e[p];
      }
      const float inv = 1.f / sm;
      for (int p = 0; p < kP; ++p) w[p] = e[p] * inv;
    }
  }
  __syncthreads();
  // sum_p w_p * bilinear(value, point p): one wave per query, a float4 of channels per lane; the value
  // rows are the gathered value_proj rows of the scene's distinct tap pixels (slots)
  for (int q = wave; q < 32; q += 8) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < QG) {
      int4 sl[kP];
#pragma unroll
      for (int p = 0; p < kP; ++p) sl[p] = SLOT[q * kP + p];
#pragma unroll
      for (int g = 0; g < kP; g += 4) {
        float4 v[4][4];
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
          const int sv[4] = {sl[g + pp].x, sl[g + pp].y, sl[g + pp].z, sl[g + pp].w};
#pragma unroll
          for (int u = 0; u < 4; ++u)  // slot -1 <=> the tap reads zero padding
            v[pp][u] = sv[u] >= 0 ? *reinterpret_cast<const float4*>(a.vrows + (int64_t)sv[u] * kD + lane * 4)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
          const int t = q * kP + g + pp;
          int x0, y0;
          float wt[4];
          tap_geom(SM[S_PTS + 2 * t], SM[S_PTS + 2 * t + 1], x0, y0, wt);
          float4 sp = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            sp.x += v[pp][u].x * wt[u];
            sp.y += v[pp][u].y * wt[u];
            sp.z += v[pp][u].z * wt[u];
            sp.w += v[pp][u].w * wt[u];
          }
          const float wp = SM[S_W8 + t];
          acc.x += wp * sp.x;
          acc.y += wp * sp.y;
          acc.z += wp * sp.z;
          acc.w += wp * sp.w;
        }
      }
      *reinterpret_cast<float4*>(a.gs_out + (int64_t)(row0 + q) * kD + lane * 4) = acc;
    }
    st_split4(SA, HP, q, lane * 4, acc);
  }
  __syncthreads();
  stamp(6);
  // output_proj + residual (blocks.py:127-129): x1 = W gso + b + query
  mk_f16 acc;
  zero_acc(acc);
  mk_gemm<16>(SA, SA + SPLIT_BYTES, HP, L.outp, wave, 0, acc, 0, R, L.ag_q, wave, 0);
  mk_epi<QG>(acc, L.outp, wave, a.flags, [&](int row, int col, float v) {
    float x = 0.f;
    if (row < QG) {
      x = v + X1[row * FP + col];
      X1[row * FP + col] = x;
    }
    st_split(SB, HP, row, col, x);
  });
  __syncthreads();
  stamp(7);

  // ================================================================ cross_agent_attention (+ norm1)
  zero_acc(acc);
  mk_gemm<16>(SB, SB + SPLIT_BYTES, HP, L.ag_q, wave, 0, acc, 0, R, L.ag_out, wave, 0);
  mk_epi<QG>(acc, L.ag_q, wave, a.flags, [&](int row, int col, float v) {
    if (row < QG) T1[row * FP + col] = v;
  });
  // the scene's agent K | V rows into the two split buffers (free until the output is written; the
  // barrier retires every wave's q-projection reads of SB first)
  __syncthreads();
  stamp(8);
  float* KV = reinterpret_cast<float*>(SA);
  {
    const float4* src = reinterpret_cast<const float4*>(a.akv + (int64_t)bp * kA * 2 * kD);
    for (int e = tid; e < kA * 2 * kD / 4; e += NT) reinterpret_cast<float4*>(KV)[e] = src[e];
  }
  __syncthreads();
  stamp(9);
  {
    // wave = head h, lane = (query i = lane & 31, half = lane >> 5): scores of keys half*15 .. +14
    const int h = wave, i = lane & 31, half = lane >> 5;
    const bool live = i < QG;
    float qv[kHD];
#pragma unroll
    for (int e = 0; e < kHD; e += 4) {
      const float4 v = live ? *reinterpret_cast<const float4*>(T1 + i * FP + h * kHD + e) : make_float4(0.f, 0.f, 0.f, 0.f);
      qv[e] = v.x;
      qv[e + 1] = v.y;
      qv[e + 2] = v.z;
      qv[e + 3] = v.w;
    }
    __syncthreads();  // every lane holds its query slice: T1 becomes the probability buffer
    stamp(10);
    const float scale = 1.0f / sqrtf((float)kHD);
    constexpr int KH = kA / 2;
    float sc[KH];
    float m = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < KH; ++jj) {
      const int j = half * KH + jj;
      const float* kr = KV + j * 2 * kD + h * kHD;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < kHD; ++e) d += qv[e] * kr[e];
      sc[jj] = d * scale;
      m = fmaxf(m, sc[jj]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int jj = 0; jj < KH; ++jj) {
      sc[jj] = expf(sc[jj] - m);
      sum += sc[jj];
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    // [head][query][key] probabilities of the live queries, pitch 33 (conflict-free column walk); the dead
    // lanes (padding queries) read a live row and their outputs are written as zeros
    float* pr = T1 + (h * QG + (live ? i : QG - 1)) * 33;
    if (live) {
#pragma unroll
      for (int jj = 0; jj < KH; ++jj) pr[half * KH + jj] = sc[jj] * inv;
    }
    __syncthreads();
    stamp(11);
    float o[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] = 0.f;
#ifdef DDMI_MK_NOPV
    for (int j = 0; j < 0; ++j) {
#else
#pragma unroll 6
    for (int j = 0; j < kA; ++j) {
#endif
      const float pj = pr[j];
      const float* vr = KV + j * 2 * kD + kD + h * kHD + half * 16;
#pragma unroll
      for (int d = 0; d < 16; ++d) o[d] += pj * vr[d];
    }
    __syncthreads();  // every lane is done with K / V: the split buffer takes the attention output
    stamp(12);
#pragma unroll
    for (int d = 0; d < 16; d += 4)
      st_split4(SA, HP, i, h * kHD + half * 16 + d,
                live ? make_float4(o[d], o[d + 1], o[d + 2], o[d + 3]) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
  __syncthreads();
  stamp(13);
  // out_proj + residual
  zero_acc(acc);
  mk_gemm<16>(SA, SA + SPLIT_BYTES, HP, L.ag_out, wave, 0, acc, 0, R, L.ffn0, wave, 0);
  mk_epi<QG>(acc, L.ag_out, wave, a.flags, [&](int row, int col, float v) {
    if (row < QG) X1[row * FP + col] = v + X1[row * FP + col];
  });
  __syncthreads();
  stamp(14);
  // norm1; cross_ego_attention over one key = the hoisted ego row, residual; norm2 -> FFN operand
  {
    const float4 eg = reinterpret_cast<const float4*>(a.ego + (int64_t)bp * kD)[lane];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = wave + 8 * k;
      if (q >= QG) {
        st_split4(SB, HP, q, lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
        continue;
      }
      float4 v = ln256(reinterpret_cast<const float4*>(X1 + q * FP)[lane], L.n1g, L.n1b, lane);
      v.x += eg.x;
      v.y += eg.y;
      v.z += eg.z;
      v.w += eg.w;
      const float4 o = ln256(v, L.n2g, L.n2b, lane);
      st_split4(SB, HP, q, lane * 4, q < QG ? o : make_float4(0.f, 0.f, 0.f, 0.f));
    }
  }
  __syncthreads();
  stamp(15);

  // ================================================================ FFN 256 -> 1024 -> 256, norm3, FiLM
  mk_f16 acc2;
  zero_acc(acc2);
  for (int c = 0; c < kFF / kD; ++c) {
    zero_acc(acc);
    mk_gemm<16>(SB, SB + SPLIT_BYTES, HP, L.ffn0, c * 8 + wave, 0, acc, 0, R, L.ffn2, wave, c * 16);
    mk_epi<QG>(acc, L.ffn0, c * 8 + wave, a.flags,
           [&](int row, int col, float v) { st_split(SA, HP, row, col - c * kD, row < QG ? fmaxf(v, 0.f) : 0.f); });
    __syncthreads();
    stamp(16 + 2 * c);
    const bool more = c + 1 < kFF / kD;
    mk_gemm<16>(SA, SA + SPLIT_BYTES, HP, L.ffn2, wave, c * 16, acc2, 0, R, more ? L.ffn0 : L.c0,
                more ? (c + 1) * 8 + wave : wave, 0);
    __syncthreads();
    stamp(17 + 2 * c);
  }
  mk_epi<QG>(acc2, L.ffn2, wave, a.flags, [&](int row, int col, float v) {
    if (row < QG) T1[row * FP + col] = v;
  });
  __syncthreads();
  stamp(24);
  {
    const float* film = a.film + (int64_t)b * a.film_stride;  // film_stride 0: one FiLM for the batch
    const float4 fs = reinterpret_cast<const float4*>(film)[lane];
    const float4 fb = reinterpret_cast<const float4*>(film + kD)[lane];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = wave + 8 * k;
      if (q >= QG) {
        st_split4(SB, HP, q, lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
        continue;
      }
      float4 o = ln256(reinterpret_cast<const float4*>(T1 + q * FP)[lane], L.n3g, L.n3b, lane);
      o.x = o.x * (1.f + fs.x) + fb.x;
      o.y = o.y * (1.f + fs.y) + fb.y;
      o.z = o.z * (1.f + fs.z) + fb.z;
      o.w = o.w * (1.f + fs.w) + fb.w;
      st_split4(SB, HP, q, lane * 4, q < QG ? o : make_float4(0.f, 0.f, 0.f, 0.f));
    }
  }
  __syncthreads();
  stamp(25);

  // ================================================================ task decoder: cls and reg branches
  zero_acc(acc);
  mk_gemm<16>(SB, SB + SPLIT_BYTES, HP, L.c0, wave, 0, acc, 0, R, L.r0, wave, 0);
  mk_epi<QG>(acc, L.c0, wave, a.flags, [&](int row, int col, float v) {
    if (row < QG) T1[row * FP + col] = fmaxf(v, 0.f);
  });
  zero_acc(acc);
  mk_gemm<16>(SB, SB + SPLIT_BYTES, HP, L.r0, wave, 0, acc, 0, R, L.c3, wave, 0);
  mk_epi<QG>(acc, L.r0, wave, a.flags, [&](int row, int col, float v) { st_split(SA, HP, row, col, row < QG ? fmaxf(v, 0.f) : 0.f); });
  __syncthreads();
  stamp(26);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = wave + 8 * k;
    if (q >= QG) {
      st_split4(SB, HP, q, lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
      continue;
    }
    const float4 o = ln256(reinterpret_cast<const float4*>(T1 + q * FP)[lane], L.c2g, L.c2b, lane);
    st_split4(SB, HP, q, lane * 4, q < QG ? o : make_float4(0.f, 0.f, 0.f, 0.f));
  }
  __syncthreads();
  stamp(27);
  zero_acc(acc);
  mk_gemm<16>(SB, SB + SPLIT_BYTES, HP, L.c3, wave, 0, acc, 0, R, L.r2, wave, 0);
  mk_epi<QG>(acc, L.c3, wave, a.flags, [&](int row, int col, float v) {
    if (row < QG) T1[row * FP + col] = fmaxf(v, 0.f);
  });
  zero_acc(acc);
  mk_gemm<16>(SA, SA + SPLIT_BYTES, HP, L.r2, wave, 0, acc, 0, R, none, 0, 0);
  mk_epi<QG>(acc, L.r2, wave, a.flags, [&](int row, int col, float v) {
    if (row < QG) X1[row * FP + col] = fmaxf(v, 0.f);
  });
  __syncthreads();
  stamp(28);
  // cls: LN, Linear 256 -> 1 (a wave per query); reg: Linear 256 -> 24 (a thread per output)
  {
    const float4 w = reinterpret_cast<const float4*>(L.c6_w)[lane];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // queries wave, wave + 8, wave + 16
      const int q = wave + 8 * k;
      if (q >= QG) break;
      const float4 o = ln256(reinterpret_cast<const float4*>(T1 + q * FP)[lane], L.c5g, L.c5b, lane);
      const float s = wave_sum((o.x * w.x + o.y * w.y) + (o.z * w.z + o.w * w.w));
      if (lane == 0 && q < QG) {
        const float c = s + L.c6_b[0];
        SM[S_CLS + q] = c;
        a.cls_out[row0 + q] = c;
        if constexpr (G > 1) st_x(a.cls_x + b * 32 + q0 + q, c);
      }
    }
  }

  {
    float* RW = reinterpret_cast<float*>(SA);  // r4 weights [24][FP]: padded rows, conflict-free across outputs
    for (int e = tid; e < kP * 3 * kD / 4; e += NT)
      *reinterpret_cast<float4*>(RW + (e >> 6) * FP + (e & 63) * 4) = reinterpret_cast<const float4*>(L.r4_w)[e];
    __syncthreads();
    if (tid < QG * kP * 3) {
      const int q = tid / (kP * 3), o = tid - q * (kP * 3);
      const float4* xr = reinterpret_cast<const float4*>(X1 + q * FP);
      const float4* wr = reinterpret_cast<const float4*>(RW + o * FP);
      float s0 = 0.f;
#pragma unroll 8
      for (int c = 0; c < kD / 4; ++c) {
        const float4 x = xr[c], w = wr[c];
        s0 += x.x * w.x;
        s0 += x.y * w.y;
        s0 += x.z * w.z;
        s0 += x.w * w.w;
      }
      SM[S_RR + tid] = s0 + L.r4_b[o];
    }
  }
  __syncthreads();
  // reg[..., :2] += points; reg[..., 2] = tanh * pi (transfuser_model_v2.py:376-380)
  for (int t = tid; t < QGP; t += NT) {
    const float* rr = SM + S_RR + t * 3;
    const float x = rr[0] + SM[S_PTS + 2 * t];
    const float y = rr[1] + SM[S_PTS + 2 * t + 1];
    const float hd = tanhf(rr[2]) * 3.14159265358979323846f;
    float* ro = a.reg_out + (pt0 + t) * 3;
    if constexpr (G > 1) {
      st_x(ro, x);
      st_x(ro + 1, y);
      st_x(ro + 2, hd);
    } else {
      ro[0] = x;
      ro[1] = y;
      ro[2] = hd;
    }
    SM[S_REG + 3 * t] = x;
    SM[S_REG + 3 * t + 1] = y;
    SM[S_REG + 3 * t + 2] = hd;
    SM[S_PN + 2 * t] = x;
    SM[S_PN + 2 * t + 1] = y;
    if (a.pts_next) {
      if constexpr (G > 1) {
        st_x(a.pts_next + (pt0 + t) * 2, x);
        st_x(a.pts_next + (pt0 + t) * 2 + 1, y);
      } else {
        a.pts_next[(pt0 + t) * 2] = x;
        a.pts_next[(pt0 + t) * 2 + 1] = y;
      }
    }
  }
  __syncthreads();
  stamp(30);

  // ================================================================ DDIM step / mode selection / next taps
  if (a.layer == 1 && a.ddim) {
    for (int t = tid; t < QGP; t += NT) {
      float* im = a.imgx + (pt0 + t) * 2;
      const float x0x = norm_x(SM[S_REG + 3 * t]);
      const float x0y = norm_y(SM[S_REG + 3 * t + 1]);
      const float ex = (im[0] - a.sa_t * x0x) / a.sb_t;
      const float ey = (im[1] - a.sa_t * x0y) / a.sb_t;
      const float cx = fminf(fmaxf(x0x, -1.f), 1.f);
      const float cy = fminf(fmaxf(x0y, -1.f), 1.f);
      const float nx = a.sa_p * cx + a.sdir * ex;
      const float ny = a.sa_p * cy + a.sdir * ey;
      im[0] = nx;
      im[1] = ny;
      // the next step's points (traj_embed arithmetic)
      SM[S_PN + 2 * t] = denorm_x(fminf(fmaxf(nx, -1.f), 1.f));
      SM[S_PN + 2 * t + 1] = denorm_y(fminf(fmaxf(ny, -1.f), 1.f));
    }
    __syncthreads();
    stamp(31);
  }
  if constexpr (G > 1) {
    // the scene-level tail (mode selection, the next taps' dedup) needs every group's queries: each group publishes
    // its next points (the DDIM-updated points at a step's layer 1; pts_next holds layer 0's), all its published
    // words sc1 (st_x), drains them and arrives at the scene's counter; the last to arrive (told by its add's return)
    // reads the scene's cls / reg / next points back with sc1 loads and runs the tail, then resets the counter for
    // the next launch. An add that returns G or more found a counter this launch did not start from zero (the tail
    // would run twice or never): DD_NUM_SYNC_STATE.
    if (a.layer == 1 && a.ddim)
      for (int t = tid; t < QGP; t += NT) {
        st_x(a.next_pts + (pt0 + t) * 2, SM[S_PN + 2 * t]);
        st_x(a.next_pts + (pt0 + t) * 2 + 1, SM[S_PN + 2 * t + 1]);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int last;
    if (tid == 0) {
      const unsigned old = __hip_atomic_fetch_add(a.scene_cnt + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old >= (unsigned)G && a.flags) atomicOr(a.flags, DD_NUM_SYNC_STATE);
      last = old == (unsigned)(G - 1);
      if (last) __hip_atomic_store(a.scene_cnt + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    const float* np = (a.layer == 1 && a.ddim) ? a.next_pts : a.pts_next;
    for (int t = tid; t < kQP; t += NT) {
      if (a.traj) {
        const float* ro = a.reg_out + ((int64_t)b * kQP + t) * 3;
        SM[S_REG + 3 * t] = ld_x(ro);
        SM[S_REG + 3 * t + 1] = ld_x(ro + 1);
        SM[S_REG + 3 * t + 2] = ld_x(ro + 2);
      }
      if (a.next_rows && np) {
        SM[S_PN + 2 * t] = ld_x(np + ((int64_t)b * kQP + t) * 2);
        SM[S_PN + 2 * t + 1] = ld_x(np + ((int64_t)b * kQP + t) * 2 + 1);
      }
    }
    if (tid < kQ) SM[S_CLS + tid] = ld_x(a.cls_x + b * 32 + tid);
    __syncthreads();
  }
  if (a.traj && tid == 0) {
    int best = 0;
    float bv = SM[S_CLS];
    for (int q = 1; q < kQ; ++q) {
      const float v = SM[S_CLS + q];
      if (v > bv || (v != v && bv == bv)) {  // first maximal index; NaN propagates like torch.argmax
        bv = v;
        best = q;
      }
    }
    if (a.mode_idx) a.mode_idx[b] = best;
    for (int e = 0; e < kP * 3; ++e) a.traj[(int64_t)b * kP * 3 + e] = SM[S_REG + best * kP * 3 + e];
  }
  if (a.next_rows) {
    int* table = reinterpret_cast<int*>(T1);
    dedup_scene(SM + S_PN, table, table + 4096, b, bp, a.next_rows, a.next_slots, a.next_counts);
  }
#ifdef DDMI_MK_STAMPS
  stamp(32);
  if (a.stamps && tid < 40 && G == 1) a.stamps[(int64_t)b * 40 + tid] = st_lds[tid];
#endif
}

// DDIM add_noise at the truncation step (:591-597), the first step's points and their tap dedup
__global__ __launch_bounds__(256) void decoder_mk_init_kernel(MkInitArgs a) {
  __shared__ float pts[2 * kQP];
  __shared__ int table[4096 + 256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float sa = a.sa_b ? a.sa_b[b] : a.sa, s1a = a.s1a_b ? a.s1a_b[b] : a.s1a;  // per scene: training head
  for (int t = tid; t < kQP; t += 256) {
    const int64_t i = (int64_t)b * kQP + t;
    const float ax = a.anchor[t * 2], ay = a.anchor[t * 2 + 1];
    const float ix = sa * norm_x(ax) + s1a * a.noise[i * 2];
    const float iy = sa * norm_y(ay) + s1a * a.noise[i * 2 + 1];
    a.imgx[i * 2] = ix;
    a.imgx[i * 2 + 1] = iy;
    pts[2 * t] = denorm_x(fminf(fmaxf(ix, -1.f), 1.f));
    pts[2 * t + 1] = denorm_y(fminf(fmaxf(iy, -1.f), 1.f));
  }
  __syncthreads();
  dedup_scene(pts, table, table + 4096, b, b / a.samples, a.rows, a.slots, a.counts);
}

// GEMM-core test: A [32][K] fp32 -> split LDS image -> mk_gemm over 256-column units -> out
__global__ __launch_bounds__(NT, 1) void mk_linear_test_kernel(const float* __restrict__ A, int K, MkLin W, int N,
                                                               float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int hp = K + 8;
  for (int e = tid; e < 32 * K; e += NT) st_split(lds, hp, e / K, e % K, A[e]);
  __syncthreads();
  const MkLin none{};
  for (int nt = wave; nt < N / 32; nt += 8) {
    mk_f16 acc;
    zero_acc(acc);
    Ring R;
    ring_fill(R, W, nt, 0);
    for (int ks = 0; ks < K / 16; ks += 16)
      mk_gemm<16>(lds, lds + 32 * hp * 2, hp, W, nt, ks, acc, ks, R, ks + 16 < K / 16 ? W : none, nt, ks + 16);
    mk_epi<kQ>(acc, W, nt, nullptr, [&](int row, int col, float v) { out[row * N + col] = v; });
  }
}

// pull a read-only range into the caches (MALL / L2) ahead of its first real use: every lane reads 16-B
// pieces; the sum is stored only if it equals a value it cannot take, so the loads are kept
__global__ __launch_bounds__(256) void mk_prefetch_kernel(const float4* __restrict__ p, int64_t n4, float* sink) {
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = p[i];
    acc += v.x + v.w;
  }
  if (acc == -1.2345e-38f && sink) *sink = acc;
}

}  // namespace

void launch_mk_prefetch(const void* p, size_t bytes, hipStream_t st) {
  const int64_t n4 = (int64_t)(bytes / 16);
  if (n4 <= 0) return;
  hipLaunchKernelGGL(mk_prefetch_kernel, dim3(256), dim3(256), 0, st, reinterpret_cast<const float4*>(p), n4,
                     (float*)nullptr);
  DD_HIP_CHECK(hipGetLastError());
}

void pack_mk_weights(const float* w, int nout, int nin, std::vector<_Float16>& pk, std::vector<float>& sinv) {
  if (nin % 16 || nout % 32) throw std::runtime_error("pack_mk_weights: nin % 16 / nout % 32");
  const int nnt = nout / 32, nks = nin / 16;
  std::vector<float> scale(nout, 1.f);
  sinv.assign(nout, 1.f);
  for (int r = 0; r < nout; ++r) {
    float amax = 0.f;
    for (int k = 0; k < nin; ++k) amax = std::max(amax, std::fabs(w[(size_t)r * nin + k]));
    int e = 0;
    if (amax > 0.f && std::isfinite(amax)) {
      int ex;
      std::frexp(amax, &ex);
      e = std::min(15 - ex, kSplitMaxExp);  // as prep_split
    }
    scale[r] = std::ldexp(1.0f, e);
    sinv[r] = std::ldexp(1.0f, -e);
  }
  pk.assign((size_t)nnt * nks * 64 * 16, (_Float16)0.f);
  for (int nt = 0; nt < nnt; ++nt)
    for (int ks = 0; ks < nks; ++ks)
      for (int lane = 0; lane < 64; ++lane) {
        const int col = nt * 32 + (lane & 31);
        _Float16* dst = pk.data() + (((size_t)nt * nks + ks) * 64 + lane) * 16;
        for (int e = 0; e < 8; ++e) {
          const int k = ks * 16 + 8 * (lane >> 5) + e;
          const float v = w[(size_t)col * nin + k] * scale[col];
          const _Float16 h = (_Float16)v;
          dst[e] = h;
          dst[8 + e] = (_Float16)(v - (float)h);
        }
      }
}

void launch_mk_linear_test(const float* A, int K, const MkLin& W, int N, float* out, hipStream_t st) {
  if (K % 256 || N % 32 || W.nks != K / 16) throw std::runtime_error("mk_linear_test: K % 256, N % 32");
  const size_t lds = (size_t)2 * 32 * (K + 8) * 2;
  DD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mk_linear_test_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(mk_linear_test_kernel, dim3(1), dim3(NT), lds, st, A, K, W, N, out);
  DD_HIP_CHECK(hipGetLastError());
}

bool decoder_mk_supported(int Q, int P, int d, int nagents, int Hv, int Wv, int ffn) {
  return Q == kQ && P == kP && d == kD && nagents == kA && Hv == kHV && Wv == kHV && ffn == kFF;
}

void launch_decoder_mk(const MkArgs& a, hipStream_t st) {
  if (a.B <= 0) return;
  if (a.samples < 1 || a.B % a.samples) throw std::runtime_error("decoder_mk: B must be a multiple of samples");
  if (!a.dim_t || !a.slots || !a.vrows || !a.akv || !a.ego || !a.film || !a.tfe || !a.pts || !a.imgx)
    throw std::runtime_error("decoder_mk: missing operand");
  if (a.groups != 1 && (!a.scene_cnt || !a.cls_x || (a.layer == 1 && a.ddim && !a.next_pts) ||
                        (a.next_rows && a.layer == 0 && !a.pts_next)))
    throw std::runtime_error("decoder_mk: query groups need the scene counters and the next-point buffers");
  static std::atomic<uint64_t> attr[3];
  auto go = [&](auto kern, int i, int g) {
    set_max_lds_once(attr[i], reinterpret_cast<const void*>(kern), LDS_BYTES);
    hipLaunchKernelGGL(kern, dim3(a.B * g), dim3(NT), LDS_BYTES, st, a);
  };
  switch (a.groups) {
    case 1: go(decoder_mk_kernel<20>, 0, 1); break;
    case 2: go(decoder_mk_kernel<10>, 1, 2); break;
    case 4: go(decoder_mk_kernel<5>, 2, 4); break;
    default: throw std::runtime_error("decoder_mk: groups must be 1, 2 or 4");
  }
  DD_HIP_CHECK(hipGetLastError());
}

void launch_decoder_mk_init(const MkInitArgs& a, hipStream_t st) {
  if (a.B <= 0) return;
  if (a.samples < 1 || a.B % a.samples) throw std::runtime_error("decoder_mk_init: B must be a multiple of samples");
  hipLaunchKernelGGL(decoder_mk_init_kernel, dim3(a.B), dim3(256), 0, st, a);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
