// PDM comfort metrics on the device (dd_comfort, include/ddmi.h): NAVSIM's ego_is_comfortable
// (pdm_planner/scoring/pdm_comfort_metrics.py:313-336) over the (N, 41, 11) float64 states dd_simulate writes, read in
// place. float64 throughout; built with -ffp-contract=off (np.round's multiply and the unwrap's 2 pi * k are separate
// roundings in the reference). Deterministic: no atomics, every sum in a fixed order. One launch, no scratch.
//
// Every signal is a Savitzky-Golay filter in scipy's mode "interp" followed by np.round(., 8):
//   window 41 = the whole series (lon / lat acceleration, and the derivative of the jerk signals): ONE least-squares
//     quadratic per series, every output read off it (scipy convolves for sample 20 alone, which is the same
//     polynomial's value). Fitted in the orthogonal basis 1, x, x^2 - 140 on x = t - 20 (sum x^2 = 5740 = 41 * 140,
//     sum (x^2 - 140)^2 = 641732): three moments per series, no normal matrix to invert, each coefficient a ratio
//     of a 41-term sum and an exact integer. Lane t forms its three products and the wavefront sums them by an xor
//     butterfly (the same order in every call, the same bits in every lane); a serial loop over LDS, one dependent
//     float64 add per sample and moment, made the kernel issue-bound.
//   window 8 (the jerk signals' pre-smoothing, even: fitted half a sample off the grid, output i reads samples
//     i - 3 .. i + 4) and window 5 (the yaw signals): banded. Output i < window / 2 (and the mirrored last ones) read
//     the polynomial fitted to the first (last) `window` samples. The host forms the rows once per call in long double
//     from the call's delta (comfort_tables) and passes them by value.
// Layout: one candidate per wavefront, four per workgroup. The candidate's 451 doubles are read coalesced into LDS;
// lane t then owns sample t of every series.
#include <cmath>
#include <limits>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int CT = 41;             // samples per candidate
constexpr int CNS = 11;            // StateIndex size
constexpr int CROW = CT * CNS;     // doubles per candidate
constexpr int CWAVES = 4;          // candidates per workgroup
constexpr int CH = 2, CAX = 5, CAY = 6;
constexpr double FIT_S2 = 5740.0;     // sum x^2, x = -20..20
constexpr double FIT_P2 = 641732.0;   // sum (x^2 - 140)^2
constexpr double FIT_MEAN2 = 140.0;   // FIT_S2 / 41

struct ComfortTables {
  double lo[6], hi[6];   // effective bounds: -inf / +inf where the parameter is 0
  double delta;
  // rows 0..3: outputs 0..3 over samples 0..7; row 4: interior output i over samples i-3..i+4; rows 5..8: outputs
  // 37..40 over samples 33..40
  double pre[9][8];
  // rows 0, 1: outputs 0, 1 over samples 0..4; row 2: interior over i-2..i+2; rows 3, 4: outputs 39, 40 over 36..40
  double yaw_accel[5][5];
  double yaw_rate[5][5];
};

// Rows of the least-squares operator of a `window`-sample, degree-`order` fit: out[r][j] = weight of window sample j
// in the deriv-th derivative (per delta^deriv) of the fitted polynomial at window position at[r].
void fit_rows(int window, int order, int deriv, double delta, const double* at, int rows, double* out) {
  typedef long double ld;
  const int K = order + 1;
  const ld c = (ld)(window - 1) / 2;
  ld G[4][4], P[4][8];   // normal matrix, then P = G^-1 A^T (K x window)
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b) {
      ld s = 0;
      for (int j = 0; j < window; ++j) s += std::pow((ld)j - c, a + b);
      G[a][b] = s;
    }
  for (int j = 0; j < window; ++j) {
    ld M[4][5];
    for (int a = 0; a < K; ++a) {
      for (int b = 0; b < K; ++b) M[a][b] = G[a][b];
      M[a][K] = std::pow((ld)j - c, a);
    }
    for (int k = 0; k < K; ++k) {   // Gauss-Jordan with partial pivoting
      int piv = k;
      for (int a = k + 1; a < K; ++a)
        if (std::fabs(M[a][k]) > std::fabs(M[piv][k])) piv = a;
      for (int b = 0; b <= K; ++b) std::swap(M[k][b], M[piv][b]);
      for (int a = 0; a < K; ++a) {
        if (a == k) continue;
        const ld f = M[a][k] / M[k][k];
        for (int b = k; b <= K; ++b) M[a][b] -= f * M[k][b];
      }
    }
    for (int a = 0; a < K; ++a) P[a][j] = M[a][K] / M[a][a];
  }
  ld scale = 1;
  for (int d = 0; d < deriv; ++d) scale /= (ld)delta;
  for (int r = 0; r < rows; ++r) {
    const ld x = (ld)at[r] - c;
    for (int j = 0; j < window; ++j) {
      ld s = 0;
      for (int k = deriv; k < K; ++k) {
        ld f = 1;   // k! / (k - deriv)!
        for (int d = 0; d < deriv; ++d) f *= (ld)(k - d);
        s += f * std::pow(x, k - deriv) * P[k][j];
      }
      out[r * window + j] = (double)(s * scale);
    }
  }
}

// np.diff(np.arange(41) * dt).mean() as numpy sums it: 40 addends in eight interleaved partial sums, combined pairwise.
double mean_step(double dt) {
  double d[CT - 1], r[8];
  for (int i = 0; i < CT - 1; ++i) d[i] = (double)(i + 1) * dt - (double)i * dt;
  for (int k = 0; k < 8; ++k) r[k] = d[k];
  for (int i = 8; i < CT - 1; i += 8)
    for (int k = 0; k < 8; ++k) r[k] += d[i + k];
  return (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) / (double)(CT - 1);
}

ComfortTables comfort_tables(const dd_comfort_params& p) {
  ComfortTables tb;
  const double inf = std::numeric_limits<double>::infinity();
  const double lo[6] = {p.min_lon_accel,     -p.max_abs_lat_accel, -p.max_abs_mag_jerk,
                        -p.max_abs_lon_jerk, -p.max_abs_yaw_accel, -p.max_abs_yaw_rate};
  const double hi[6] = {p.max_lon_accel,    p.max_abs_lat_accel, p.max_abs_mag_jerk,
                        p.max_abs_lon_jerk, p.max_abs_yaw_accel, p.max_abs_yaw_rate};
  for (int k = 0; k < 6; ++k) {   // _within_bound: `min_bound if min_bound else -inf`
    tb.lo[k] = lo[k] != 0.0 ? lo[k] : -inf;
    tb.hi[k] = hi[k] != 0.0 ? hi[k] : inf;
  }
  tb.delta = mean_step(p.dt);
  const double at8[9] = {0, 1, 2, 3, 3.5, 4, 5, 6, 7};
  const double at5[5] = {0, 1, 2, 3, 4};
  fit_rows(8, 2, 0, tb.delta, at8, 9, &tb.pre[0][0]);
  fit_rows(5, 3, 2, tb.delta, at5, 5, &tb.yaw_accel[0][0]);
  fit_rows(5, 2, 1, tb.delta, at5, 5, &tb.yaw_rate[0][0]);
  return tb;
}

// np.round(v, 8)
__device__ inline double round8(double v) { return rint(v * 1e8) / 1e8; }

// Sum of v over the wavefront's 64 lanes by an xor butterfly: a fixed order, and every lane ends with the same bits
// (each step adds the same two partial sums in both partners).
__device__ inline double wave_sum(double v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// The fitted quadratic's coefficients in the basis 1, x, x^2 - 140 of the 41-sample series of which this lane holds
// sample v at abscissa x (p2 = x^2 - 140); lanes past the series (row false) add exact zeros.
__device__ inline void fit_moments(double v, double x, double p2, bool row, double& a0, double& a1, double& a2) {
  v = row ? v : 0.0;
  a0 = wave_sum(v) / (double)CT, a1 = wave_sum(x * v) / FIT_S2, a2 = wave_sum(p2 * v) / FIT_P2;
}

// Inclusive prefix sum over the lanes (Hillis-Steele). The addends are whole numbers of turns, so every order gives
// cumsum's result exactly; a NaN reaches every later lane, as in cumsum.
__device__ inline double wave_cumsum(double v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const double u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

__device__ inline double banded(const double* w, const double* y, int taps) {
  double s = 0.0;
  for (int j = 0; j < taps; ++j) s += w[j] * y[j];
  return s;
}

__global__ __launch_bounds__(64 * CWAVES) void comfort_kernel(const double* __restrict__ states, int N,
                                                              ComfortTables tb, uint8_t* __restrict__ flags,
                                                              double* __restrict__ signals) {
  __shared__ double sRaw[CWAVES][CROW + 1];
  __shared__ double sV[CWAVES][3][64];
  __shared__ double sPre[9 * 8], sYa[5 * 5], sYr[5 * 5];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = blockIdx.x * CWAVES + wave;
  const bool live = slot < N;
  const int n = live ? slot : N - 1;   // a spare wavefront repeats the last candidate (uniform barriers), stores none
  const bool row = lane < CT;
  const int t = row ? lane : CT - 1;   // a spare lane repeats sample 40, stores nothing
  double* raw = sRaw[wave];
  double* v0 = sV[wave][0];
  double* v1 = sV[wave][1];
  double* v2 = sV[wave][2];

  const double* S = states + (size_t)n * CROW;
  for (int i = lane; i < CROW; i += 64) raw[i] = S[i];
  if (threadIdx.x < 72) sPre[threadIdx.x] = (&tb.pre[0][0])[threadIdx.x];
  if (threadIdx.x < 25) {
    sYa[threadIdx.x] = (&tb.yaw_accel[0][0])[threadIdx.x];
    sYr[threadIdx.x] = (&tb.yaw_rate[0][0])[threadIdx.x];
  }
  __syncthreads();
  const double h = raw[t * CNS + CH], ax = raw[t * CNS + CAX], ay = raw[t * CNS + CAY];
  v0[lane] = ax, v1[lane] = hypot(ax, ay), v2[lane] = h;
  __syncthreads();

  const double x = (double)(t - 20), p2 = x * x - FIT_MEAN2;
  const double two_pi = 2.0 * M_PI;
  double sig[6], a0, a1, a2;
  fit_moments(ax, x, p2, row, a0, a1, a2);
  sig[0] = round8(a0 + a1 * x + a2 * p2);
  fit_moments(ay, x, p2, row, a0, a1, a2);
  sig[1] = round8(a0 + a1 * x + a2 * p2);
  // window 8: which row of the table, and the first sample it reads
  const int prow = t < 4 ? t : (t > 36 ? t - 32 : 4), pbase = t < 4 ? 0 : (t > 36 ? 33 : t - 3);
  const double a8x = round8(banded(sPre + prow * 8, v0 + pbase, 8));
  const double a8m = round8(banded(sPre + prow * 8, v1 + pbase, 8));
  fit_moments(a8m, x, p2, row, a0, a1, a2);
  sig[2] = round8((a1 + a2 * (2.0 * x)) / tb.delta);
  fit_moments(a8x, x, p2, row, a0, a1, a2);
  sig[3] = round8((a1 + a2 * (2.0 * x)) / tb.delta);
  // _phase_unwrap: this sample's whole turns against the one before, then cumsum
  const double turn = t >= 1 ? rint((h - v2[t >= 1 ? t - 1 : 0]) / two_pi) : 0.0;
  const double unwrapped = h - two_pi * wave_cumsum(turn, lane);
  __syncthreads();   // every window of v0 has been read
  v0[lane] = unwrapped;
  __syncthreads();

  const int yrow = t < 2 ? t : (t > 38 ? t - 36 : 2), ybase = t < 2 ? 0 : (t > 38 ? 36 : t - 2);
  sig[4] = round8(banded(sYa + yrow * 5, v0 + ybase, 5));
  sig[5] = round8(banded(sYr + yrow * 5, v0 + ybase, 5));

  unsigned pass = 0;
  for (int k = 0; k < 6; ++k) {
    const bool out = row && !(sig[k] > tb.lo[k] && sig[k] < tb.hi[k]);   // false comparisons on NaN: out of bounds
    if (__ballot(out) == 0ull) pass |= 1u << k;
  }
  if (!live) return;
  if (lane < 6) flags[(size_t)n * 6 + lane] = (uint8_t)((pass >> lane) & 1u);
  if (signals && row)
    for (int k = 0; k < 6; ++k) signals[((size_t)n * 6 + k) * CT + lane] = sig[k];
}

}  // namespace

void launch_comfort(const double* states, int N, const dd_comfort_params& p, uint8_t* out_flags, double* out_signals,
                    hipStream_t st) {
  const ComfortTables tb = comfort_tables(p);
  hipLaunchKernelGGL(comfort_kernel, dim3((unsigned)((N + CWAVES - 1) / CWAVES)), dim3(64 * CWAVES), 0, st, states, N,
                     tb, out_flags, out_signals);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
