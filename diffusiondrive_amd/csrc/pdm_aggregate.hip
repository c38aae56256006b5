// PDM progress along the centerline and the score's aggregation on the device (dd_progress, dd_pdm_aggregate,
// include/ddmi.h): PDMScorer._calculate_progress (pdm_planner/scoring/pdm_scorer.py:398-412, PDMPath.project,
// utils/pdm_path.py:61-65) and _aggregate_scores (:156-183). float64 throughout; built with -ffp-contract=off (the
// aggregation is separate numpy products and sums, and the projection's cross terms must round alike for every
// segment). Deterministic: no atomics, every sum in a fixed order.
#include <cmath>
#include <limits>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int PT = 41;    // states per candidate
constexpr int PNS = 11;   // StateIndex size
constexpr int PTHREADS = 256;

// One thread per candidate: both centers walk the scene's polyline once, segment by segment, with the running length
// of the segments passed. shapely's LineString.project as GEOS is remembered to do it: the nearest segment (strictly
// nearer than every earlier one: the first on a tie), the parameter clamped to [0, 1], the summed lengths before it
// plus the partial length. Everything is a difference against the segment's start. A NaN center is nearer to nothing
// and projects to NaN.
__global__ __launch_bounds__(PTHREADS) void progress_kernel(const double* __restrict__ states, int N, int per_group,
                                                           const double* __restrict__ verts,
                                                           const int32_t* __restrict__ scene_off, double r,
                                                           double* __restrict__ out) {
  const int n = blockIdx.x * PTHREADS + threadIdx.x;
  if (n >= N) return;
  const int g = n / per_group;
  const int v0 = scene_off[g], v1 = scene_off[g + 1];
  double qx[2], qy[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const double* S = states + ((size_t)n * PT + (e ? PT - 1 : 0)) * PNS;
    qx[e] = S[0] + r * cos(S[2]), qy[e] = S[1] + r * sin(S[2]);
  }
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double best[2] = {inf, inf}, at[2] = {nan, nan};
  double passed = 0.0;
  double ax = verts[2 * (size_t)v0], ay = verts[2 * (size_t)v0 + 1];
  for (int v = v0 + 1; v < v1; ++v) {
    const double bx = verts[2 * (size_t)v], by = verts[2 * (size_t)v + 1];
    const double dx = bx - ax, dy = by - ay;
    const double len2 = dx * dx + dy * dy, len = sqrt(len2);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double wx = qx[e] - ax, wy = qy[e] - ay;
      double s = len2 > 0.0 ? (wx * dx + wy * dy) / len2 : 0.0;
      s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);   // keeps a NaN
      const double ex = wx - s * dx, ey = wy - s * dy;
      const double d2 = ex * ex + ey * ey;
      if (d2 < best[e]) best[e] = d2, at[e] = passed + s * len;
    }
    passed += len;
    ax = bx, ay = by;
  }
  const double d = at[1] - at[0];
  out[n] = d < 0.0 ? 0.0 : d;   // np.clip(., 0, None): a NaN stays
}

// max that propagates NaN, as np.max does
__device__ inline double nan_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

struct AggConsts {
  double wp, wt, wc, wd, wsum, threshold;
};

// One workgroup per scene: the NaN-keeping max of p = raw * multi over the scene's candidates (a butterfly per
// wavefront, then the four wavefronts' through LDS: the order is fixed), or with a reference the pair's max per
// candidate; then the progress term and the score.
__global__ __launch_bounds__(PTHREADS) void aggregate_kernel(
    const double* __restrict__ no_collision, const double* __restrict__ drivable_area,
    const double* __restrict__ driving_direction, const double* __restrict__ raw_progress,
    const double* __restrict__ ttc, const uint8_t* __restrict__ comfort, int per_group, AggConsts k,
    const double* __restrict__ reference, double* __restrict__ out_score, double* __restrict__ out_progress) {
  __shared__ double sMax[PTHREADS / 64];
  const int g = blockIdx.x;
  const size_t first = (size_t)g * per_group;
  const double ninf = -std::numeric_limits<double>::infinity();
  double group_max = ninf;
  if (!reference) {
    double m = ninf;
    for (int i = threadIdx.x; i < per_group; i += PTHREADS) {
      const size_t n = first + i;
      m = nan_max(m, raw_progress[n] * (no_collision[n] * drivable_area[n]));
    }
    for (int s = 1; s < 64; s <<= 1) m = nan_max(m, __shfl_xor(m, s));
    if ((threadIdx.x & 63) == 0) sMax[threadIdx.x >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < PTHREADS / 64; ++w) group_max = nan_max(group_max, sMax[w]);
  }
  for (int i = threadIdx.x; i < per_group; i += PTHREADS) {
    const size_t n = first + i;
    const double multi = no_collision[n] * drivable_area[n];
    const double p = raw_progress[n] * multi;
    const double pmax = reference ? nan_max(reference[g], p) : group_max;
    const double progress = pmax > k.threshold ? p / pmax : (multi == 0.0 ? 0.0 : 1.0);
    const uint8_t* c = comfort + 6 * n;
    const double comfortable = (c[0] && c[1] && c[2] && c[3] && c[4] && c[5]) ? 1.0 : 0.0;
    const double weighted =
        (((progress * k.wp) + (ttc[n] * k.wt)) + (comfortable * k.wc)) + (driving_direction[n] * k.wd);
    out_progress[n] = progress;
    out_score[n] = multi * (weighted / k.wsum);
  }
}

}  // namespace

void launch_progress(const double* states, int N, int per_group, const dd_centerlines& lines,
                     double rear_axle_to_center, double* out_raw, hipStream_t st) {
  hipLaunchKernelGGL(progress_kernel, dim3((unsigned)((N + PTHREADS - 1) / PTHREADS)), dim3(PTHREADS), 0, st, states, N,
                     per_group, lines.verts, lines.scene_off, rear_axle_to_center, out_raw);
  DD_HIP_CHECK(hipGetLastError());
}

void launch_pdm_aggregate(const double* no_collision, const double* drivable_area, const double* driving_direction,
                          const double* raw_progress, const double* ttc, const uint8_t* comfort, int N, int per_group,
                          const dd_score_params& sp, const double* progress_reference, double* out_score,
                          double* out_progress, hipStream_t st) {
  AggConsts k;
  k.wp = sp.progress_weight, k.wt = sp.ttc_weight, k.wc = sp.comfortable_weight, k.wd = sp.driving_direction_weight;
  k.wsum = ((k.wp + k.wt) + k.wc) + k.wd;
  k.threshold = sp.progress_distance_threshold;
  hipLaunchKernelGGL(aggregate_kernel, dim3((unsigned)(N / per_group)), dim3(PTHREADS), 0, st, no_collision,
                     drivable_area, driving_direction, raw_progress, ttc, comfort, per_group, k, progress_reference,
                     out_score, out_progress);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
