// PDM proposal simulation on the device (dd_simulate / dd_simulate_proposals, include/ddmi.h): NAVSIM's
// PDMSimulator.simulate_proposals (pdm_planner/simulation/pdm_simulator.py:32-79) for N candidate trajectories - the
// batch LQR tracker (batch_lqr.py, batch_lqr_utils.py) closed over the kinematic bicycle model
// (batch_kinematic_bicycle.py) for 40 steps of 0.1 s. float64 throughout, as the reference: the curvature fit
// regularises with 1e-10, its normal matrix reaches cond ~1e8 for a plan that barely moves, and nuPlan's global
// coordinates are ~4e6 m. Built with -ffp-contract=off. Deterministic: no atomics, every sum in a fixed order.
//
// Launch sequence (all on the caller's stream, scratch in the caller's `work`):
//   sim_factor_kernel    Cholesky factor of the velocity fit's normal matrix L^T L + jerk_penalty R^T R. The design
//                        matrix's rows are (cos h_i, sin h_i) x L[i] with L lower triangular (column 0 = dt, the others
//                        dt^2), so A^T A = L^T L whatever the candidate: one constant 40 x 40 per launch. R is what
//                        _make_banded_difference_matrix (batch_lqr_utils.py:59-70) really returns - its second slice
//                        assignment overwrites the first's +1 entries, leaving -1 at (r, r + 1) and a single +1 at
//                        (37, 39) - so R^T R = diag(0, 1, ..., 1) with -1 at (38, 39) and (39, 38).
//   sim_knots_kernel     dd_simulate only: the 41-pose proposal from the planner's 8 ego-frame poses.
//   sim_fit_kernel       one candidate per wavefront: the velocity fit (a solve against the constant factor), then the
//                        curvature fit, whose normal matrix depends on the candidate's velocity profile: built in
//                        closed form in LDS (A[i][0] = v_i dt, A[i][j] = v_i dt^2 for 1 <= j <= i - the reference
//                        scales the ROWS of the triangle, batch_lqr_utils.py:165-168 - so A^T A[j][k] is a suffix sum
//                        of v_i^2 from max(j, k)), Cholesky-factored and solved there.
//   sim_step_kernel      one candidate per thread: 40 sequential tracker + bicycle steps, 11 states written per step.
#include <cmath>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int SM = 40;        // displacements / steps / profile length
constexpr int ST = SM + 1;    // states per candidate
constexpr int SLD = SM + 1;   // LDS row stride of a 40 x 40 matrix (doubles): lanes reading a column hit distinct banks
constexpr int NS = 11;        // StateIndex size
constexpr int FIT_WAVES = 4;  // candidates per sim_fit_kernel workgroup

struct SimDev {
  dd_sim_params p;
  double dt2;   // dt * dt
  double dtc;   // the bicycle model's step: int(dt * 1e6) microseconds read back as time_us * 1e-6
};

// In-place Cholesky (lower) of the 40 x 40 matrix G (row stride SLD, lower triangle read and written) by lanes 0..39
// of a wavefront; every wavefront of the workgroup calls it together (uniform barriers).
// Left-looking, a column per step: lane i owns row i and forms L[i][k] = (G[i][k] - sum_{j<k} L[i][j] L[k][j]) / L[k][k]
// in a register from its own row (conflict-free at stride SLD) and row k (one address, broadcast), so the inner loop
// only reads LDS and one barrier per column orders lane k's row before the others read it.
__device__ inline void chol_lds(double* G, int lane) {
  const bool row = lane < SM;
  double* mine = G + (row ? lane : 0) * SLD;
  __syncthreads();
  for (int k = 0; k < SM; ++k) {
    const double* rk = G + k * SLD;
    double s = 0.0;
    if (row && lane >= k) {
      s = mine[k];
      for (int j = 0; j < k; ++j) s -= mine[j] * rk[j];
    }
    const double d = sqrt(__shfl(s, k));
    if (lane == k) mine[k] = d;
    else if (row && lane > k) mine[k] = s / d;
    __syncthreads();
  }
}

// Solve (L L^T) x = b with L from chol_lds: lane j passes b_j and receives x_j. Reads G only.
__device__ inline double chol_solve(const double* G, double b, int lane) {
  double y = b;
  for (int k = 0; k < SM; ++k) {
    const double yk = __shfl(y, k) / G[k * SLD + k];
    if (lane == k) y = yk;
    else if (lane > k && lane < SM) y -= G[lane * SLD + k] * yk;
  }
  for (int k = SM - 1; k >= 0; --k) {
    const double xk = __shfl(y, k) / G[k * SLD + k];
    if (lane == k) y = xk;
    else if (lane < k) y -= G[k * SLD + lane] * xk;
  }
  return y;
}

__global__ __launch_bounds__(64) void sim_factor_kernel(double* fact, double dt, double jerk_penalty) {
  __shared__ double G[SM * SLD];
  const int lane = threadIdx.x;
  if (lane < SM) {
    const double dt2 = dt * dt;
    for (int j = 0; j <= lane; ++j) {
      // L^T L [lane][j], lane >= j: (40 - lane) rows i >= lane, each L[i][lane] * L[i][j]
      const double a = lane == 0 ? dt : dt2, b = j == 0 ? dt : dt2;
      double g = (double)(SM - lane) * (a * b);
      if (lane == j && lane >= 1) g += jerk_penalty;
      if (lane == SM - 1 && j == SM - 2) g -= jerk_penalty;
      G[lane * SLD + j] = g;
    }
  }
  chol_lds(G, lane);
  if (lane < SM)
    for (int j = 0; j < SLD; ++j) fact[lane * SLD + j] = j <= lane ? G[lane * SLD + j] : 0.0;
}

// np.unwrap's correction of one heading step d (period 2 pi).
__device__ inline double unwrap_correction(double d) {
  const double two_pi = 2.0 * M_PI;
  double m = fmod(d + M_PI, two_pi);
  if (m != 0.0 && m < 0.0) m += two_pi;
  m -= M_PI;
  if (m == -M_PI && d > 0.0) m = M_PI;
  return fabs(d) < M_PI ? 0.0 : m - d;
}

__global__ __launch_bounds__(64) void sim_knots_kernel(const float* __restrict__ traj, const double* __restrict__ ego,
                                                       double* __restrict__ prop, int N, int per_group) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const double* e = ego + (size_t)(n / per_group) * NS;
  const float* t = traj + (size_t)n * 8 * 3;
  const double x0 = e[0], y0 = e[1], h0 = e[2];
  const double c = cos(h0), s = sin(h0);
  double* o = prop + (size_t)n * ST * 3;
  double ax = x0, ay = y0, ah = h0;  // knot k (heading unwrapped)
  double raw = h0, corr = 0.0;       // knot k's heading before unwrapping, the corrections summed so far
  for (int k = 0; k < 8; ++k) {
    const double px = (double)t[k * 3], py = (double)t[k * 3 + 1], ph = (double)t[k * 3 + 2];
    const double bx = x0 + c * px - s * py;
    const double by = y0 + s * px + c * py;
    const double braw = h0 + ph;
    corr += unwrap_correction(braw - raw);
    const double bh = braw + corr;
    for (int j = 0; j < 5; ++j) {
      const double w = (double)j / 5.0;
      double* q = o + (size_t)(k * 5 + j) * 3;
      q[0] = ax + (bx - ax) * w;
      q[1] = ay + (by - ay) * w;
      q[2] = ah + (bh - ah) * w;
    }
    ax = bx, ay = by, ah = bh, raw = braw;
  }
  o[SM * 3] = ax, o[SM * 3 + 1] = ay, o[SM * 3 + 2] = ah;
}

// initial + [0, cumsum(deriv * dt)] (batch_lqr_utils.py:20-36): lane k's entry, the steps summed in cumsum's order.
__device__ inline double profile_entry(const double* step, double initial, int lane) {
  double c = 0.0;
  for (int m = 1; m < SM; ++m)
    if (m <= lane) c += step[m];
  return initial + c;
}

__global__ __launch_bounds__(64 * FIT_WAVES) void sim_fit_kernel(const double* __restrict__ prop,
                                                                 const double* __restrict__ fact,
                                                                 double* __restrict__ prof, int N, SimDev sd) {
  __shared__ double sG[FIT_WAVES][SM * SLD];
  __shared__ double sV[FIT_WAVES][3][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = blockIdx.x * FIT_WAVES + wave;
  const bool live = slot < N;
  const int n = live ? slot : N - 1;  // a spare wavefront repeats the last candidate (uniform barriers), stores nothing
  double* G = sG[wave];
  double* v0 = sV[wave][0];
  double* v1 = sV[wave][1];
  double* v2 = sV[wave][2];
  const double* P = prop + (size_t)n * ST * 3;
  const double dt = sd.p.dt, dt2 = sd.dt2;
  const bool row = lane < SM;

  for (int i = lane; i < SM * SLD; i += 64) G[i] = fact[i];
  double proj = 0.0, dh = 0.0;
  if (row) {
    const double xa = P[lane * 3], ya = P[lane * 3 + 1], ha = P[lane * 3 + 2];
    const double xb = P[lane * 3 + 3], yb = P[lane * 3 + 4], hb = P[lane * 3 + 5];
    proj = (xb - xa) * cos(ha) + (yb - ya) * sin(ha);
    const double d = hb - ha;
    dh = atan2(sin(d), cos(d));
  }
  v0[lane] = proj;
  __syncthreads();
  // velocity fit: rhs_j = sum_{i >= j} L[i][j] proj_i
  double b = 0.0;
  if (row) {
    const double l = lane == 0 ? dt : dt2;
    for (int i = lane; i < SM; ++i) b += v0[i] * l;
  }
  double x = chol_solve(G, b, lane);
  v1[lane] = x * dt;
  __syncthreads();
  const double vel = row ? profile_entry(v1, __shfl(x, 0), lane) : 0.0;
  __syncthreads();

  // curvature fit: G = A^T A + Q, rhs = A^T dh with A[i][0] = u_i = v_i dt, A[i][j] = w_i = v_i dt^2 (1 <= j <= i)
  const double u = vel * dt, w = vel * dt2;
  v0[lane] = u, v1[lane] = w, v2[lane] = dh;
  __syncthreads();
  double suu = 0.0, suy = 0.0;
  for (int i = 0; i < SM; ++i) {
    suu += v0[i] * v0[i];
    suy += v0[i] * v2[i];
  }
  double sww = 0.0, suw = 0.0, swy = 0.0;
  if (row)
    for (int i = lane; i < SM; ++i) {
      sww += v1[i] * v1[i];
      suw += v0[i] * v1[i];
      swy += v1[i] * v2[i];
    }
  if (row) {
    if (lane == 0) {
      G[0] = suu + sd.p.initial_curvature_penalty;
    } else {
      G[lane * SLD] = suw;
      for (int j = 1; j < lane; ++j) G[lane * SLD + j] = sww;
      G[lane * SLD + lane] = sww + sd.p.curvature_rate_penalty;
    }
  }
  chol_lds(G, lane);
  x = chol_solve(G, lane == 0 ? suy : swy, lane);
  __syncthreads();
  v1[lane] = x * dt;
  __syncthreads();
  const double curv = row ? profile_entry(v1, __shfl(x, 0), lane) : 0.0;
  if (live && row) {
    prof[(size_t)lane * N + n] = vel;
    prof[(size_t)(SM + lane) * N + n] = curv;
  }
}

__device__ inline double wrap_angle(double a) { return atan2(sin(a), cos(a)); }

// nuPlan's principal_value(angle, min_ = -pi): Python's floor-mod.
__device__ inline double principal_value(double a) {
  const double two_pi = 2.0 * M_PI;
  double m = fmod(a + M_PI, two_pi);
  if (m != 0.0 && m < 0.0) m += two_pi;
  return m - M_PI;
}

__global__ __launch_bounds__(64) void sim_step_kernel(const double* __restrict__ prop, const double* __restrict__ ego,
                                                      const double* __restrict__ prof, double* __restrict__ out, int N,
                                                      int per_group, SimDev sd) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const dd_sim_params& p = sd.p;
  const double dt = p.dt, dtc = sd.dtc, wb = p.wheel_base;
  const int H = p.tracking_horizon;
  const double* e = ego + (size_t)(n / per_group) * NS;
  const double* P = prop + (size_t)n * ST * 3;
  const double* vprof = prof + n;                    // entry k at vprof[k * N]
  const double* kprof = prof + (size_t)SM * N + n;
  double* o = out + (size_t)n * ST * NS;
  double sx = e[0], sy = e[1], sh = e[2], sv = e[3], sa = e[5], steer = e[7], yaw = e[9];
  for (int i = 0; i < NS; ++i) o[i] = e[i];

  const double Blon = (double)H * dt;
  const double inv_lon = -1.0 / (Blon * p.q_lon * Blon + p.r_lon);
  for (int it = 0; it < SM; ++it) {
    // ---- tracker (batch_lqr.py:134-200)
    const double rx = P[it * 3], ry = P[it * 3 + 1], rh = P[it * 3 + 2];
    const double xe = sx - rx, ye = sy - ry;
    const double lat = -xe * sin(rh) + ye * cos(rh);
    const double herr = wrap_angle(sh - rh);
    const int ridx = min(it + H, SM - 1);
    const int len = ridx - it;
    const double vref = vprof[(size_t)ridx * N];
    const bool stop = vref <= p.stopping_velocity && sv <= p.stopping_velocity;
    double accel_cmd, rate_cmd = 0.0;
    if (stop) {
      accel_cmd = -p.stopping_gain * (sv - vref);
    } else {
      accel_cmd = inv_lon * Blon * p.q_lon * (sv - vref);
      // H Euler steps of the linearised lateral error dynamics: A, B, g of error_H = A error_0 + B rate + g
      double A[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
      double Bv[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
      const double astep = accel_cmd * dt;
      double csum = 0.0;
      for (int k = 0; k < H; ++k) {
        const double vk = sv + csum;
        csum += astep;
        const double kap = kprof[(size_t)(k < len ? it + k : ridx) * N];
        const double m01 = vk * dt, m12 = vk * dt / wb;
        const double aff = -vk * kap * dt;
        for (int c = 0; c < 3; ++c) {
          A[0][c] = A[0][c] + m01 * A[1][c];
          A[1][c] = A[1][c] + m12 * A[2][c];
        }
        Bv[0] = Bv[0] + m01 * Bv[1];
        Bv[1] = Bv[1] + m12 * Bv[2];
        Bv[2] = Bv[2] + dt;
        g[0] = g[0] + m01 * g[1];
        g[1] = g[1] + m12 * g[2] + aff;
      }
      double err[3];
      for (int r = 0; r < 3; ++r) err[r] = A[r][0] * lat + A[r][1] * herr + A[r][2] * steer + g[r];
      err[1] = wrap_angle(err[1]);
      err[2] = wrap_angle(err[2]);
      const double b0 = Bv[0] * p.q_lat[0], b1 = Bv[1] * p.q_lat[1], b2 = Bv[2] * p.q_lat[2];
      const double inv = -1.0 / (b0 * Bv[0] + b1 * Bv[1] + b2 * Bv[2] + p.r_lat);
      rate_cmd = inv * (b0 * err[0] + b1 * err[1] + b2 * err[2]);
    }
    // ---- bicycle step (batch_kinematic_bicycle.py:76-185). The low-passed steering ANGLE is not written into the
    // propagating state: the heading integrates tan of the old angle, the new angle is clip(old + updated_rate * dt).
    const double ideal_steer = dtc * rate_cmd + steer;
    const double upd_accel = dtc / (dtc + p.accel_time_constant) * (accel_cmd - sa) + sa;
    const double upd_steer = dtc / (dtc + p.steering_time_constant) * (ideal_steer - steer) + steer;
    const double upd_rate = (upd_steer - steer) / dtc;
    const double nx = sx + sv * cos(sh) * dtc;
    const double ny = sy + sv * sin(sh) * dtc;
    const double nh = principal_value(sh + sv * tan(steer) / wb * dtc);
    const double nv = sv + upd_accel * dtc;
    const double nsteer = fmin(fmax(steer + upd_rate * dtc, -p.max_steering_angle), p.max_steering_angle);
    const double nyaw = nv * tan(nsteer) / wb;
    const double nyacc = (nyaw - yaw) / dtc;
    sx = nx, sy = ny, sh = nh, sv = nv, sa = upd_accel, steer = nsteer, yaw = nyaw;
    double* q = o + (size_t)(it + 1) * NS;
    q[0] = sx, q[1] = sy, q[2] = sh, q[3] = sv, q[4] = 0.0, q[5] = sa, q[6] = 0.0, q[7] = steer, q[8] = upd_rate;
    q[9] = yaw, q[10] = nyacc;
  }
}

}  // namespace

size_t simulate_work_doubles(int N) {
  // the factor, the two profiles (40 x N each) and dd_simulate's proposals
  return (size_t)SM * SLD + (size_t)N * (2 * SM + ST * 3);
}

void launch_simulate(const float* traj, const double* proposals, const double* ego_states, int N, int per_group,
                     const dd_sim_params& p, double* work, double* out_states, hipStream_t st) {
  SimDev sd;
  sd.p = p;
  sd.dt2 = p.dt * p.dt;
  sd.dtc = (double)(long long)(p.dt * 1e6) * 1e-6;
  double* fact = work;
  double* prof = work + (size_t)SM * SLD;
  double* built = prof + (size_t)N * 2 * SM;
  const unsigned per_thread_blocks = (unsigned)((N + 63) / 64);
  hipLaunchKernelGGL(sim_factor_kernel, dim3(1), dim3(64), 0, st, fact, p.dt, p.jerk_penalty);
  DD_HIP_CHECK(hipGetLastError());
  if (traj) {
    hipLaunchKernelGGL(sim_knots_kernel, dim3(per_thread_blocks), dim3(64), 0, st, traj, ego_states, built, N,
                       per_group);
    DD_HIP_CHECK(hipGetLastError());
    proposals = built;
  }
  hipLaunchKernelGGL(sim_fit_kernel, dim3((unsigned)((N + FIT_WAVES - 1) / FIT_WAVES)), dim3(64 * FIT_WAVES), 0, st,
                     proposals, fact, prof, N, sd);
  DD_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sim_step_kernel, dim3(per_thread_blocks), dim3(64), 0, st, proposals, ego_states, prof,
                     out_states, N, per_group, sd);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
