// PDM's forecasted observation from raw detections on the device (dd_observe, include/ddmi.h): PDMObservation.update
// (pdm_planner/observation/pdm_observation.py:105-205) with PDMObjectManager (observation/pdm_object_manager.py), and
// the detections of the planner's own agent head (dd_detections_from_agents). float64 throughout; built with
// -ffp-contract=off (the corner lever arms, the squared distance and the forecast's delta_t * dxy are separate products
// and sums in the reference). Deterministic: no atomics. Two launches.
//
// select_kernel, one workgroup per scene. The reference sorts each class by distance to the ego center and keeps the
// first `cap`; here a row's place is the number of rows of its class that come before it (a smaller distance, or the
// same distance and a lower index), counted against LDS chunks of CHUNK rows, so a scene of any size works with a fixed
// 3.1 KB of LDS and nothing is sorted. The class totals are counted first, so a kept row's slot (the kept static
// objects, vehicles, pedestrians, bicycles, in that order) is known as soon as its place is, and the row that holds
// place cap - 1 leaves its key behind as the class's threshold. A second walk, in detection order, gives every row that
// was not kept its slot behind them through a running count. Every slot's t = 0 box, displacement per second and
// validity go to the scratch; the kept rows are tested against the ego quad there (collisions.hip's closed
// separating-axis test on differences against the ego quad's first corner).
//
// forecast_kernel, one thread per corner of the (K, T_obs, 4, 2) output: 16 bytes per lane, a wavefront writes eight
// whole 128-byte lines; the 11 scratch doubles of a slot are read by its 4 T_obs threads out of the cache.
#include <cmath>
#include <cstdlib>
#include <limits>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int ONS = 11;      // StateIndex size
constexpr int DET = 7;       // x, y, heading, length, width, vx, vy
constexpr int CHUNK = 256;   // rows ranked against at a time: one per thread
constexpr int OWAVES = CHUNK / 64;
constexpr int SLOT = 11;     // scratch doubles per slot: 8 corners, dxy, valid
constexpr int NCLS = 4;      // DD_DET_VEHICLE, PEDESTRIAN, BICYCLE, STATIC

struct ObsConsts {
  double half_length, half_width, rear_axle_to_center;
  double radius, stopped_speed;
  int cap[NCLS];   // by type
};

// true where the four points of a and the four of b are separated along (nx, ny)
__device__ inline bool separated_on(double nx, double ny, const double* ax, const double* ay, const double* bx,
                                    const double* by) {
  double a0 = nx * ax[0] + ny * ay[0], a1 = a0, b0 = nx * bx[0] + ny * by[0], b1 = b0;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const double v = nx * ax[i] + ny * ay[i], w = nx * bx[i] + ny * by[i];
    a0 = fmin(a0, v), a1 = fmax(a1, v), b0 = fmin(b0, w), b1 = fmax(b1, w);
  }
  return a1 < b0 || b1 < a0;
}

// collisions.hip's convex_touch<4>: the closed intersection of the convex quads q and t, every coordinate taken
// relative to q's first corner before any product. Non-finite anywhere: false.
__device__ inline bool quads_touch(const double* qx, const double* qy, const double* tx, const double* ty) {
  double ax[4], ay[4], bx[4], by[4];
  double fin = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ax[i] = qx[i] - qx[0], ay[i] = qy[i] - qy[0];
    bx[i] = tx[i] - qx[0], by[i] = ty[i] - qy[0];
    fin += ((qx[i] - qx[i]) + (qy[i] - qy[i])) + ((tx[i] - tx[i]) + (ty[i] - ty[i]));
  }
  if (fin != fin) return false;
  bool sep = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int f = (e + 1) & 3;
    sep |= separated_on(-(ay[f] - ay[e]), ax[f] - ax[e], ax, ay, bx, by);
    sep |= separated_on(-(by[f] - by[e]), bx[f] - bx[e], ax, ay, bx, by);
  }
  return !sep;
}

// the four corners of a box of half sizes (hl, hw) at center (cx, cy), heading h, as dd_ego_areas forms them
__device__ inline void box_corners(double cx, double cy, double h, double hl, double hw, double* px, double* py) {
  const double half_pi = M_PI / 2.0;
  const double ch = cos(h), sh = sin(h), cq = cos(h + half_pi), sq = sin(h + half_pi);
  const double lon[4] = {hl, -hl, -hl, hl};
  const double lat[4] = {hw, hw, -hw, -hw};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    px[c] = cx + ((lat[c] * cq) + (lon[c] * ch));
    py[c] = cy + ((lat[c] * sq) + (lon[c] * sh));
  }
}

__device__ inline double normalize_angle(double a) { return atan2(sin(a), cos(a)); }

// the class of row d (0..3, -1 where the row is dropped before the selection) and its distance to the ego center
__device__ inline int classify(const double* __restrict__ boxes, const uint8_t* __restrict__ type,
                               const uint8_t* __restrict__ collided_in, int d, double ex, double ey, double radius,
                               double& dist) {
  const int ty = type[d];
  const double dx = boxes[(size_t)d * DET] - ex, dy = boxes[(size_t)d * DET + 1] - ey;
  dist = sqrt((dx * dx) + (dy * dy));
  if (ty >= NCLS || dist != dist) return -1;   // a NaN distance (a NaN ego pose) has no place in any order
  if (collided_in && collided_in[d]) return -1;
  if (radius != 0.0 && hypot(dx, dy) > radius) return -1;
  return ty;
}

// slot k takes row d: the track's own figures, and into the scratch its t = 0 box, displacement per second and validity
__device__ inline void emit(const double* __restrict__ boxes, const uint8_t* __restrict__ type,
                            const uint8_t* __restrict__ collided_in, int d, int k, bool kept, const double* qx,
                            const double* qy, const ObsConsts& c, double* __restrict__ work,
                            double* __restrict__ out_heading, double* __restrict__ out_speed,
                            uint8_t* __restrict__ out_flags, int32_t* __restrict__ out_order,
                            uint8_t* __restrict__ out_collided) {
  const double* b = boxes + (size_t)d * DET;
  const double h = b[2], vx = b[5], vy = b[6];
  const bool agent = type[d] < DD_DET_STATIC;
  const double speed = agent ? hypot(vx, vy) : 0.0;
  out_heading[k] = h;
  out_speed[k] = speed;
  out_flags[k] = (uint8_t)(((!agent || speed <= c.stopped_speed) ? 1 : 0) | (agent ? 2 : 0));
  out_order[k] = d;
  double* w = work + (size_t)k * SLOT;
  bool valid = false, hit = false;
  if (kept) {
    double px[4], py[4], dx = 0.0, dy = 0.0;
    box_corners(b[0], b[1], h, b[3] / 2.0, b[4] / 2.0, px, py);
    if (agent) {
      const double velocity_angle = atan2(vy, vx);
      const bool forward = fabs(normalize_angle(h - velocity_angle)) < M_PI / 2.0;
      const double track_heading = forward ? h : normalize_angle(h + M_PI);
      dx = cos(track_heading) * speed, dy = sin(track_heading) * speed;
    }
    hit = quads_touch(qx, qy, px, py);
    valid = !hit;
    if (valid) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w[2 * i] = px[i], w[2 * i + 1] = py[i];
      w[8] = dx, w[9] = dy, w[10] = 1.0;
    }
  }
  if (!valid) {
#pragma unroll
    for (int i = 0; i < SLOT; ++i) w[i] = 0.0;
  }
  out_collided[d] = (uint8_t)((hit || (collided_in && collided_in[d])) ? 1 : 0);
}

__global__ __launch_bounds__(CHUNK) void select_kernel(const double* __restrict__ boxes, const uint8_t* __restrict__ type,
                                                       const int32_t* __restrict__ scene_det_off,
                                                       const uint8_t* __restrict__ collided_in,
                                                       const double* __restrict__ ego, ObsConsts c,
                                                       double* __restrict__ work, double* __restrict__ out_heading,
                                                       double* __restrict__ out_speed, uint8_t* __restrict__ out_flags,
                                                       int32_t* __restrict__ out_order,
                                                       uint8_t* __restrict__ out_collided) {
  __shared__ double s_dist[CHUNK];
  __shared__ int s_cls[CHUNK];
  __shared__ int s_wave[OWAVES][NCLS];
  __shared__ double s_thr_dist[NCLS];
  __shared__ int s_thr_idx[NCLS];

  const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int begin = scene_det_off[g], n = scene_det_off[g + 1] - begin;   // the same in every thread
  if (n <= 0) return;
  const double* E = ego + (size_t)g * ONS;
  const double eh = E[2];
  const double ex = E[0] + c.rear_axle_to_center * cos(eh), ey = E[1] + c.rear_axle_to_center * sin(eh);
  double qx[4], qy[4];
  box_corners(ex, ey, eh, c.half_length, c.half_width, qx, qy);

  // the class totals
  int mine[NCLS] = {0, 0, 0, 0};
  for (int i = tid; i < n; i += CHUNK) {
    double dist;
    const int cls = classify(boxes, type, collided_in, begin + i, ex, ey, c.radius, dist);
#pragma unroll
    for (int q = 0; q < NCLS; ++q) mine[q] += cls == q;
  }
#pragma unroll
  for (int q = 0; q < NCLS; ++q) {
    for (int m = 1; m < 64; m <<= 1) mine[q] += __shfl_xor(mine[q], m);
    if (lane == 0) s_wave[wave][q] = mine[q];
  }
  if (tid < NCLS) s_thr_idx[tid] = -1, s_thr_dist[tid] = 0.0;
  __syncthreads();
  int total[NCLS], kept_n[NCLS], base[NCLS];
#pragma unroll
  for (int q = 0; q < NCLS; ++q) {
    total[q] = 0;
    for (int w = 0; w < OWAVES; ++w) total[q] += s_wave[w][q];
    kept_n[q] = total[q] < c.cap[q] ? total[q] : c.cap[q];
  }
  base[DD_DET_STATIC] = 0;
  base[DD_DET_VEHICLE] = kept_n[DD_DET_STATIC];
  base[DD_DET_PEDESTRIAN] = base[DD_DET_VEHICLE] + kept_n[DD_DET_VEHICLE];
  base[DD_DET_BICYCLE] = base[DD_DET_PEDESTRIAN] + kept_n[DD_DET_PEDESTRIAN];
  const int kept_all = base[DD_DET_BICYCLE] + kept_n[DD_DET_BICYCLE];

  // the place of every row within its class; a kept row takes its slot at once
  for (int ib = 0; ib < n; ib += CHUNK) {
    const int i = ib + tid;
    double dist_i = 0.0;
    const int cls_i = i < n ? classify(boxes, type, collided_in, begin + i, ex, ey, c.radius, dist_i) : -1;
    int place = 0;
    for (int jb = 0; jb < n; jb += CHUNK) {
      __syncthreads();   // the chunk before has been read
      const int j = jb + tid;
      double dist_j = 0.0;
      s_cls[tid] = j < n ? classify(boxes, type, collided_in, begin + j, ex, ey, c.radius, dist_j) : -1;
      s_dist[tid] = dist_j;
      __syncthreads();
      const int m = n - jb < CHUNK ? n - jb : CHUNK;
      if (cls_i >= 0)
        for (int q = 0; q < m; ++q) {
          const double dj = s_dist[q];
          place += (s_cls[q] == cls_i) && (dj < dist_i || (dj == dist_i && jb + q < i));
        }
    }
    if (cls_i >= 0) {
      const int cap = c.cap[cls_i];
      if (place < cap)
        emit(boxes, type, collided_in, begin + i, begin + base[cls_i] + place, true, qx, qy, c, work, out_heading,
             out_speed, out_flags, out_order, out_collided);
      if (place == cap - 1) s_thr_dist[cls_i] = dist_i, s_thr_idx[cls_i] = i;   // one row per class at the most
    }
  }
  __syncthreads();

  // every other row, in detection order, behind the kept ones
  int run = 0;   // the same in every thread
  for (int ib = 0; ib < n; ib += CHUNK) {
    const int i = ib + tid;
    bool dropped = false;
    if (i < n) {
      double dist_i;
      const int cls_i = classify(boxes, type, collided_in, begin + i, ex, ey, c.radius, dist_i);
      bool kept = false;
      if (cls_i >= 0) {
        const int ti = s_thr_idx[cls_i];   // -1: the class has fewer rows than its cap (all kept), or a cap of 0
        if (ti < 0)
          kept = c.cap[cls_i] > 0;
        else
          kept = dist_i < s_thr_dist[cls_i] || (dist_i == s_thr_dist[cls_i] && i <= ti);
      }
      dropped = !kept;
    }
    const unsigned long long bal = __ballot(dropped);
    if (lane == 0) s_wave[wave][0] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < OWAVES; ++w) {
      const int cnt = s_wave[w][0];
      before += w < wave ? cnt : 0;
      all += cnt;
    }
    if (dropped) {
      const int slot = kept_all + run + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (slot < n)   // always: the two walks agree on who is kept; the scene's slots are never left whatever the input
        emit(boxes, type, collided_in, begin + i, begin + slot, false, qx, qy, c, work, out_heading, out_speed,
             out_flags, out_order, out_collided);
    }
    run += all;
    __syncthreads();   // s_wave is written again
  }
}

// boxes[k, t, corner] = corner + (double(res (t / res)) dt) dxy where slot k is valid, else 0; one corner per thread
__global__ __launch_bounds__(256) void forecast_kernel(const double* __restrict__ work, long long corners, int T_obs,
                                                       int res, double dt, double2* __restrict__ out_boxes,
                                                       uint8_t* __restrict__ out_valid) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= corners) return;
  const long long kt = idx >> 2;   // k T_obs + t
  const int corner = (int)(idx & 3);
  const long long k = kt / T_obs;
  const int t = (int)(kt - k * T_obs);
  const double* w = work + k * SLOT;
  const bool valid = w[10] != 0.0;
  double2 v = make_double2(0.0, 0.0);
  if (valid) {
    const double delta = (double)(res * (t / res)) * dt;
    v.x = w[2 * corner] + delta * w[8];
    v.y = w[2 * corner + 1] + delta * w[9];
  }
  out_boxes[idx] = v;
  if (corner == 0) out_valid[kt] = valid ? 1 : 0;
}

__global__ __launch_bounds__(256) void agents_kernel(const float* __restrict__ states, const float* __restrict__ labels,
                                                     const double* __restrict__ ego, int B, int A, float threshold,
                                                     double* __restrict__ out_boxes, uint8_t* __restrict__ out_type,
                                                     int32_t* __restrict__ out_off) {
  const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
  if (d <= B) out_off[d] = (int32_t)(d * A);
  if (d >= (long long)B * A) return;
  const int b = (int)(d / A);
  const float* s = states + d * 5;
  const double x = s[0], y = s[1], h = s[2], length = s[3], width = s[4], logit = labels[d];
  const double* E = ego + (size_t)b * ONS;
  const double x0 = E[0], y0 = E[1], h0 = E[2];
  const double c0 = cos(h0), s0 = sin(h0);
  const double cx = x0 + ((c0 * x) - (s0 * y)), cy = y0 + ((s0 * x) + (c0 * y)), heading = h0 + h;
  const double fin = (((x - x) + (y - y)) + ((h - h) + (length - length))) + ((width - width) + (logit - logit));
  // a pose that is not finite makes the row's own values non-finite: it is passed over like a non-finite box
  const bool ok = fin == 0.0 && (cx - cx) + (cy - cy) + (heading - heading) == 0.0 && logit > (double)threshold &&
                  length > 0.0 && width > 0.0;
  double* o = out_boxes + d * DET;
  o[0] = ok ? cx : 0.0, o[1] = ok ? cy : 0.0, o[2] = ok ? heading : 0.0;
  o[3] = ok ? length : 0.0, o[4] = ok ? width : 0.0, o[5] = 0.0, o[6] = 0.0;
  out_type[d] = ok ? DD_DET_VEHICLE : DD_DET_SKIP;
}

}  // namespace

size_t observe_work_doubles(int D) { return (size_t)SLOT * (size_t)(D > 0 ? D : 1); }

void launch_observe(const dd_detections& det, const double* ego_states, int G, const dd_observe_params& p,
                    const dd_area_params& ap, double* work, double* out_boxes, uint8_t* out_valid, double* out_heading,
                    double* out_speed, uint8_t* out_flags, int32_t* out_order, uint8_t* out_collided, hipStream_t st) {
  const int D = det.num_dets;
  if (D <= 0) return;
  ObsConsts c;
  c.half_length = ap.half_length, c.half_width = ap.half_width, c.rear_axle_to_center = ap.rear_axle_to_center;
  c.radius = p.map_radius, c.stopped_speed = p.stopped_speed;
  c.cap[DD_DET_VEHICLE] = p.max_vehicles, c.cap[DD_DET_PEDESTRIAN] = p.max_pedestrians;
  c.cap[DD_DET_BICYCLE] = p.max_bicycles, c.cap[DD_DET_STATIC] = p.max_static;
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)G), dim3(CHUNK), 0, st, det.boxes, det.type, det.scene_det_off,
                     det.collided_in, ego_states, c, work, out_heading, out_speed, out_flags, out_order, out_collided);
  DD_HIP_CHECK(hipGetLastError());
  const int T_obs = p.num_samples + p.sample_res;
  const long long corners = (long long)D * T_obs * 4;   // below 2^30: the caller checked
  hipLaunchKernelGGL(forecast_kernel, dim3((unsigned)((corners + 255) / 256)), dim3(256), 0, st, work, corners, T_obs,
                     p.sample_res, p.dt, reinterpret_cast<double2*>(out_boxes), out_valid);
  DD_HIP_CHECK(hipGetLastError());
}

void launch_detections_from_agents(const float* agent_states, const float* agent_labels, const double* ego_states,
                                   int B, int A, float threshold, double* out_boxes, uint8_t* out_type,
                                   int32_t* out_scene_det_off, hipStream_t st) {
  const long long rows = (long long)B * A;   // >= B + 1 does not hold for A = 1: cover both
  const long long threads = rows > B + 1 ? rows : B + 1;
  hipLaunchKernelGGL(agents_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, agent_states,
                     agent_labels, ego_states, B, A, threshold, out_boxes, out_type, out_scene_det_off);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
