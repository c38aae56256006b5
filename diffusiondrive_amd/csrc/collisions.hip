// PDM no-at-fault collision and time-to-collision on the device (dd_collisions, include/ddmi.h):
// PDMScorer._calculate_no_at_fault_collision (pdm_planner/scoring/pdm_scorer.py:293-349) with get_collision_type
// (scoring/pdm_scorer_utils.py:13-65), and _calculate_ttc (:414-498), over the (N, 41, 11) float64 states dd_simulate
// writes and the (N, 41, 3) flags dd_ego_areas writes, both read in place. float64 throughout; built with
// -ffp-contract=off (the corner lever arms and the TTC shift are separate products and sums in the reference, and the
// containment rule is ego_areas.hip's). Deterministic: no atomics. Two launches: every track's bounding box over its
// valid times into the scratch, then the scoring.
//
// The reference walks t = 0..40 and keeps, per candidate, a list of tokens that no longer count. A token joins the
// list at its first not-at-fault hit and an at-fault hit only lowers a min, so per (candidate, track) the FIRST
// intersection alone decides, and the pairs are independent: the walk over t is a first-set-bit search over a ballot.
// Layout: one candidate per wavefront, lane t owns state t - its four corners, its speed, its three shifted TTC quads
// (the k = 0 quad is the ego quad itself wherever the shift is finite: corner + d * 0.0 = corner) - and the four
// wavefronts of a workgroup share a scene, so that the tracks they read sit in the same cache lines. No LDS and no
// barrier: a wavefront takes the scene's tracks 64 at a time (TRACK_CHUNK), lane j holding track j's box against the
// candidate's, and walks the survivors' bits. Per track and look-ahead step the lanes first hold their quad's box
// against the track's box at that time and skip the separating-axis test where no lane's overlaps; both culls widen
// the ego side by CULL_SLACK, many orders above the rounding of the test they stand in front of, so they never remove
// an intersection the test would find, and DDMI_COLLISIONS_CULL=0 turns both off with the same results.
//
// Intersection is a separating-axis test of two convex quads, closed (touching counts), formed from differences
// against the ego quad's first corner only: the boxes sit at 6.6e5 / 4.0e6 m, where a product of absolute
// coordinates is good to 1e-3 m^2. A quad with a non-finite corner intersects nothing.
#include <cmath>
#include <cstdlib>
#include <limits>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int CT = 41;            // states per candidate
constexpr int CNS = 11;           // StateIndex size
constexpr int CWAVES = 4;         // candidates per workgroup
constexpr int TRACK_CHUNK = 64;   // tracks culled at a time: one per lane
constexpr int TTC_STEPS = 4;      // look-ahead steps 0, 3, 6, 9
constexpr int TTC_STRIDE = 3;
constexpr double CULL_SLACK = 0x1p-10;   // metres; the tests' rounding is below 1e-8 m at 4e6 m

// every track's closed bounding box over the times it is valid at: one wavefront per track
__global__ __launch_bounds__(64 * CWAVES) void track_boxes_kernel(const double* __restrict__ boxes,
                                                                  const uint8_t* __restrict__ valid, int K, int T_obs,
                                                                  double* __restrict__ out) {
  const int j = blockIdx.x * CWAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= K) return;
  const double inf = std::numeric_limits<double>::infinity();
  double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
  for (int t = lane; t < T_obs; t += 64) {
    if (!valid[(size_t)j * T_obs + t]) continue;
    const double* b = boxes + ((size_t)j * T_obs + t) * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      x0 = fmin(x0, b[2 * c]), y0 = fmin(y0, b[2 * c + 1]), x1 = fmax(x1, b[2 * c]), y1 = fmax(y1, b[2 * c + 1]);
  }
  for (int m = 1; m < 64; m <<= 1) {
    x0 = fmin(x0, __shfl_xor(x0, m)), y0 = fmin(y0, __shfl_xor(y0, m));
    x1 = fmax(x1, __shfl_xor(x1, m)), y1 = fmax(y1, __shfl_xor(y1, m));
  }
  if (lane == 0) {
    double* o = out + 4 * (size_t)j;
    o[0] = x0, o[1] = y0, o[2] = x1, o[3] = y1;
  }
}

// true where the NA points of a (relative to the origin o) and the four of b are separated along (nx, ny)
template <int NA>
__device__ inline bool separated_on(double nx, double ny, const double* ax, const double* ay, const double* bx,
                                    const double* by) {
  double a0 = nx * ax[0] + ny * ay[0], a1 = a0;
#pragma unroll
  for (int i = 1; i < NA; ++i) {
    const double v = nx * ax[i] + ny * ay[i];
    a0 = fmin(a0, v), a1 = fmax(a1, v);
  }
  double b0 = nx * bx[0] + ny * by[0], b1 = b0;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const double v = nx * bx[i] + ny * by[i];
    b0 = fmin(b0, v), b1 = fmax(b1, v);
  }
  return a1 < b0 || b1 < a0;
}

// closed intersection of the convex polygon a (NA = 4: a quad; NA = 2: a segment) with the convex quad b; every
// coordinate is taken relative to a's first point before any product. Non-finite anywhere: false.
template <int NA>
__device__ inline bool convex_touch(const double* qx, const double* qy, const double* tx, const double* ty) {
  double ax[NA], ay[NA], bx[4], by[4];
  double fin = 0.0;   // NaN as soon as a coordinate is NaN or infinite
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    ax[i] = qx[i] - qx[0], ay[i] = qy[i] - qy[0];
    fin += (qx[i] - qx[i]) + (qy[i] - qy[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bx[i] = tx[i] - qx[0], by[i] = ty[i] - qy[0];
    fin += (tx[i] - tx[i]) + (ty[i] - ty[i]);
  }
  if (fin != fin) return false;
  bool sep = false;
  constexpr int EA = NA == 2 ? 1 : NA;   // a segment has one edge direction
#pragma unroll
  for (int e = 0; e < EA; ++e) {
    const int f = (e + 1) % NA;
    sep |= separated_on<NA>(-(ay[f] - ay[e]), ax[f] - ax[e], ax, ay, bx, by);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int f = (e + 1) & 3;
    sep |= separated_on<NA>(-(by[f] - by[e]), bx[f] - bx[e], ax, ay, bx, by);
  }
  return !sep;
}

// the area centroid of quad b relative to its first corner (the corner mean for a zero-area quad)
__device__ inline void quad_centroid_rel(const double* bx, const double* by, double& cx, double& cy) {
  const double ux = bx[1] - bx[0], uy = by[1] - by[0], vx = bx[2] - bx[0], vy = by[2] - by[0];
  const double wx = bx[3] - bx[0], wy = by[3] - by[0];
  const double a1 = ux * vy - vx * uy, a2 = vx * wy - wx * vy;   // twice the signed areas of (0,1,2) and (0,2,3)
  const double a = a1 + a2;
  if (a == 0.0) {
    cx = ((ux + vx) + wx) / 4.0, cy = ((uy + vy) + wy) / 4.0;
    return;
  }
  cx = (a1 * (ux + vx) + a2 * (vx + wx)) / (3.0 * a);
  cy = (a1 * (uy + vy) + a2 * (vy + wy)) / (3.0 * a);
}

// nuPlan's get_agent_relative_angle: arccos(dot((cos h, sin h), v / |v|)), v from the rear axle to the centroid
__device__ inline double relative_angle(double ch, double sh, double x, double y, const double* bx, const double* by) {
  double cx, cy;
  quad_centroid_rel(bx, by, cx, cy);
  const double vx = (bx[0] - x) + cx, vy = (by[0] - y) + cy;
  const double norm = sqrt(vx * vx + vy * vy);
  return acos(ch * (vx / norm) + sh * (vy / norm));
}

// (x, y) strictly inside any polygon of the scene: ego_areas.hip's rule (an even-odd crossing count over differences;
// a point on an edge is outside), walked by one lane
__device__ bool in_any_polygon(double x, double y, const double* __restrict__ verts,
                               const int32_t* __restrict__ ring_off, const int32_t* __restrict__ poly_ring_off,
                               int p_begin, int p_end) {
  for (int p = p_begin; p < p_end; ++p) {
    bool parity = false, on_edge = false;
    for (int r = poly_ring_off[p]; r < poly_ring_off[p + 1]; ++r) {
      const int v0 = ring_off[r], nv = ring_off[r + 1] - v0;
      double a = verts[2 * (size_t)v0], b = verts[2 * (size_t)v0 + 1];
      for (int e = 0; e < nv; ++e) {
        const int w = e + 1 == nv ? 0 : e + 1;
        const double c = verts[2 * (size_t)(v0 + w)], d = verts[2 * (size_t)(v0 + w) + 1];
        const double dx = c - a, dy = d - b;
        const double cross = dx * (y - b) - (x - a) * dy;
        if ((b > y) != (d > y) && (dy > 0.0 ? cross > 0.0 : cross < 0.0)) parity = !parity;
        if (cross == 0.0 && x >= fmin(a, c) && x <= fmax(a, c) && y >= fmin(b, d) && y <= fmax(b, d)) on_edge = true;
        a = c, b = d;
      }
    }
    if (parity && !on_edge) return true;
  }
  return false;
}

struct ColConsts {
  double half_length, half_width, rear_axle_to_center, dt;
  double ttc_speed, col_speed, ahead, behind;
  int cull;
};

__global__ __launch_bounds__(64 * CWAVES) void collisions_kernel(
    const double* __restrict__ states, const uint8_t* __restrict__ areas, int per_group, int blocks_per_group,
    const double* __restrict__ boxes, const uint8_t* __restrict__ valid, const double* __restrict__ heading,
    const uint8_t* __restrict__ flags, const int32_t* __restrict__ scene_track_off, int T_obs,
    const double* __restrict__ track_box, const double* __restrict__ ix_verts, const int32_t* __restrict__ ix_ring_off,
    const int32_t* __restrict__ ix_poly_ring_off, const int32_t* __restrict__ ix_scene_poly_off, ColConsts k,
    double* __restrict__ out_no_collision, double* __restrict__ out_collision_idx, double* __restrict__ out_ttc,
    double* __restrict__ out_ttc_idx) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x / blocks_per_group;
  const int slot = (blockIdx.x - g * blocks_per_group) * CWAVES + wave;
  if (slot >= per_group) return;   // the kernel has no barrier: a spare wavefront leaves
  const size_t n = (size_t)g * per_group + slot;
  const bool row = lane < CT;
  const int t = row ? lane : CT - 1;   // a spare lane repeats state 40 and takes no part

  const double* S = states + (n * CT + t) * CNS;
  const double x = S[0], y = S[1], h = S[2];
  const double speed = hypot(S[3], S[4]);
  const double half_pi = M_PI / 2.0;
  const double ch = cos(h), sh = sin(h), cq = cos(h + half_pi), sq = sin(h + half_pi);
  const double cx = x + k.rear_axle_to_center * ch, cy = y + k.rear_axle_to_center * sh;
  const double lon[4] = {k.half_length, -k.half_length, -k.half_length, k.half_length};
  const double lat[4] = {k.half_width, k.half_width, -k.half_width, -k.half_width};
  double px[4], py[4];   // front-left, rear-left, rear-right, front-right, as dd_ego_areas forms them
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    px[c] = cx + ((lat[c] * cq) + (lon[c] * ch));
    py[c] = cy + ((lat[c] * sq) + (lon[c] * sh));
  }
  const double dxs = ch * speed, dys = sh * speed;   // dxy_per_s
  // the shift of look-ahead step q: dxy_per_s * (float(3 q) * dt), the product formed exactly so
  double shx[TTC_STEPS], shy[TTC_STEPS];
#pragma unroll
  for (int q = 0; q < TTC_STEPS; ++q) {
    const double delta = (double)(TTC_STRIDE * q) * k.dt;
    shx[q] = dxs * delta, shy[q] = dys * delta;
  }
  const bool shift0_finite = shx[0] - shx[0] == 0.0 && shy[0] - shy[0] == 0.0;
  const uint8_t* A = areas + (n * CT + t) * 3;
  const bool off_lane = A[0] != 0 || A[1] != 0;   // multiple lanes or non-drivable area at t
  const bool ttc_live = row && !(speed < k.ttc_speed);

  // this lane's quads, step by step, as boxes (widened), and the candidate's box over all of them
  const double inf = std::numeric_limits<double>::infinity();
  double qx0[TTC_STEPS], qy0[TTC_STEPS], qx1[TTC_STEPS], qy1[TTC_STEPS];
  double wx0 = inf, wy0 = inf, wx1 = -inf, wy1 = -inf;
#pragma unroll
  for (int q = 0; q < TTC_STEPS; ++q) {
    double a0 = inf, b0 = inf, a1 = -inf, b1 = -inf;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double vx = q == 0 ? px[c] : px[c] + shx[q], vy = q == 0 ? py[c] : py[c] + shy[q];
      a0 = fmin(a0, vx), b0 = fmin(b0, vy), a1 = fmax(a1, vx), b1 = fmax(b1, vy);
    }
    qx0[q] = a0 - CULL_SLACK, qy0[q] = b0 - CULL_SLACK, qx1[q] = a1 + CULL_SLACK, qy1[q] = b1 + CULL_SLACK;
    wx0 = fmin(wx0, qx0[q]), wy0 = fmin(wy0, qy0[q]), wx1 = fmax(wx1, qx1[q]), wy1 = fmax(wy1, qy1[q]);
  }
  for (int m = 1; m < 64; m <<= 1) {
    wx0 = fmin(wx0, __shfl_xor(wx0, m)), wy0 = fmin(wy0, __shfl_xor(wy0, m));
    wx1 = fmax(wx1, __shfl_xor(wx1, m)), wy1 = fmax(wy1, __shfl_xor(wy1, m));
  }

  double no_collision = 1.0, collision_idx = inf, ttc = 1.0, ttc_idx = inf;   // the same in every lane
  const int k_begin = scene_track_off[g], k_end = scene_track_off[g + 1];
  const int p_begin = ix_scene_poly_off[g], p_end = ix_scene_poly_off[g + 1];
  for (int base = k_begin; base < k_end; base += TRACK_CHUNK) {
    bool keep = false;
    if (base + lane < k_end) {
      const double* b = track_box + 4 * (size_t)(base + lane);
      keep = !k.cull || (wx0 <= b[2] && wx1 >= b[0] && wy0 <= b[3] && wy1 >= b[1]);
    }
    unsigned long long kept = __ballot(keep);
    while (kept) {
      const int j = base + __builtin_ctzll(kept);   // the same in every lane
      kept &= kept - 1ull;
      const double* B = boxes + (size_t)j * T_obs * 8;
      const uint8_t* V = valid + (size_t)j * T_obs;
      bool hit[TTC_STEPS];
#pragma unroll
      for (int q = 0; q < TTC_STEPS; ++q) {
        const int tt = t + TTC_STRIDE * q;   // <= 49 < T_obs
        const bool there = row && V[tt] != 0;
        double bx[4], by[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bx[c] = there ? B[tt * 8 + 2 * c] : 0.0, by[c] = there ? B[tt * 8 + 2 * c + 1] : 0.0;
        const double tx0 = fmin(fmin(bx[0], bx[1]), fmin(bx[2], bx[3])), tx1 = fmax(fmax(bx[0], bx[1]), fmax(bx[2], bx[3]));
        const double ty0 = fmin(fmin(by[0], by[1]), fmin(by[2], by[3])), ty1 = fmax(fmax(by[0], by[1]), fmax(by[2], by[3]));
        const bool near = there && qx0[q] <= tx1 && qx1[q] >= tx0 && qy0[q] <= ty1 && qy1[q] >= ty0;
        hit[q] = false;
        if (k.cull ? __ballot(near) == 0ull : __ballot(there) == 0ull) continue;
        double ex[4], ey[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) ex[c] = q == 0 ? px[c] : px[c] + shx[q], ey[c] = q == 0 ? py[c] : py[c] + shy[q];
        hit[q] = there && convex_touch<4>(ex, ey, bx, by);
      }

      // collision: the first t whose ego quad meets the track's box at t; that lane classifies
      const unsigned long long met = __ballot(hit[0]);
      if (met) {
        const int t0 = __builtin_ctzll(met);
        int fault = 0;   // 0 not at fault, 1 at fault with an agent, 2 at fault with another object
        if (lane == t0) {
          const unsigned fl = flags[j];
          double bx[4], by[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) bx[c] = B[t * 8 + 2 * c], by[c] = B[t * 8 + 2 * c + 1];
          bool at_fault;
          if (speed <= k.col_speed) {
            at_fault = false;                                          // STOPPED_EGO
          } else if (fl & 1u) {
            at_fault = true;                                           // STOPPED_TRACK
          } else if (relative_angle(ch, sh, x, y, bx, by) > k.behind) {
            at_fault = false;                                          // ACTIVE_REAR
          } else {
            const double fx[2] = {px[0], px[3]}, fy[2] = {py[0], py[3]};
            at_fault = convex_touch<2>(fx, fy, bx, by) || off_lane;    // ACTIVE_FRONT, else ACTIVE_LATERAL
          }
          fault = at_fault ? ((fl & 2u) ? 1 : 2) : 0;
        }
        fault = __shfl(fault, t0);
        if (fault) {
          no_collision = fmin(no_collision, fault == 1 ? 0.0 : 0.5);
          collision_idx = fmin(collision_idx, (double)t0);
        }
      }

      // TTC: the first (t, k) with a live speed at t whose shifted quad meets the track's box at t + k
      hit[0] = hit[0] && shift0_finite;
      int mine = -1;
#pragma unroll
      for (int q = TTC_STEPS - 1; q >= 0; --q)
        if (hit[q]) mine = q;
      const unsigned long long close = __ballot(ttc_live && mine >= 0);
      if (close) {
        const int t1 = __builtin_ctzll(close);
        int infraction = 0;
        if (lane == t1) {
          const int tt = t + TTC_STRIDE * mine;
          double bx[4], by[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) bx[c] = B[tt * 8 + 2 * c], by[c] = B[tt * 8 + 2 * c + 1];
          const double angle = relative_angle(ch, sh, x, y, bx, by);
          if (angle < k.ahead)
            infraction = 1;
          else if (!(angle > k.behind))
            infraction = off_lane || in_any_polygon(x, y, ix_verts, ix_ring_off, ix_poly_ring_off, p_begin, p_end);
        }
        infraction = __shfl(infraction, t1);
        if (infraction) {
          ttc = 0.0;
          ttc_idx = fmin(ttc_idx, (double)t1);
        }
      }
    }
  }
  if (lane == 0) {
    out_no_collision[n] = no_collision, out_collision_idx[n] = collision_idx;
    out_ttc[n] = ttc, out_ttc_idx[n] = ttc_idx;
  }
}

}  // namespace

size_t collisions_work_doubles(int K) { return 4 * (size_t)(K > 0 ? K : 1); }

void launch_collisions(const double* states, const uint8_t* areas, int N, int per_group, const dd_observations& obs,
                       const dd_drivable_maps& ix, int G, const dd_area_params& ap, const dd_score_params& sp,
                       double* work, double* out_no_collision, double* out_collision_idx, double* out_ttc,
                       double* out_ttc_idx, hipStream_t st) {
  const int K = obs.num_tracks;
  if (K > 0) {
    hipLaunchKernelGGL(track_boxes_kernel, dim3((unsigned)((K + CWAVES - 1) / CWAVES)), dim3(64 * CWAVES), 0, st,
                       obs.boxes, obs.valid, K, obs.num_times, work);
    DD_HIP_CHECK(hipGetLastError());
  }
  // DDMI_COLLISIONS_CULL=0: every quad tested against every track of the scene (tools/bench_pdm_score.py measures what
  // the boxes save); the results are the same
  const char* env = std::getenv("DDMI_COLLISIONS_CULL");
  ColConsts k;
  k.half_length = ap.half_length, k.half_width = ap.half_width, k.rear_axle_to_center = ap.rear_axle_to_center;
  k.dt = ap.dt;
  k.ttc_speed = sp.ttc_stopped_speed_threshold, k.col_speed = sp.collision_stopped_speed_threshold;
  k.ahead = sp.ahead_angle, k.behind = sp.behind_angle;
  k.cull = !(env && env[0] == '0');
  const int blocks_per_group = (per_group + CWAVES - 1) / CWAVES;
  hipLaunchKernelGGL(collisions_kernel, dim3((unsigned)G * (unsigned)blocks_per_group), dim3(64 * CWAVES), 0, st, states,
                     areas, per_group, blocks_per_group, obs.boxes, obs.valid, obs.heading, obs.flags,
                     obs.scene_track_off, obs.num_times, work, ix.verts, ix.ring_off, ix.poly_ring_off,
                     ix.scene_poly_off, k, out_no_collision, out_collision_idx, out_ttc, out_ttc_idx);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
