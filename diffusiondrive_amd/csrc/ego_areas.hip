// PDM map compliance on the device (dd_ego_areas, include/ddmi.h): PDMScorer._calculate_ego_area
// (pdm_planner/scoring/pdm_scorer.py:240-291) with the five points of state_array_to_coords_array
// (utils/pdm_array_representation.py:142-181), and the two scores taken from it alone: drivable-area compliance
// (:351-358) and driving-direction compliance (:360-396), over the (N, 41, 11) float64 states dd_simulate writes, read
// in place. float64 throughout; built with -ffp-contract=off (the reference's lever arms are separate products and
// sums, and a crossing test that contracts one of its two products is no longer antisymmetric in them).
// Deterministic: no atomics, every sum in a fixed order. Two launches: the polygons' bounding boxes into the scratch,
// then the scoring.
//
// Containment is a crossing count (even-odd over all rings of a polygon, so a hole is outside) over coordinate
// differences only: an edge (a, b) -> (c, d) flips the parity of point (x, y) where (b > y) != (d > y) and
// cross = (c - a)(y - b) - (x - a)(d - b) has the sign of d - b (a NaN has neither: such a point is outside). Map
// coordinates sit at 6.6e5 / 4.0e6 m, where the differences are exact and their products good to 1e-16 relative; a
// product of absolute coordinates would be good to 1e-3 m^2 only. shapely's contains is the interior: a point with
// cross == 0 inside the edge's box lies on the boundary and is outside whatever the parity says.
// Layout: one candidate per wavefront, lane t owns state t and its five points, so every per-state aggregate stays
// in the lane's registers; four wavefronts of the SAME scene per workgroup, which stages each ring's vertices into
// LDS in chunks of RING_CHUNK edges (every lane reads the same edge: a broadcast) and carries the parity across
// chunks. A polygon whose closed bounding box misses the workgroup's points is not staged; a wavefront none of whose
// points lies in the box skips its edge tests (a point outside the box is outside the polygon: the cull is
// conservative, and it is the whole performance story - a vehicle is 5 m long, a map polygon tens of metres); and
// an edge in whose closed y range no point of the wavefront lies is skipped after one product per point.
#include <cmath>
#include <cstdlib>
#include <limits>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int AT = 41;              // states per candidate
constexpr int ANS = 11;             // StateIndex size
constexpr int AWAVES = 4;           // candidates per workgroup
constexpr int NPTS = 5;             // BBCoordsIndex: front-left, rear-left, rear-right, front-right, center
constexpr int RING_CHUNK = 256;     // edges staged at a time (RING_CHUNK + 1 vertices, 4 KB: eight workgroups a CU)
constexpr unsigned KIND_LANE = 1u, KIND_DRIVABLE = 2u, KIND_ROUTE = 4u;

// The closed bounding box of every polygon: one wavefront per polygon, the lanes stride over the vertices of all its
// rings (they follow each other in verts), then a butterfly. The vertices are finite (ddmi.h).
__global__ __launch_bounds__(64 * AWAVES) void area_boxes_kernel(const double* __restrict__ verts,
                                                                 const int32_t* __restrict__ ring_off,
                                                                 const int32_t* __restrict__ poly_ring_off, int P,
                                                                 double* __restrict__ boxes) {
  const int p = blockIdx.x * AWAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const int v0 = ring_off[poly_ring_off[p]], v1 = ring_off[poly_ring_off[p + 1]];
  const double inf = std::numeric_limits<double>::infinity();
  double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
  for (int v = v0 + lane; v < v1; v += 64) {
    const double x = verts[2 * (size_t)v], y = verts[2 * (size_t)v + 1];
    x0 = fmin(x0, x), y0 = fmin(y0, y), x1 = fmax(x1, x), y1 = fmax(y1, y);
  }
  for (int m = 1; m < 64; m <<= 1) {
    x0 = fmin(x0, __shfl_xor(x0, m)), y0 = fmin(y0, __shfl_xor(y0, m));
    x1 = fmax(x1, __shfl_xor(x1, m)), y1 = fmax(y1, __shfl_xor(y1, m));
  }
  if (lane == 0) {
    double* b = boxes + 4 * (size_t)p;
    b[0] = x0, b[1] = y0, b[2] = x1, b[3] = y1;
  }
}

// max that propagates NaN, as np.max does
__device__ inline double nan_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

struct AreaConsts {
  double half_length, half_width, rear_axle_to_center;
  double compliance_threshold, violation_threshold;
  int horizon;
  int cull;
};

__global__ __launch_bounds__(64 * AWAVES) void ego_areas_kernel(
    const double* __restrict__ states, int per_group, int blocks_per_group, const double* __restrict__ verts,
    const int32_t* __restrict__ ring_off, const int32_t* __restrict__ poly_ring_off,
    const uint8_t* __restrict__ poly_kind, const int32_t* __restrict__ scene_poly_off,
    const double* __restrict__ boxes, AreaConsts k, uint8_t* __restrict__ out_areas, double* __restrict__ out_scores,
    double* __restrict__ out_progress, double* __restrict__ out_coords) {
  __shared__ double sVx[RING_CHUNK + 1], sVy[RING_CHUNK + 1];
  __shared__ double sBox[AWAVES][4];
  __shared__ double sPolyBox[64 * AWAVES][4];   // the listed polygons' boxes
  __shared__ int sPolyRing[64 * AWAVES][3];     // their first ring, the ring past their last, their kind
  __shared__ int sCount[AWAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x / blocks_per_group;
  const int slot = (blockIdx.x - g * blocks_per_group) * AWAVES + wave;
  const bool live = slot < per_group;
  // a spare wavefront repeats the group's last candidate (uniform barriers) and stores nothing
  const size_t n = (size_t)g * per_group + (live ? slot : per_group - 1);
  const bool row = lane < AT;
  const int t = row ? lane : AT - 1;   // a spare lane repeats state 40, stores nothing

  const double* S = states + (n * AT + t) * ANS;
  const double x = S[0], y = S[1], h = S[2];
  const double half_pi = M_PI / 2.0;
  const double ch = cos(h), sh = sin(h), cq = cos(h + half_pi), sq = sin(h + half_pi);
  double px[NPTS], py[NPTS];
  px[4] = x + k.rear_axle_to_center * ch, py[4] = y + k.rear_axle_to_center * sh;
  const double lon[4] = {k.half_length, -k.half_length, -k.half_length, k.half_length};
  const double lat[4] = {k.half_width, k.half_width, -k.half_width, -k.half_width};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    px[c] = px[4] + ((lat[c] * cq) + (lon[c] * ch));
    py[c] = py[4] + ((lat[c] * sq) + (lon[c] * sh));
  }

  // the workgroup's box: what none of its points can leave (fmin / fmax drop a NaN: such a point is in no polygon)
  const double inf = std::numeric_limits<double>::infinity();
  double bx0 = inf, by0 = inf, bx1 = -inf, by1 = -inf;
#pragma unroll
  for (int c = 0; c < NPTS; ++c)
    bx0 = fmin(bx0, px[c]), by0 = fmin(by0, py[c]), bx1 = fmax(bx1, px[c]), by1 = fmax(by1, py[c]);
  for (int m = 1; m < 64; m <<= 1) {
    bx0 = fmin(bx0, __shfl_xor(bx0, m)), by0 = fmin(by0, __shfl_xor(by0, m));
    bx1 = fmax(bx1, __shfl_xor(bx1, m)), by1 = fmax(by1, __shfl_xor(by1, m));
  }
  if (lane == 0) sBox[wave][0] = bx0, sBox[wave][1] = by0, sBox[wave][2] = bx1, sBox[wave][3] = by1;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < AWAVES; ++w) {
    bx0 = fmin(bx0, sBox[w][0]), by0 = fmin(by0, sBox[w][1]);
    bx1 = fmax(bx1, sBox[w][2]), by1 = fmax(by1, sBox[w][3]);
  }

  int lanes_with_corner = 0;     // lane-class polygons that hold at least one corner
  bool one_holds_all = false;    // a lane-class polygon holds all four
  unsigned in_drivable = 0;      // per corner: in some drivable-class polygon
  bool center_on_route = false;  // the center is in an on-route lane-class polygon

  // The scene's polygons, 256 at a time: every thread holds one polygon's box against the workgroup's and the
  // survivors are listed in LDS in index order with their boxes, ring ranges and kinds (a serial walk over the
  // scene's boxes cost 200 dependent loads per workgroup). Then the workgroup goes through the list together.
  const int p_begin = scene_poly_off[g], p_end = scene_poly_off[g + 1];
  for (int base = p_begin; base < p_end; base += 64 * AWAVES) {
    const int mine_p = base + (int)threadIdx.x;
    bool keep = false;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
    if (mine_p < p_end) {
      const double* b = boxes + 4 * (size_t)mine_p;
      q0 = b[0], q1 = b[1], q2 = b[2], q3 = b[3];
      keep = !k.cull || (bx0 <= q2 && bx1 >= q0 && by0 <= q3 && by1 >= q1);
    }
    const unsigned long long kept = __ballot(keep);
    __syncthreads();   // the last list and the last chunk have been read
    if (lane == 0) sCount[wave] = __popcll(kept);
    __syncthreads();
    int slot_in_list = __popcll(kept & ((1ull << lane) - 1ull)), listed = 0;
#pragma unroll
    for (int w = 0; w < AWAVES; ++w) {
      if (w < wave) slot_in_list += sCount[w];
      listed += sCount[w];
    }
    if (keep) {
      sPolyBox[slot_in_list][0] = q0, sPolyBox[slot_in_list][1] = q1;
      sPolyBox[slot_in_list][2] = q2, sPolyBox[slot_in_list][3] = q3;
      sPolyRing[slot_in_list][0] = poly_ring_off[mine_p], sPolyRing[slot_in_list][1] = poly_ring_off[mine_p + 1];
      sPolyRing[slot_in_list][2] = poly_kind[mine_p];
    }
    __syncthreads();
    for (int li = 0; li < listed; ++li) {
      const double qx0 = sPolyBox[li][0], qy0 = sPolyBox[li][1], qx1 = sPolyBox[li][2], qy1 = sPolyBox[li][3];
      bool mine = false;
#pragma unroll
      for (int c = 0; c < NPTS; ++c) mine |= px[c] >= qx0 && px[c] <= qx1 && py[c] >= qy0 && py[c] <= qy1;
      const bool test = !k.cull || __ballot(mine) != 0ull;   // uniform over the wavefront
      unsigned parity = 0, on_edge = 0;
      // the same value in every lane: say so, and the ring and edge loops run on scalar counters
      const int r_end = __builtin_amdgcn_readfirstlane(sPolyRing[li][1]);
      for (int r = __builtin_amdgcn_readfirstlane(sPolyRing[li][0]); r < r_end; ++r) {
        const int v0 = ring_off[r], nv = ring_off[r + 1] - v0;
        for (int e0 = 0; e0 < nv; e0 += RING_CHUNK) {
          const int cnt = min(RING_CHUNK, nv - e0);   // edges e0 .. e0 + cnt - 1; edge e = vertex e -> (e + 1) % nv
          __syncthreads();                            // the last chunk has been read
          for (int i = threadIdx.x; i <= cnt; i += 64 * AWAVES) {
            const int v = e0 + i == nv ? 0 : e0 + i;
            sVx[i] = verts[2 * (size_t)(v0 + v)], sVy[i] = verts[2 * (size_t)(v0 + v) + 1];
          }
          __syncthreads();
          if (!test) continue;
          double a = sVx[0], bb = sVy[0];
          for (int e = 0; e < cnt; ++e) {
            const double c = sVx[e + 1], d = sVy[e + 1];
            const double dx = c - a, dy = d - bb;
            // An edge matters to a point only if the point's y lies in the edge's closed y range - the crossing rule
            // and the on-edge rule both need it - which is (y - b)(y - d) <= 0 (an underflow to 0 keeps the edge: the
            // test errs to the safe side). Most edges of a polygon near the path matter to no point of the wavefront.
            double ty[NPTS];
            bool near = false;
#pragma unroll
            for (int q = 0; q < NPTS; ++q) {
              ty[q] = py[q] - bb;
              near |= ty[q] * (py[q] - d) <= 0.0;
            }
            if (__ballot(near) != 0ull) {
#pragma unroll
              for (int q = 0; q < NPTS; ++q) {
                const double cross = dx * ty[q] - (px[q] - a) * dy;
                if ((bb > py[q]) != (d > py[q]) && (dy > 0.0 ? cross > 0.0 : cross < 0.0)) parity ^= 1u << q;
                if (cross == 0.0 && px[q] >= fmin(a, c) && px[q] <= fmax(a, c) && py[q] >= fmin(bb, d) &&
                    py[q] <= fmax(bb, d))
                  on_edge |= 1u << q;
              }
            }
            a = c, bb = d;
          }
        }
      }
      const unsigned in = parity & ~on_edge;
      const unsigned kind = (unsigned)__builtin_amdgcn_readfirstlane(sPolyRing[li][2]);
      if (kind & KIND_LANE) {
        lanes_with_corner += (in & 0xFu) != 0u;
        one_holds_all |= (in & 0xFu) == 0xFu;
        center_on_route |= (kind & KIND_ROUTE) && (in & 0x10u);
      }
      if (kind & KIND_DRIVABLE) in_drivable |= in & 0xFu;
    }
  }

  const bool multiple = lanes_with_corner > 1 && !one_holds_all;
  const bool non_drivable = in_drivable != 0xFu;
  const bool oncoming = !center_on_route;

  // driving direction: p[t] where the flag AT t is set, the window sums over t - horizon .. t, their NaN-keeping max
  const double ddx = px[4] - __shfl_up(px[4], 1), ddy = py[4] - __shfl_up(py[4], 1);
  const double step = (row && lane >= 1 && oncoming) ? sqrt(ddx * ddx + ddy * ddy) : 0.0;
  double win = step;
  for (int j = 1; j <= k.horizon; ++j) {
    const double u = __shfl_up(step, j);
    if (lane >= j) win += u;
  }
  double m = win;   // lanes past the series hold sums of real steps and zeros: no more than lane 40's
  for (int s = 1; s < 64; s <<= 1) m = nan_max(m, __shfl_xor(m, s));
  const bool any_off = __ballot(row && non_drivable) != 0ull;

  if (!live) return;
  if (row) {
    uint8_t* A = out_areas + (n * AT + lane) * 3;
    A[0] = multiple, A[1] = non_drivable, A[2] = oncoming;
    if (out_coords) {
      double* C = out_coords + (n * AT + lane) * (NPTS * 2);
#pragma unroll
      for (int c = 0; c < NPTS; ++c) C[2 * c] = px[c], C[2 * c + 1] = py[c];
    }
  }
  if (lane == 0) {
    out_scores[2 * n] = any_off ? 0.0 : 1.0;
    out_scores[2 * n + 1] = m < k.compliance_threshold ? 1.0 : (m < k.violation_threshold ? 0.5 : 0.0);
    if (out_progress) out_progress[n] = m;
  }
}

}  // namespace

size_t ego_areas_work_doubles(int P) { return 4 * (size_t)(P > 0 ? P : 1); }

void launch_ego_areas(const double* states, int N, int per_group, const dd_drivable_maps& maps, int G,
                      const dd_area_params& p, int horizon, double* work, uint8_t* out_areas, double* out_scores,
                      double* out_progress, double* out_coords, hipStream_t st) {
  const int P = maps.num_polys;
  if (P > 0) {
    hipLaunchKernelGGL(area_boxes_kernel, dim3((unsigned)((P + AWAVES - 1) / AWAVES)), dim3(64 * AWAVES), 0, st,
                       maps.verts, maps.ring_off, maps.poly_ring_off, P, work);
    DD_HIP_CHECK(hipGetLastError());
  }
  // DDMI_EGO_AREAS_CULL=0: every polygon tested by every wavefront (tools/bench_ego_areas.py measures what the
  // bounding boxes save); the results are the same
  const char* env = std::getenv("DDMI_EGO_AREAS_CULL");
  AreaConsts k;
  k.half_length = p.half_length, k.half_width = p.half_width, k.rear_axle_to_center = p.rear_axle_to_center;
  k.compliance_threshold = p.driving_direction_compliance_threshold;
  k.violation_threshold = p.driving_direction_violation_threshold;
  k.horizon = horizon;
  k.cull = !(env && env[0] == '0');
  const int blocks_per_group = (per_group + AWAVES - 1) / AWAVES;
  hipLaunchKernelGGL(ego_areas_kernel, dim3((unsigned)G * (unsigned)blocks_per_group), dim3(64 * AWAVES), 0, st,
                     states, per_group, blocks_per_group, maps.verts, maps.ring_off, maps.poly_ring_off,
                     maps.poly_kind, maps.scene_poly_off, work, k, out_areas, out_scores, out_progress, out_coords);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
