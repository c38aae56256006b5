// PDM-Closed's proposal generation on the device (dd_proposals, include/ddmi.h): PDMGenerator.generate_proposals
// (pdm_planner/proposal/pdm_generator.py:68-95, 185-366) with BatchIDMPolicy.propagate (proposal/batch_idm_policy.py:
// 102-168) and PDMPath.interpolate / substring (utils/pdm_path.py:67-105), and the pick of the best proposal
// (dd_pdm_select: np.argmax over a scene's scores). float64 throughout; built with -ffp-contract=off (scipy's
// slope * dx + y_lo, the IDM's separate products and sums, the lever arms of ego_areas.hip). Deterministic: no atomics.
//
// Three launches, split where the reference's own caches split the work:
//   1. setup, one thread per (scene, path): the start's projection on the path, state 0, the driving corridor as a
//      point list (the path's vertices inside the interval; with one or none inside, shapely's substring: the two
//      interpolated ends and the vertices strictly between) and its bounding box, into the scratch.
//   2. corridor, one wavefront per (scene, path, update index), lane j holding object j of the scene (tracks, then
//      stop polygons), 64 at a time: whether the object at that time meets the corridor and, if so, the progress of
//      its centroid along the whole path (NaN otherwise), into the scratch. Independent of the proposals.
//   3. rollout, one wavefront per (scene, path): lane l holds proposal l (policy l) of the path. The reference fills
//      ONE scratch row for all proposals of a path at an update index and never clears it (pdm_generator.py:258-312: a
//      leader found after a free-driving proposal keeps that proposal's rear length, a red light after a track keeps
//      the track's velocity), so the proposals of a path are walked in order at every update: per proposal the lanes
//      take the objects ahead, each computes its distance to the ego quad, a butterfly finds the least (the lowest
//      index on a tie). Then every lane advances its IDM state and interpolates the path.
// No LDS and no barrier. An object is a simple ring - a box is a ring of four - and meets a convex quad when one of its
// edges meets it (the closed separating-axis test of collisions.hip on a segment) or the quad's first corner lies
// inside it (ego_areas.hip's crossing rule): for a box this is the quad - quad test's own set. Coordinates sit at
// 6.6e5 / 4.0e6 m: every product is of differences against a segment start, a disc centre or the ego quad's corner.
#include <cmath>
#include <cstdlib>
#include <limits>

#include "../../include/ddmi.h"
#include "common.h"

namespace ddmi {

namespace {

constexpr int PT = 41;             // states per proposal
constexpr int PNS = 11;            // StateIndex size
constexpr int PWAVES = 4;          // wavefronts per workgroup of the corridor pass
constexpr int HDR = 24;            // doubles per (scene, path) header in the scratch
constexpr int MAX_UPDATES = 40;    // update indices per path the scratch holds (rate 1)
constexpr double CULL_SLACK = 0x1p-10;   // metres

// the header of one (scene, path)
enum { H_PROGRESS = 0, H_X0, H_Y0, H_H0, H_AX, H_AY, H_BX, H_BY, H_BOX, H_I0 = 12, H_I1, H_FLAGS, H_FIRST, H_LAST,
       H_LENGTH, H_POINTS };

struct PropConsts {
  double min_gap, headway, accel, decel, dt, exponent;
  double half_length, half_width, rear_axle_to_center;
  int rate, corridor_poses, updates, cull;
};

struct Scene {
  const double* verts;          // (V, 3)
  const double* progress;       // (V)
  const int32_t* path_off;      // (G P + 1)
  const double* boxes;          // (K, T_obs, 4, 2)
  const uint8_t* valid;         // (K, T_obs)
  const double* heading;        // (K)
  const double* speed;          // (K)
  const int32_t* track_off;     // (G + 1)
  const double* stop_verts;     // (Vs, 2)
  const int32_t* ring_off;      // (R + 1)
  const int32_t* scene_ring_off;  // (G + 1)
  int T_obs, P, L;
};

// np.clip on one value: a NaN stays
__device__ inline double clip(double x, double lo, double hi) { return x != x ? x : fmin(fmax(x, lo), hi); }

// searchsorted(s, c) (side left) clipped to [1, V - 1]: numpy sorts a NaN behind everything
__device__ inline int upper_vertex(const double* __restrict__ s, int V, double c) {
  int lo = 0, hi = V;   // the first index with s[i] >= c
  if (c != c) lo = V;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo < 1 ? 1 : (lo > V - 1 ? V - 1 : lo);
}

// PDMPath.interpolate for one distance: (x, y, heading)
__device__ inline void interpolate(const double* __restrict__ xyh, const double* __restrict__ s, int V, double d,
                                   double& ox, double& oy, double& oh) {
  const double c = clip(d, 1e-5, s[V - 1]);
  const int hi = upper_vertex(s, V, c), lo = hi - 1;
  const double run = s[hi] - s[lo], at = c - s[lo];
  double o[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double slope = (xyh[3 * hi + k] - xyh[3 * lo + k]) / run;
    o[k] = slope * at + xyh[3 * lo + k];
  }
  o[2] = atan2(sin(o[2]), cos(o[2]));
  ox = o[0] != o[0] ? 0.0 : o[0], oy = o[1] != o[1] ? 0.0 : o[1], oh = o[2] != o[2] ? 0.0 : o[2];
}

// LineString.project by pdm_aggregate.hip's rule over the (V, 3) vertices of a path
__device__ inline double project_on(const double* __restrict__ xyh, int V, double qx, double qy) {
  double best = std::numeric_limits<double>::infinity(), at = std::numeric_limits<double>::quiet_NaN();
  double passed = 0.0;
  double ax = xyh[0], ay = xyh[1];
  for (int v = 1; v < V; ++v) {
    const double bx = xyh[3 * v], by = xyh[3 * v + 1];
    const double dx = bx - ax, dy = by - ay;
    const double len2 = dx * dx + dy * dy, len = sqrt(len2);
    const double wx = qx - ax, wy = qy - ay;
    double s = len2 > 0.0 ? (wx * dx + wy * dy) / len2 : 0.0;
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const double ex = wx - s * dx, ey = wy - s * dy;
    const double d2 = ex * ex + ey * ey;
    if (d2 < best) best = d2, at = passed + s * len;
    passed += len;
    ax = bx, ay = by;
  }
  return at;
}

// the point of the polyline at arc length d by the path's own cumulative progress (shapely's interpolate)
__device__ inline void point_at(const double* __restrict__ xyh, const double* __restrict__ s, int V, double d,
                                double& ox, double& oy) {
  const int hi = upper_vertex(s, V, d), lo = hi - 1;
  ox = xyh[3 * lo], oy = xyh[3 * lo + 1];
  if (s[hi] == s[lo]) return;
  const double f = (d - s[lo]) / (s[hi] - s[lo]);
  ox = ox + f * (xyh[3 * hi] - ox), oy = oy + f * (xyh[3 * hi + 1] - oy);
}

// max that keeps a NaN, as np.max does
__device__ inline double nan_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

// point i of the corridor's point list
__device__ inline void corridor_point(const double* __restrict__ hdr, const double* __restrict__ xyh, int i, int M,
                                      double& x, double& y) {
  const int flags = (int)hdr[H_FLAGS], has_a = flags & 1, has_b = (flags >> 1) & 1;
  if (has_a && i == 0) {
    x = hdr[H_AX], y = hdr[H_AY];
  } else if (has_b && i == M - 1) {
    x = hdr[H_BX], y = hdr[H_BY];
  } else {
    const int v = (int)hdr[H_I0] + i - has_a;
    x = xyh[3 * v], y = xyh[3 * v + 1];
  }
}

__global__ __launch_bounds__(64) void setup_kernel(Scene sc, const double* __restrict__ ego, const double* __restrict__ targets,
                                                   int paths, PropConsts k, double* __restrict__ work) {
  const int gp = blockIdx.x * 64 + threadIdx.x;
  if (gp >= paths) return;
  const int g = gp / sc.P;
  const int v0 = sc.path_off[gp], V = sc.path_off[gp + 1] - v0;
  const double* xyh = sc.verts + 3 * (size_t)v0;
  const double* s = sc.progress + v0;
  double* hdr = work + (size_t)HDR * gp;
  const double ego_progress = project_on(xyh, V, ego[(size_t)g * PNS], ego[(size_t)g * PNS + 1]);
  hdr[H_PROGRESS] = ego_progress;
  interpolate(xyh, s, V, ego_progress, hdr[H_X0], hdr[H_Y0], hdr[H_H0]);
  double top = targets[(size_t)g * sc.L];
  for (int l = 1; l < sc.L; ++l) top = nan_max(top, targets[(size_t)g * sc.L + l]);
  const double length = s[V - 1];
  const double far = ego_progress + (fabs(top) * (double)k.corridor_poses) * k.dt;
  const double start = clip(ego_progress, 0.0, length), end = clip(far, 0.0, length);
  int count = 0, i0 = 0, i1 = -1;
  for (int v = 0; v < V; ++v)
    if (start <= s[v] && s[v] <= end) {
      if (!count) i0 = v;
      i1 = v, ++count;
    }
  int flags = 0;
  double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
  if (count <= 1) {   // shapely's substring
    flags = 1;
    point_at(xyh, s, V, start, ax, ay);
    i0 = 0, i1 = -1;
    if (start == end || start != start || end != end) {
      // one point (a NaN interval holds nothing either)
    } else {
      flags = 3;
      point_at(xyh, s, V, end, bx, by);
      bool any = false;
      for (int v = 0; v < V; ++v)
        if (start < s[v] && s[v] < end) {
          if (!any) i0 = v;
          i1 = v, any = true;
        }
    }
  }
  hdr[H_AX] = ax, hdr[H_AY] = ay, hdr[H_BX] = bx, hdr[H_BY] = by;
  hdr[H_I0] = (double)i0, hdr[H_I1] = (double)i1, hdr[H_FLAGS] = (double)flags;
  const int M = (flags & 1) + (i1 - i0 + 1) + ((flags >> 1) & 1);
  hdr[H_POINTS] = (double)M, hdr[H_LENGTH] = length;
  // the first and the last segment of positive length take the square caps; the bounding box of all points
  const double inf = std::numeric_limits<double>::infinity();
  double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
  int first = -1, last = -1;
  double px = 0.0, py = 0.0;
  for (int i = 0; i < M; ++i) {
    double x, y;
    corridor_point(hdr, xyh, i, M, x, y);
    x0 = fmin(x0, x), y0 = fmin(y0, y), x1 = fmax(x1, x), y1 = fmax(y1, y);
    if (i > 0) {
      const double dx = x - px, dy = y - py;
      if (dx * dx + dy * dy > 0.0) {
        if (first < 0) first = i - 1;
        last = i - 1;
      }
    }
    px = x, py = y;
  }
  hdr[H_FIRST] = (double)first, hdr[H_LAST] = (double)last;
  // every point of the region is within r sqrt(2) of a point of the list (the caps' corners)
  const double grow = 1.5 * k.half_width + CULL_SLACK;
  hdr[H_BOX] = x0 - grow, hdr[H_BOX + 1] = y0 - grow, hdr[H_BOX + 2] = x1 + grow, hdr[H_BOX + 3] = y1 + grow;
}

// true where the two points of a (relative coordinates) and the four of b are separated along (nx, ny)
__device__ inline bool separated_on(double nx, double ny, const double* ax, const double* ay, const double* bx,
                                    const double* by) {
  const double p = nx * ax[0] + ny * ay[0], q = nx * ax[1] + ny * ay[1];
  const double a0 = fmin(p, q), a1 = fmax(p, q);
  double b0 = nx * bx[0] + ny * by[0], b1 = b0;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const double v = nx * bx[i] + ny * by[i];
    b0 = fmin(b0, v), b1 = fmax(b1, v);
  }
  return a1 < b0 || b1 < a0;
}

// closed intersection of the segment (sx, sy)[2] with the convex quad (tx, ty)[4]: collisions.hip's test, every
// coordinate taken relative to the segment's first point before any product
__device__ inline bool segment_touches(const double* sx, const double* sy, const double* tx, const double* ty) {
  double ax[2] = {0.0, sx[1] - sx[0]}, ay[2] = {0.0, sy[1] - sy[0]}, bx[4], by[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bx[i] = tx[i] - sx[0], by[i] = ty[i] - sy[0];
  bool sep = separated_on(-ay[1], ax[1], ax, ay, bx, by);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int f = (e + 1) & 3;
    sep |= separated_on(-(by[f] - by[e]), bx[f] - bx[e], ax, ay, bx, by);
  }
  return !sep;
}

// squared distance of the point p to the segment a - b
__device__ inline double point_segment2(double px, double py, double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  const double len2 = dx * dx + dy * dy;
  const double wx = px - ax, wy = py - ay;
  double s = len2 > 0.0 ? (wx * dx + wy * dy) / len2 : 0.0;
  s = fmin(fmax(s, 0.0), 1.0);
  const double ex = wx - s * dx, ey = wy - s * dy;
  return ex * ex + ey * ey;
}

// An object: n vertices (x, y) in a row, the closing edge implied. Against a quad given relative to the origin o:
// whether a ring edge meets the quad or the quad's first corner is strictly inside the ring (ego_areas.hip's rule),
// and the least squared distance between the two boundaries.
__device__ inline bool ring_meets_quad(const double* __restrict__ v, int n, double ox, double oy, const double* qx,
                                       const double* qy) {
  bool parity = false, on_edge = false, touch = false;
  double ax = v[0] - ox, ay = v[1] - oy;
  for (int e = 0; e < n; ++e) {
    const int w = e + 1 == n ? 0 : e + 1;
    const double cx = v[2 * w] - ox, cy = v[2 * w + 1] - oy;
    const double sx[2] = {ax, cx}, sy[2] = {ay, cy};
    touch |= segment_touches(sx, sy, qx, qy);
    const double dx = cx - ax, dy = cy - ay;
    const double cross = dx * (qy[0] - ay) - (qx[0] - ax) * dy;
    if ((ay > qy[0]) != (cy > qy[0]) && (dy > 0.0 ? cross > 0.0 : cross < 0.0)) parity = !parity;
    if (cross == 0.0 && qx[0] >= fmin(ax, cx) && qx[0] <= fmax(ax, cx) && qy[0] >= fmin(ay, cy) && qy[0] <= fmax(ay, cy))
      on_edge = true;
    ax = cx, ay = cy;
  }
  return touch || (parity && !on_edge);
}

// whether the ring meets the closed disc of radius r about c: the centre strictly inside, or within r of an edge
__device__ inline bool ring_meets_disc(const double* __restrict__ v, int n, double cx0, double cy0, double r) {
  bool parity = false, on_edge = false;
  double least = std::numeric_limits<double>::infinity();
  double ax = v[0] - cx0, ay = v[1] - cy0;
  for (int e = 0; e < n; ++e) {
    const int w = e + 1 == n ? 0 : e + 1;
    const double cx = v[2 * w] - cx0, cy = v[2 * w + 1] - cy0;
    least = fmin(least, point_segment2(0.0, 0.0, ax, ay, cx, cy));
    const double dx = cx - ax, dy = cy - ay;
    const double cross = dx * (0.0 - ay) - (0.0 - ax) * dy;
    if ((ay > 0.0) != (cy > 0.0) && (dy > 0.0 ? cross > 0.0 : cross < 0.0)) parity = !parity;
    if (cross == 0.0 && 0.0 >= fmin(ax, cx) && 0.0 <= fmax(ax, cx) && 0.0 >= fmin(ay, cy) && 0.0 <= fmax(ay, cy))
      on_edge = true;
    ax = cx, ay = cy;
  }
  return (parity && !on_edge) || least <= r * r;
}

__device__ bool meets_corridor(const double* __restrict__ v, int n, const double* __restrict__ hdr,
                               const double* __restrict__ xyh, double r) {
  const int M = (int)hdr[H_POINTS], first = (int)hdr[H_FIRST], last = (int)hdr[H_LAST];
  double ax, ay;
  corridor_point(hdr, xyh, 0, M, ax, ay);
  if (first < 0) return ring_meets_disc(v, n, ax, ay, r);
  for (int i = 0; i + 1 < M; ++i) {
    double bx, by;
    corridor_point(hdr, xyh, i + 1, M, bx, by);
    if (i > 0 && ring_meets_disc(v, n, ax, ay, r)) return true;   // an interior vertex
    const double dx = bx - ax, dy = by - ay;
    const double len2 = dx * dx + dy * dy;
    if (len2 > 0.0) {
      const double len = sqrt(len2);
      const double ux = dx / len, uy = dy / len;
      const double nx = -uy, ny = ux;
      const double sx = i == first ? -(r * ux) : 0.0, sy = i == first ? -(r * uy) : 0.0;
      const double ex = i == last ? dx + r * ux : dx, ey = i == last ? dy + r * uy : dy;
      const double qx[4] = {sx + r * nx, ex + r * nx, ex - r * nx, sx - r * nx};
      const double qy[4] = {sy + r * ny, ey + r * ny, ey - r * ny, sy - r * ny};
      if (ring_meets_quad(v, n, ax, ay, qx, qy)) return true;
    }
    ax = bx, ay = by;
  }
  return false;
}

// the polygon area centroid against the first vertex (the vertex mean for zero area); a box by collisions.hip's formula
__device__ inline void ring_centroid(const double* __restrict__ v, int n, bool box, double& cx, double& cy) {
  if (box) {
    const double ux = v[2] - v[0], uy = v[3] - v[1], vx = v[4] - v[0], vy = v[5] - v[1];
    const double wx = v[6] - v[0], wy = v[7] - v[1];
    const double a1 = ux * vy - vx * uy, a2 = vx * wy - wx * vy;
    const double a = a1 + a2;
    if (a == 0.0) {
      cx = v[0] + ((ux + vx) + wx) / 4.0, cy = v[1] + ((uy + vy) + wy) / 4.0;
      return;
    }
    cx = v[0] + (a1 * (ux + vx) + a2 * (vx + wx)) / (3.0 * a);
    cy = v[1] + (a1 * (uy + vy) + a2 * (vy + wy)) / (3.0 * a);
    return;
  }
  double area = 0.0, mx = 0.0, my = 0.0, sx = 0.0, sy = 0.0;
  double ax = 0.0, ay = 0.0;
  for (int e = 0; e < n; ++e) {
    const int w = e + 1 == n ? 0 : e + 1;
    const double bx = v[2 * w] - v[0], by = v[2 * w + 1] - v[1];
    const double cross = ax * by - bx * ay;
    area += cross;
    mx += (ax + bx) * cross, my += (ay + by) * cross;
    sx += ax, sy += ay;
    ax = bx, ay = by;
  }
  if (area == 0.0) {
    cx = v[0] + sx / (double)n, cy = v[1] + sy / (double)n;
    return;
  }
  cx = v[0] + mx / (3.0 * area), cy = v[1] + my / (3.0 * area);
}

// object j of scene g at time t: its vertices, or null where a track is absent
__device__ inline const double* object_at(const Scene& sc, int g, int j, int t, int& n) {
  const int k0 = sc.track_off[g], tracks = sc.track_off[g + 1] - k0;
  if (j < tracks) {
    n = 4;
    const size_t at = (size_t)(k0 + j) * sc.T_obs + t;
    return sc.valid[at] ? sc.boxes + at * 8 : nullptr;
  }
  const int r = sc.scene_ring_off[g] + (j - tracks);
  n = sc.ring_off[r + 1] - sc.ring_off[r];
  return sc.stop_verts + 2 * (size_t)sc.ring_off[r];
}

__device__ inline int objects_of(const Scene& sc, int g) {
  return (sc.track_off[g + 1] - sc.track_off[g]) + (sc.scene_ring_off[g + 1] - sc.scene_ring_off[g]);
}

// where the (scene, path)'s rows of the corridor pass start: `paths` headers, then per scene P paths x MAX_UPDATES rows
__device__ inline double* rows_of(double* work, const Scene& sc, int paths, int g, int p, int objects) {
  const size_t before = (size_t)sc.track_off[g] + (size_t)sc.scene_ring_off[g];
  return work + (size_t)HDR * paths + ((size_t)sc.P * before + (size_t)p * objects) * MAX_UPDATES;
}

__global__ __launch_bounds__(64 * PWAVES) void corridor_kernel(Scene sc, int paths, PropConsts k,
                                                               double* __restrict__ work) {
  const int w = blockIdx.x * PWAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= paths * k.updates) return;   // no barrier: a spare wavefront leaves
  const int gp = w / k.updates, e = w - gp * k.updates;
  const int g = gp / sc.P, p = gp - g * sc.P;
  const int t = k.rate * (e + 1);
  const int objects = objects_of(sc, g);
  const int v0 = sc.path_off[gp], V = sc.path_off[gp + 1] - v0;
  const double* xyh = sc.verts + 3 * (size_t)v0;
  const double* hdr = work + (size_t)HDR * gp;
  double* row = rows_of(work, sc, paths, g, p, objects) + (size_t)e * objects;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int j = lane; j < objects; j += 64) {
    int n;
    const double* v = object_at(sc, g, j, t, n);
    double at = nan;
    bool near = v != nullptr;
    if (near && k.cull) {
      const double inf = std::numeric_limits<double>::infinity();
      double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
      for (int i = 0; i < n; ++i)
        x0 = fmin(x0, v[2 * i]), y0 = fmin(y0, v[2 * i + 1]), x1 = fmax(x1, v[2 * i]), y1 = fmax(y1, v[2 * i + 1]);
      near = hdr[H_BOX] <= x1 && hdr[H_BOX + 2] >= x0 && hdr[H_BOX + 1] <= y1 && hdr[H_BOX + 3] >= y0;
    }
    if (near && meets_corridor(v, n, hdr, xyh, k.half_width)) {
      double cx, cy;
      ring_centroid(v, n, j < sc.track_off[g + 1] - sc.track_off[g], cx, cy);
      at = project_on(xyh, V, cx, cy);
    }
    row[j] = at;
  }
}

// ego_polygon.distance(object) squared: 0 where they intersect, else the least point-to-segment distance of the two
// boundaries, on coordinates relative to the ego quad's first corner (ox, oy); (qx, qy) is the quad so taken
__device__ inline double distance2(const double* __restrict__ v, int n, double ox, double oy, const double* qx,
                                   const double* qy) {
  if (ring_meets_quad(v, n, ox, oy, qx, qy)) return 0.0;
  double best = std::numeric_limits<double>::infinity();
  double ax = v[0] - ox, ay = v[1] - oy;
  for (int e = 0; e < n; ++e) {
    const int w = e + 1 == n ? 0 : e + 1;
    const double bx = v[2 * w] - ox, by = v[2 * w + 1] - oy;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      best = fmin(best, point_segment2(qx[c], qy[c], ax, ay, bx, by));
      best = fmin(best, point_segment2(ax, ay, qx[c], qy[c], qx[(c + 1) & 3], qy[(c + 1) & 3]));
    }
    ax = bx, ay = by;
  }
  return best;
}

__global__ __launch_bounds__(64) void rollout_kernel(Scene sc, const double* __restrict__ ego,
                                                     const double* __restrict__ targets, int paths, PropConsts k,
                                                     double* __restrict__ work, double* __restrict__ out_proposals,
                                                     double* __restrict__ out_idm, double* __restrict__ out_lead,
                                                     int32_t* __restrict__ out_index) {
  const int gp = blockIdx.x, lane = threadIdx.x;
  const int g = gp / sc.P, p = gp - g * sc.P;
  const int v0 = sc.path_off[gp], V = sc.path_off[gp + 1] - v0;
  const double* xyh = sc.verts + 3 * (size_t)v0;
  const double* s = sc.progress + v0;
  const double* hdr = work + (size_t)HDR * gp;
  const int objects = objects_of(sc, g), tracks = sc.track_off[g + 1] - sc.track_off[g];
  const double* rows = rows_of(work, sc, paths, g, p, objects);
  const bool mine = lane < sc.L;
  const size_t n = (size_t)gp * sc.L + (mine ? lane : 0);
  const double target = targets[(size_t)g * sc.L + (mine ? lane : 0)];

  double x = hdr[H_PROGRESS], vel = ego[(size_t)g * PNS + 3];
  double px = hdr[H_X0], py = hdr[H_Y0], ph = hdr[H_H0];
  double lx = 0.0, lv = 0.0, lr = 0.0;   // the leader row: zero until the first update, as the reference's array
  int li = -1;
  const double half_pi = M_PI / 2.0;
  const double lon[4] = {k.half_length, -k.half_length, -k.half_length, k.half_length};
  const double lat[4] = {k.half_width, k.half_width, -k.half_width, -k.half_width};

  auto store = [&](int t) {
    if (!mine) return;
    double* o = out_proposals + (n * PT + t) * 3;
    o[0] = px, o[1] = py, o[2] = ph;
    if (out_idm) out_idm[(n * PT + t) * 2] = x, out_idm[(n * PT + t) * 2 + 1] = vel;
    if (out_lead) {
      double* q = out_lead + (n * PT + t) * 3;
      q[0] = lx, q[1] = lv, q[2] = lr;
    }
    if (out_index) out_index[n * PT + t] = li;
  };
  store(0);

  for (int t = 1; t < PT; ++t) {
    if (t % k.rate == 0) {
      const double* row = rows + (size_t)(t / k.rate - 1) * objects;
      double carry_v = 0.0, carry_r = 0.0;   // the reference's one scratch row per update, never cleared
      for (int l = 0; l < sc.L; ++l) {
        const double xl = __shfl(x, l), ex = __shfl(px, l), ey = __shfl(py, l), eh = __shfl(ph, l);
        // the ego quad at the state of t - 1 (ego_areas.hip's corners), relative to its first corner
        const double ch = cos(eh), sh = sin(eh), cq = cos(eh + half_pi), sq = sin(eh + half_pi);
        const double cx = ex + k.rear_axle_to_center * ch, cy = ey + k.rear_axle_to_center * sh;
        double qx[4], qy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          qx[c] = cx + ((lat[c] * cq) + (lon[c] * ch));
          qy[c] = cy + ((lat[c] * sq) + (lon[c] * sh));
        }
        const double ox = qx[0], oy = qy[0];
#pragma unroll
        for (int c = 0; c < 4; ++c) qx[c] -= ox, qy[c] -= oy;
        double best = std::numeric_limits<double>::infinity();
        int who = 0x7fffffff;
        for (int j = lane; j < objects; j += 64) {
          if (!(row[j] > xl)) continue;   // not in the corridor (NaN), or not strictly ahead
          int nv;
          const double* v = object_at(sc, g, j, t, nv);
          const double d2 = distance2(v, nv, ox, oy, qx, qy);
          if (d2 < best) best = d2, who = j;
        }
        for (int m = 1; m < 64; m <<= 1) {
          const double ob = __shfl_xor(best, m);
          const int ow = __shfl_xor(who, m);
          if (ob < best || (ob == best && ow < who)) best = ob, who = ow;
        }
        double row_x;
        int row_i = -1;
        if (who != 0x7fffffff) {
          row_x = xl + sqrt(best);
          row_i = who;
          if (who < tracks) {
            const int kk = sc.track_off[g] + who;
            const double rel = sc.heading[kk] - eh;
            carry_v = cos(atan2(sin(rel), cos(rel))) * sc.speed[kk];
          }
        } else {
          row_x = hdr[H_LENGTH];
          carry_r = k.half_length;
        }
        if (lane == l) lx = row_x, lv = carry_v, lr = carry_r, li = row_i;
      }
    }
    // BatchIDMPolicy.propagate
    const double s_star = (k.min_gap + vel * k.headway) + (vel * (vel - lv)) / (2.0 * sqrt(k.accel * k.decel));
    const double gap = (lx - x) - lr;
    const double s_alpha = gap != gap ? gap : fmax(gap, k.min_gap);
    const double ratio = s_star / s_alpha;
    const double v_dot = k.accel * ((1.0 - pow(vel / target, k.exponent)) - ratio * ratio);
    const double clipped = clip(v_dot, -k.decel, k.accel);
    x = x + k.dt * vel;
    vel = vel + k.dt * clipped;
    interpolate(xyh, s, V, x, px, py, ph);
    store(t);
  }
}

// np.argmax over a scene's scores (the first maximum; a NaN counts as the maximum), the winner's states and its
// raw progress * no_collision * drivable_area: one wavefront per scene
__global__ __launch_bounds__(64) void select_kernel(const double* __restrict__ score, const double* __restrict__ raw,
                                                    const double* __restrict__ no_collision,
                                                    const double* __restrict__ drivable_area,
                                                    const double* __restrict__ states, int per_group,
                                                    int32_t* __restrict__ out_index, double* __restrict__ out_states,
                                                    double* __restrict__ out_reference) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const size_t first = (size_t)g * per_group;
  double best = -std::numeric_limits<double>::infinity();
  int who = 0x7fffffff;
  bool nan = false;
  for (int i = lane; i < per_group; i += 64) {
    const double v = score[first + i];
    if (nan) continue;
    if (v != v) nan = true, who = i;
    else if (who == 0x7fffffff || v > best) best = v, who = i;
  }
  for (int m = 1; m < 64; m <<= 1) {
    const double ob = __shfl_xor(best, m);
    const int ow = __shfl_xor(who, m);
    const bool on = __shfl_xor((int)nan, m) != 0;
    bool take;
    if (ow == 0x7fffffff) take = false;
    else if (who == 0x7fffffff) take = true;
    else if (on != nan) take = on;
    else if (nan) take = ow < who;
    else take = ob > best || (ob == best && ow < who);
    if (take) best = ob, who = ow, nan = on;
  }
  const size_t n = first + who;
  if (lane == 0) {
    out_index[g] = who;
    out_reference[g] = raw[n] * (no_collision[n] * drivable_area[n]);
  }
  for (int i = lane; i < PT * PNS; i += 64) out_states[(size_t)g * PT * PNS + i] = states[n * PT * PNS + i];
}

}  // namespace

size_t proposals_work_doubles(int G, int P, int K, int R) {
  const size_t g = G > 0 ? G : 0, p = P > 0 ? P : 0, k = K > 0 ? K : 0, r = R > 0 ? R : 0;
  return 1 + (size_t)HDR * g * p + (size_t)MAX_UPDATES * p * (k + r);
}

void launch_proposals(const dd_paths& paths, const dd_lead_objects& obs, const double* ego_states,
                      const double* targets, int G, int L, const dd_idm_params& ip, const dd_area_params& ap,
                      double* work, double* out_proposals, double* out_idm, double* out_lead, int32_t* out_lead_index,
                      hipStream_t st) {
  Scene sc;
  sc.verts = paths.verts, sc.progress = paths.progress, sc.path_off = paths.path_off;
  sc.boxes = obs.boxes, sc.valid = obs.valid, sc.heading = obs.heading, sc.speed = obs.speed;
  sc.track_off = obs.scene_track_off, sc.stop_verts = obs.stop_verts, sc.ring_off = obs.ring_off;
  sc.scene_ring_off = obs.scene_ring_off;
  sc.T_obs = obs.num_times, sc.P = paths.paths_per_scene, sc.L = L;
  PropConsts k;
  k.min_gap = ip.min_gap_to_lead_agent, k.headway = ip.headway_time, k.accel = ip.accel_max, k.decel = ip.decel_max;
  k.dt = ip.dt, k.exponent = (double)ip.acceleration_exponent;
  k.half_length = ap.half_length, k.half_width = ap.half_width, k.rear_axle_to_center = ap.rear_axle_to_center;
  k.rate = ip.leading_agent_update_rate, k.corridor_poses = ip.corridor_poses;
  k.updates = (PT - 1) / k.rate;
  // DDMI_PROPOSALS_CULL=0: every object tested against every corridor; the results are the same
  const char* env = std::getenv("DDMI_PROPOSALS_CULL");
  k.cull = !(env && env[0] == '0');
  const int n_paths = G * sc.P;
  hipLaunchKernelGGL(setup_kernel, dim3((unsigned)((n_paths + 63) / 64)), dim3(64), 0, st, sc, ego_states, targets,
                     n_paths, k, work);
  DD_HIP_CHECK(hipGetLastError());
  if (obs.num_tracks + obs.num_rings > 0) {
    const long long waves = (long long)n_paths * k.updates;
    hipLaunchKernelGGL(corridor_kernel, dim3((unsigned)((waves + PWAVES - 1) / PWAVES)), dim3(64 * PWAVES), 0, st, sc,
                       n_paths, k, work);
    DD_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(rollout_kernel, dim3((unsigned)n_paths), dim3(64), 0, st, sc, ego_states, targets, n_paths, k, work,
                     out_proposals, out_idm, out_lead, out_lead_index);
  DD_HIP_CHECK(hipGetLastError());
}

void launch_pdm_select(const double* score, const double* raw_progress, const double* no_collision,
                       const double* drivable_area, const double* states, int G, int per_group, int32_t* out_index,
                       double* out_states, double* out_reference, hipStream_t st) {
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)G), dim3(64), 0, st, score, raw_progress, no_collision,
                     drivable_area, states, per_group, out_index, out_states, out_reference);
  DD_HIP_CHECK(hipGetLastError());
}

}  // namespace ddmi
