// The ground plane for the live path: every pose's position on the floor in millimetres through a calibrated
// homography, its track's speed and distance walked, its nearest neighbour, and the poses restated in floor units for
// the anchor-based consumers, on the device, in one launch for up to 32 frames of any number of cameras
// (pave_floor_update).
//
// The rule is DESIGN section 23 and is integer-exact.  A pose stands on section 17's anchor (ax, ay) in 1/8 pixel
// (pave_tracked.h: quant, the three anchor modes and the fallback to the box).  A camera holds nine int64 words G,
// the homography from 1/8 pixel to floor millimetres times a power of two, every row with (|g0| + |g1|) 65535 + |g2|
// < 2^61, and four bounds in mm.  With
//   nx = g00 ax + g01 ay + g02,  ny = g10 ax + g11 ay + g12,  w = g20 ax + g21 ay + g22          (|.| < 2^61)
// the pose is on the floor iff w > 0 and X = floor((2 nx + w) / (2 w)), Y likewise (|2 n + w| < 2^63), lie in the
// bounds, ends included.  A pose is placed iff keep, a box score above the threshold, finite coordinates and on the
// floor; it is followed iff it is placed, its id is >= 1, no placed pose before it has that id and it finds or takes a
// slot (pave_tracked.h's slots: the clock, the expiry after max_age frames, the serial births of one lane).  A born
// slot takes pos = (X, Y), vel = 0, travel = 0, hits = 1.  A slot that was there, with dt = frame - last and d = (X, Y)
// - pos: per axis m = floor(256 d / dt), vel = m when hits == 1, else vel += floor(gain (m - vel) / 16); travel =
// min(2^31 - 1, travel + isqrt(dx^2 + dy^2)); hits = min(hits + 1, 2^30).  Among the placed poses of the frame pose i's
// nearest is the j != i of the least squared distance, the lowest j on a tie, gap its isqrt, near the number of j != i
// within `near` mm.  The bridge: P = floor(4 (X - origin) / unit) per axis; with both in 0 .. 32767 every x and y of
// the pose's key points and box becomes P / 4 (exact in fp32), else NaN; scores are copied.
//
// One block of 256 threads per camera of the launch (pave_tracked.h).  The calibration goes into LDS once.  Its own
// order: classification, then the projection rewrites det_ok to "placed", and the slot scan runs after that.
// Per frame thread t < S expires slot t; thread d < N classes pose d, projects it (two 64-bit divisions: a software
// sequence on this hardware, so the quotients go to LDS as 32-bit words and nothing divides twice) and finds its slot;
// the N^2 neighbour pass runs over all 256 threads, two per pose, each over half of j (every lane of a wave reads the
// same j: an LDS broadcast), the upper half handing its best to the lower through LDS -- the lower half holds the lower
// j, so it keeps its own on a tie; after the serial births thread d does the slot and the outputs of pose d, and all
// threads write the floor-unit key points.  Every loop bound is from the plan or the maxima of the header, every
// barrier is block-uniform, there are no global atomics and no scratch area.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using namespace pave_tracked;

constexpr int NT = 256;                              // threads of a block
constexpr int MAXP = PAVE_TRACK_MAX_POSES;
constexpr int MAXS = PAVE_TRACK_MAX_TRACKS;
constexpr int CW = PAVE_FLOOR_CALIB_WORDS;
constexpr long long MM = PAVE_FLOOR_MAX_MM;
static_assert(2 * MAXP == NT && MAXS <= NT, "thread roles: two threads per pose in the neighbour pass");

// floor(sqrt(v)) for v < 2^63.  The double holds v to 53 bits and its square root is rounded once more, so the
// truncated root is off by one at the most, either way; the two corrections make it the floor.
__device__ __forceinline__ long long isqrt(const unsigned long long v) {
  unsigned long long r = (unsigned long long)sqrt((double)v);
  if (r * r > v) --r;
  if ((r + 1) * (r + 1) <= v) ++r;
  return (long long)r;
}

__device__ __forceinline__ unsigned long long dist2(const int ax, const int ay, const int bx, const int by) {
  const unsigned long long dx = (unsigned long long)((long long)ax - bx), dy = (unsigned long long)((long long)ay - by);
  return dx * dx + dy * dy;   // (differences of two int32: below 2^65 only for words no rule stores; unsigned wraps)
}

__global__ __launch_bounds__(NT) void floor_update_kernel(const pave_floor_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int det_id[MAXP];
  __shared__ int det_bad[MAXP];      // != 0: a coordinate that is not finite
  __shared__ int det_ok[MAXP];       // != 0: keep and a box score above the threshold; after the projection: placed
  __shared__ int det_slot[MAXP];     // the slot of a followed pose, or -1
  __shared__ int det_born[MAXP];     // != 0: the slot was born in this frame
  __shared__ int det_x[MAXP];        // of a placed pose: the floor position in mm
  __shared__ int det_y[MAXP];
  __shared__ int det_px[MAXP];       // of a pose on the plan: quarter floor pixels; else -1
  __shared__ int det_py[MAXP];
  __shared__ unsigned long long nb_d2[MAXP];   // the upper half's best of pose i
  __shared__ int nb_j[MAXP];
  __shared__ int nb_near[MAXP];
  __shared__ long long cal[CW];
  __shared__ int cam_state[2];       // frame, dropped

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S, K = plan.K;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_hits = plan.slot_hits + (long long)cam * S;
  int32_t* __restrict__ g_pos = plan.slot_pos + (long long)cam * S * 2;
  int32_t* __restrict__ g_vel = plan.slot_vel + (long long)cam * S * 2;
  int32_t* __restrict__ g_travel = plan.slot_travel + (long long)cam * S;

  if (tid < CW) {   // the calibration, its bounds clamped as they are read: a floor position is an int of 21 bits
    long long v = plan.calib[(long long)cam * CW + tid];
    if (tid >= PAVE_FLOOR_CALIB_BOUNDS && tid < PAVE_FLOOR_CALIB_BOUNDS + 4) v = min(max(v, -MM), MM);
    cal[tid] = v;
  }
  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.dropped[cam];
  }
  const long long near2 = (long long)plan.near * plan.near;

  for (int e = b; e < plan.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; cal and cam_state are written
    const int n = plan.n[e];
    const float sx = plan.scale[e][0], sy = plan.scale[e][1];
    const float* __restrict__ kpts = plan.kpts[e];
    const float* __restrict__ bboxes = plan.bboxes[e];
    const int32_t* __restrict__ keep = plan.keep[e];
    const int32_t* __restrict__ ids = plan.ids[e];
    int32_t* __restrict__ out = plan.out[e];
    float* __restrict__ out_kpts = plan.out_floor[e];
    float* __restrict__ out_boxes = plan.out_floor[e] + (long long)n * K * 3;
    const int frame = (int)((unsigned)cam_state[0] + 1u);

    // ---- expire the slots; the poses' boxes ----
    if (tid < MAXS) expire_slot(plan, g_id, g_last, slot_id, tid, S, frame);
    int X1 = 0, Y1 = 0, X2 = 0, Y2 = 0;
    if (tid < n)
      classify_pose(bboxes, keep, ids, sx, sy, plan.score_thr, tid, det_id, det_bad, det_ok, det_born, X1, Y1, X2, Y2);
    __syncthreads();
    sweep_finite<NT>(kpts, n, K, tid, det_bad);
    __syncthreads();

    // ---- the anchor, the projection and the bridge of pose tid: who is placed ----
    if (tid < n) {
      int placed = 0, X = 0, Y = 0, px = -1, py = -1;
      if (det_ok[tid] != 0 && det_bad[tid] == 0 && cal[PAVE_FLOOR_CALIB_VALID] != 0) {
        long long ax, ay;
        anchor(plan, kpts, tid, K, sx, sy, X1, Y1, X2, Y2, ax, ay);
        const long long nx = cal[0] * ax + cal[1] * ay + cal[2];
        const long long ny = cal[3] * ax + cal[4] * ay + cal[5];
        const long long w = cal[6] * ax + cal[7] * ay + cal[8];
        if (w > 0) {
          const long long fx = floor_div(2 * nx + w, 2 * w), fy = floor_div(2 * ny + w, 2 * w);
          if (fx >= cal[PAVE_FLOOR_CALIB_BOUNDS] && fy >= cal[PAVE_FLOOR_CALIB_BOUNDS + 1] &&
              fx <= cal[PAVE_FLOOR_CALIB_BOUNDS + 2] && fy <= cal[PAVE_FLOOR_CALIB_BOUNDS + 3]) {
            placed = 1;
            X = (int)fx, Y = (int)fy;
            const long long qx = floor_div(4 * (fx - plan.origin_x), plan.unit);
            const long long qy = floor_div(4 * (fy - plan.origin_y), plan.unit);
            if (qx >= 0 && qx <= QMAX && qy >= 0 && qy <= QMAX) px = (int)qx, py = (int)qy;
          }
        }
      }
      det_ok[tid] = placed;
      det_x[tid] = X;
      det_y[tid] = Y;
      det_px[tid] = px;
      det_py[tid] = py;
    }
    __syncthreads();

    // ---- the slot of every pose; the neighbours of pose tid % 128 among half of the poses ----
    if (tid < n)   // (det_ok is "placed" by now, and a placed pose is not bad)
      det_slot[tid] = find_slot(det_id, det_ok, nullptr, slot_id, tid, S);
    const int pose = tid & (MAXP - 1), upper = tid >> 7;
    unsigned long long best = ~0ull;
    int best_j = -1, close = 0;
    if (pose < n && det_ok[pose] != 0) {
      const int half = (n + 1) >> 1;
      const int lo = upper ? half : 0, hi = upper ? n : half;
      const int x = det_x[pose], y = det_y[pose];
      for (int j = lo; j < hi; ++j) {   // (ascending j and a strict <: the lowest j of the least distance)
        if (j == pose || det_ok[j] == 0) continue;
        const unsigned long long d2 = dist2(x, y, det_x[j], det_y[j]);
        if (d2 < best) best = d2, best_j = j;
        close += d2 <= (unsigned long long)near2 ? 1 : 0;
      }
    }
    if (upper) {
      nb_d2[pose] = best;
      nb_j[pose] = best_j;
      nb_near[pose] = close;
    }
    __syncthreads();
    if (tid == 0)   // births, in ascending pose index into the lowest free slot; the clock
      commit_births(plan, cam, n, S, frame, true, g_id, slot_id, det_id, det_slot, det_born, cam_state);
    __syncthreads();

    // ---- pose tid in its slot; its outputs ----
    if (tid < n) {   // (tid < 128: the lower half of the neighbour pass, which holds the lower j)
      if (nb_j[tid] >= 0 && nb_d2[tid] < best) best = nb_d2[tid], best_j = nb_j[tid];
      close += nb_near[tid];
      const int t = det_slot[tid];   // (in 0 .. S - 1 or -1: a slot index is a loop counter)
      const int X = det_x[tid], Y = det_y[tid];
      long long vx = 0, vy = 0, travel = 0;
      if (t >= 0) {
        int hits = 1;
        if (det_born[tid] == 0) {
          long long dt = (long long)frame - g_last[t];
          if (dt < 1) dt = 1;   // (a live slot of the rule was last seen in an earlier frame)
          const long long dx = (long long)X - g_pos[2 * t], dy = (long long)Y - g_pos[2 * t + 1];
          const long long mx = floor_div(256 * dx, dt), my = floor_div(256 * dy, dt);
          hits = g_hits[t];
          vx = g_vel[2 * t], vy = g_vel[2 * t + 1];
          if (hits == 1) {
            vx = mx, vy = my;
          } else {   // (>> of a negative int64 is the floor)
            vx += (plan.velocity_gain * (mx - vx)) >> 4;
            vy += (plan.velocity_gain * (my - vy)) >> 4;
          }
          travel = min(2147483647ll, (long long)g_travel[t] + isqrt(dist2(X, Y, g_pos[2 * t], g_pos[2 * t + 1])));
          hits = min(max(hits, 0) + 1, PAVE_FLOOR_MAX_HITS);
        }
        g_pos[2 * t] = X;
        g_pos[2 * t + 1] = Y;
        g_vel[2 * t] = (int32_t)vx;
        g_vel[2 * t + 1] = (int32_t)vy;
        g_travel[t] = (int32_t)travel;
        g_hits[t] = hits;
        g_last[t] = frame;
      }
      const int placed = det_ok[tid];
      const int ivx = (int32_t)vx, ivy = (int32_t)vy;
      out[tid] = placed;
      out[n + 2 * tid] = X;
      out[n + 2 * tid + 1] = Y;
      out[3 * n + 2 * tid] = ivx;
      out[3 * n + 2 * tid + 1] = ivy;
      out[5 * n + tid] = (int32_t)isqrt((unsigned long long)((long long)ivx * ivx) + (unsigned long long)((long long)ivy * ivy));
      out[6 * n + tid] = (int32_t)travel;
      out[7 * n + tid] = best_j;
      out[8 * n + tid] = best_j >= 0 ? (int32_t)isqrt(best) : -1;
      out[9 * n + tid] = close;
      const float qnan = __uint_as_float(0x7fc00000u);
      const float fx = det_px[tid] >= 0 ? (float)det_px[tid] * 0.25f : qnan;
      const float fy = det_px[tid] >= 0 ? (float)det_py[tid] * 0.25f : qnan;
      float* ob = out_boxes + tid * 5;
      ob[0] = fx, ob[1] = fy, ob[2] = fx, ob[3] = fy;
      ob[4] = bboxes[tid * 5 + 4];
    }
    for (int i = tid; i < n * K; i += NT) {   // the floor-unit key points: the pose's one point, its scores as they were
      const int d = i / K;
      const float qnan = __uint_as_float(0x7fc00000u);
      const bool there = det_px[d] >= 0;
      out_kpts[3 * i] = there ? (float)det_px[d] * 0.25f : qnan;
      out_kpts[3 * i + 1] = there ? (float)det_py[d] * 0.25f : qnan;
      out_kpts[3 * i + 2] = kpts[3 * i + 2];
    }
  }
}

}  // namespace

extern "C" {

int pave_floor_update(const pave_floor_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "floor_update: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "floor_update: K outside 1 .. 32");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_hits || !plan->slot_pos || !plan->slot_vel || !plan->slot_travel ||
      !plan->frame || !plan->dropped)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: null state tensor");
  if (!plan->calib) return pave_internal_fail(PAVE_E_ARG, "floor_update: null calibration tensor");
  if (plan->velocity_gain < 1 || plan->velocity_gain > PAVE_FLOOR_MAX_GAIN)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: velocity_gain outside 1 .. 16");
  if (plan->near < 0 || plan->near > PAVE_FLOOR_MAX_NEAR)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: near outside 0 .. 2^20");
  if (plan->unit < 1 || plan->unit > PAVE_FLOOR_MAX_UNIT)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: unit outside 1 .. 1000");
  if (plan->origin_x < -PAVE_FLOOR_MAX_MM || plan->origin_x > PAVE_FLOOR_MAX_MM || plan->origin_y < -PAVE_FLOOR_MAX_MM ||
      plan->origin_y > PAVE_FLOOR_MAX_MM)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: origin outside +-(2^20 - 1)");
  if (plan->anchor < PAVE_ZONE_ANCHOR_FEET || plan->anchor > PAVE_ZONE_ANCHOR_CENTRE)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: anchor outside 0 .. 2");
  if (plan->n_anchor < 0 || plan->n_anchor > PAVE_ZONE_MAX_ANCHOR_KPTS)
    return pave_internal_fail(PAVE_E_ARG, "floor_update: n_anchor outside 0 .. 4");
  for (int i = 0; i < plan->n_anchor; ++i)
    if (plan->anchor_kpt[i] < 0 || plan->anchor_kpt[i] >= plan->K)
      return pave_internal_fail(PAVE_E_ARG, "floor_update: an anchor key point outside [0, K)");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "floor_update: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "floor_update: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "floor_update: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "floor_update: null ids tensor");
    if (n > 0 && (!plan->out[i] || !plan->out_floor[i]))
      return pave_internal_fail(PAVE_E_ARG, "floor_update: null output tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "floor_update: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "floor_update: scale must be positive and finite");
  }
  return pave_launch<floor_update_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                          reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
