// What every update that follows track ids through per-camera slots has in common, once:
// smooth_poses_kernel, zone_events_kernel, posture_events_kernel, heat_update_kernel, trail_update_kernel,
// floor_update_kernel and contact_update_kernel are built from these steps, and the units that only quantise take quant
// from here.
//
// A coordinate becomes quarter pixels as in sections 13 and 14,
//   X = clamp((int)rintf((x / sx) * 4.f), 0, 32767)     (correctly rounded division, no contraction).
// One block works per camera of a launch: block b iff entry b is the first entry of its camera (owns_camera), and it
// then takes that camera's entries in plan order, so frame f + 1 reads the state frame f stored through the same
// block and no two blocks touch one camera's state.  A camera keeps S slots of (id, last, ...), id 0 = free, a clock
// `frame` and a drop count.  Per frame, with frame = clock + 1:
//   expire_slot    thread t: slot t is freed iff it is live and frame - last > max_age; slot_id[t] is what it holds now
//                  (0 for t >= S: t may run to the end of slot_id)
//   classify_pose  thread d: the box corners of pose d in quarter pixels; det_bad = a corner is not finite, which is
//                  also the return value; det_ok = keep and a box score above score_thr; det_id; det_born = 0
//   sweep_finite   all threads: det_bad |= a key point coordinate that is not finite
//   find_slot      thread d: pose d takes part iff det_ok, not det_bad, id >= 1 and no pose before it that passes the
//                  same three tests has its id; it then has the lowest live slot of its id, or NEEDS_BIRTH; else -1
//   commit_births  one lane: in ascending pose index a NEEDS_BIRTH pose takes the lowest free slot (det_born = 1), or,
//                  when there is none, slot -1 and dropped + 1; the clock and the drop count are stored whatever
//                  was born
//   anchor         thread d: where pose d stands, in 1/8 pixel: 'feet' floor(2 sum X / n) over its n visible anchor
//                  key points (score > kpt_thr), and like 'box' when none is visible; 'box' the bottom centre
//                  (X1 + X2, 2 Y2); 'centre' (X1 + X2, Y1 + Y2)
// A slot index that leaves find_slot or commit_births is a loop counter below S, or negative.
//
// The functions hold no barrier: the kernel places one between the steps that write LDS and those that read it, where
// it can be seen to be block-uniform.  The LDS arrays are the kernel's own and come in as pointers; the plan types
// share no prefix, only field names, so the functions that read a plan are templates over it.
#ifndef PAVE_TRACKED_H
#define PAVE_TRACKED_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"

namespace pave_tracked {

constexpr int QMAX = 32767;        // the largest quarter-pixel coordinate
constexpr int NEEDS_BIRTH = -2;    // find_slot: the pose takes part and its id has no slot yet

// A coordinate in quarter pixels (the clamp in float is defined for an infinite quotient).
__device__ __forceinline__ int quant(const float x, const float s) {
#pragma clang fp contract(off)
  const float q = __fdiv_rn(x, s);
  const float v = q * 4.f;
  return (int)fminf(fmaxf(rintf(v), 0.f), (float)QMAX);
}

// floor(a / b) for b > 0 (C's / truncates)
__device__ __forceinline__ long long floor_div(const long long a, const long long b) {
  const long long q = a / b;
  return q - ((a % b) < 0 ? 1 : 0);
}

// Block-uniform, before any barrier: false iff an earlier block has this camera.
template <class Plan>
__device__ __forceinline__ bool owns_camera(const Plan& plan, const int b, const int cam) {
  for (int e = 0; e < b; ++e)
    if (plan.camera[e] == cam) return false;
  return true;
}

// Returns the id slot t held if it expires in this frame (the caller may still read its other fields), else 0.
template <class Plan>
__device__ __forceinline__ int expire_slot(const Plan& plan, int32_t* g_id, const int32_t* g_last, int* slot_id,
                                           const int t, const int S, const int frame) {
  int id = 0, expired = 0;
  if (t < S) {
    id = g_id[t];
    if (id != 0 && (long long)frame - g_last[t] > plan.max_age) {
      expired = id;
      id = 0;
      g_id[t] = 0;
    }
  }
  slot_id[t] = id;
  return expired;
}

__device__ __forceinline__ int classify_pose(const float* bboxes, const int32_t* keep, const int32_t* ids,
                                             const float sx, const float sy, const float score_thr, const int d,
                                             int* det_id, int* det_bad, int* det_ok, int* det_born, int& X1, int& Y1,
                                             int& X2, int& Y2) {
  const float* bb = bboxes + d * 5;
  const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
  X1 = quant(b0, sx), Y1 = quant(b1, sy), X2 = quant(b2, sx), Y2 = quant(b3, sy);
  const int bad = isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3) ? 0 : 1;
  det_bad[d] = bad;
  det_ok[d] = (keep == nullptr || keep[d] != 0) && bb[4] > score_thr ? 1 : 0;
  det_id[d] = ids[d];
  det_born[d] = 0;
  return bad;
}

template <int NT>
__device__ __forceinline__ void sweep_finite(const float* kpts, const int n, const int K, const int tid,
                                             int* det_bad) {
  for (int i = tid; i < n * K; i += NT) {
    const float x = kpts[3 * i], y = kpts[3 * i + 1];
    if (!(isfinite(x) && isfinite(y))) atomicOr(&det_bad[i / K], 1);
  }
}

// det_bad: null where det_ok already implies "not bad" (floor_update_kernel's "placed").
__device__ __forceinline__ int find_slot(const int* det_id, const int* det_ok, const int* det_bad, const int* slot_id,
                                         const int d, const int S) {
  const int id = det_id[d];
  int slot = -1;
  if (det_ok[d] != 0 && (det_bad == nullptr || det_bad[d] == 0) && id >= 1) {
    bool first = true;
    for (int p = 0; p < d; ++p)
      first = first && !(det_id[p] == id && det_ok[p] != 0 && (det_bad == nullptr || det_bad[p] == 0));
    if (first) {
      slot = NEEDS_BIRTH;
      for (int t = S - 1; t >= 0; --t) slot = slot_id[t] == id ? t : slot;   // (the lowest, were there two)
    }
  }
  return slot;
}

// any: false when the caller knows that no pose of the frame has NEEDS_BIRTH; the scan is then skipped.
template <class Plan>
__device__ __forceinline__ void commit_births(const Plan& plan, const int cam, const int n, const int S,
                                              const int frame, const bool any, int32_t* g_id, int* slot_id,
                                              const int* det_id, int* det_slot, int* det_born, int* cam_state) {
  int free_t = 0, dropped = cam_state[1];
  for (int d = 0; any && d < n; ++d) {
    if (det_slot[d] != NEEDS_BIRTH) continue;
    while (free_t < S && slot_id[free_t] != 0) ++free_t;
    if (free_t < S) {
      slot_id[free_t] = det_id[d];
      g_id[free_t] = det_id[d];
      det_slot[d] = free_t;
      det_born[d] = 1;
    } else {
      det_slot[d] = -1;
      dropped = (int)((unsigned)dropped + 1u);
    }
  }
  cam_state[0] = frame;
  cam_state[1] = dropped;
  plan.frame[cam] = frame;
  plan.dropped[cam] = dropped;
}

template <class Plan>
__device__ __forceinline__ void anchor(const Plan& plan, const float* kpts, const int d, const int K,
                                       const float sx, const float sy, const int X1, const int Y1, const int X2,
                                       const int Y2, long long& ax, long long& ay) {
  ax = (long long)X1 + X2, ay = 2ll * Y2;   // the bottom centre of the box
  if (plan.anchor == PAVE_ZONE_ANCHOR_CENTRE) ay = (long long)Y1 + Y2;
  if (plan.anchor == PAVE_ZONE_ANCHOR_FEET) {
    long long sum_x = 0, sum_y = 0, seen = 0;
    for (int i = 0; i < plan.n_anchor; ++i) {
      const float* kp = kpts + 3 * (d * K + plan.anchor_kpt[i]);
      if (kp[2] > plan.kpt_thr) {
        sum_x += quant(kp[0], sx);
        sum_y += quant(kp[1], sy);
        ++seen;
      }
    }
    if (seen > 0) {   // (sums >= 0: / is floor)
      ax = 2 * sum_x / seen;
      ay = 2 * sum_y / seen;
    }
  }
}

}  // namespace pave_tracked

#endif  // PAVE_TRACKED_H
