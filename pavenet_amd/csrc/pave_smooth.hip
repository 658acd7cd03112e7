// Steady poses for the live path: a per-track adaptive exponential filter on the key points and the box corners of
// tracked poses, on the device, in one launch for up to 32 frames of any number of cameras (pave_smooth_poses).
//
// The rule is DESIGN section 16 and is integer-exact.  Quarter pixels X, the slots and who is filtered (who "takes
// part") are pave_tracked.h's; a state position is Z = 16 X, 1/64 pixel.  A pose has J = K + 2 points: its key points
// (visible iff their score is > kpt_thr), then its box corners (always visible).  A slot holds (id, last, pos [J, 2],
// vel [J, 2]); a point with pos x < 0 is uninitialised; a pose is unusable iff a coordinate is not finite.  A point of
// a filtered pose in a slot that was there before, visible and initialised, per axis in int64 with gap = frame - last
// and g = velocity_gain:
//   e = Z - pos;   r = floor((2 e + gap) / (2 gap));   vel = (g r + (16 - g) vel + 8) >> 4
// then with s = max(|X2 - X1|, |Y2 - Y1|, 1) of the pose's box
//   u = ((|vel_x| + |vel_y|) << 6) / s;   alpha = min(256, alpha_min + ((beta u) >> 4))
//   pos = clamp(pos + ((alpha e + 128) >> 8), 0, 524272)
// a visible point of a born slot, or an uninitialised one, takes pos = Z, vel = 0; an invisible one pos x = -1.
// Out goes pos / 64 of a filtered pose (Z / 64 where the point is not initialised), Z / 64 of any other usable pose,
// the quiet NaN of an unusable one, and the scores as they came.
//
// One block of 256 threads per camera of the launch (pave_tracked.h).  Its own: slot_last is kept in LDS as the frame
// before left it, since the gap is read after `last` is stored, and det_size is s of the pose's box.  After the births
// the N J points are spread over the block: each reads its pos / vel pair from global memory, filters it and stores
// it.  No two poses of a frame share a slot, so no two threads share a point.  Every loop bound is from the plan,
// every barrier is block-uniform, there are no global atomics and no scratch area.
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
constexpr long long PMAX = 16 * QMAX;                // the largest state position
constexpr unsigned int QUIET_NAN = 0x7fc00000u;

__device__ __forceinline__ long long abs64(const long long v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(NT) void smooth_poses_kernel(const pave_smooth_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int slot_last[MAXS];    // as the frame before left it
  __shared__ int det_id[MAXP];
  __shared__ int det_bad[MAXP];      // != 0: a coordinate that is not finite
  __shared__ int det_ok[MAXP];       // != 0: keep and a box score above the threshold
  __shared__ int det_slot[MAXP];     // the slot of a filtered pose, or -1
  __shared__ int det_born[MAXP];     // != 0: the slot was born in this frame
  __shared__ int det_size[MAXP];     // s of the pose's box
  __shared__ int cam_state[2];       // frame, dropped

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S, K = plan.K, J = K + 2;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_pos = plan.slot_pos + (long long)cam * S * J * 2;
  int32_t* __restrict__ g_vel = plan.slot_vel + (long long)cam * S * J * 2;
  const long long gain = plan.velocity_gain, alpha_min = plan.alpha_min, beta = plan.beta;

  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.dropped[cam];
  }

  for (int e = b; e < plan.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; cam_state is written
    const int n = plan.n[e];
    const float sx = plan.scale[e][0], sy = plan.scale[e][1];
    const float* __restrict__ kpts = plan.kpts[e];
    const float* __restrict__ bboxes = plan.bboxes[e];
    const int32_t* __restrict__ keep = plan.keep[e];
    const int32_t* __restrict__ ids = plan.ids[e];
    float* __restrict__ out_kpts = plan.out_kpts[e];
    float* __restrict__ out_bboxes = plan.out_bboxes[e];
    const int frame = (int)((unsigned)cam_state[0] + 1u);

    // ---- 1, 2: expire the slots; the poses' boxes ----
    if (tid < S) {
      const int last = g_last[tid];   // (read beside the id, not behind it: expire_slot's own read folds into this one)
      expire_slot(plan, g_id, g_last, slot_id, tid, S, frame);
      slot_last[tid] = last;
    }
    if (tid < n) {
      int X1, Y1, X2, Y2;
      classify_pose(bboxes, keep, ids, sx, sy, plan.score_thr, tid, det_id, det_bad, det_ok, det_born, X1, Y1, X2, Y2);
      det_size[tid] = max(max(abs(X2 - X1), abs(Y2 - Y1)), 1);
    }
    __syncthreads();
    sweep_finite<NT>(kpts, n, K, tid, det_bad);
    __syncthreads();

    // ---- 3: the slot of every pose ----
    if (tid < n) det_slot[tid] = find_slot(det_id, det_ok, det_bad, slot_id, tid, S);
    __syncthreads();
    if (tid == 0)   // births, in ascending pose index into the lowest free slot; the clock
      commit_births(plan, cam, n, S, frame, true, g_id, slot_id, det_id, det_slot, det_born, cam_state);
    __syncthreads();

    // ---- 4, 5, 6: the points ----
    if (tid < n && det_slot[tid] >= 0) g_last[det_slot[tid]] = frame;   // (gap is read from slot_last)
    for (int i = tid; i < n * J; i += NT) {
      const int d = i / J, j = i - d * J;
      float x, y;
      bool seen = true;
      if (j < K) {
        const float* kp = kpts + 3 * (d * K + j);
        x = kp[0];
        y = kp[1];
        seen = kp[2] > plan.kpt_thr;
      } else {
        x = bboxes[d * 5 + 2 * (j - K)];
        y = bboxes[d * 5 + 2 * (j - K) + 1];
      }
      const int Zx = 16 * quant(x, sx), Zy = 16 * quant(y, sy);
      int Qx = Zx, Qy = Zy;
      const int t = det_slot[d];
      if (t >= 0) {   // (in 0 .. S - 1: a slot index is a loop counter of step 3)
        int32_t* __restrict__ pos = g_pos + 2 * (t * J + j);
        int32_t* __restrict__ vel = g_vel + 2 * (t * J + j);
        const int px = pos[0];
        if (!seen) {
          pos[0] = -1;
        } else if (det_born[d] != 0 || px < 0) {
          pos[0] = Zx;
          pos[1] = Zy;
          vel[0] = 0;
          vel[1] = 0;
        } else {
          const long long py = pos[1];
          const long long gap = max((long long)frame - slot_last[t], 1ll);   // (>= 1 on a state of the rule's own)
          const long long ex = (long long)Zx - px, ey = (long long)Zy - py;
          const long long rx = floor_div(2 * ex + gap, 2 * gap), ry = floor_div(2 * ey + gap, 2 * gap);
          const long long vx = (gain * rx + (16 - gain) * (long long)vel[0] + 8) >> 4;
          const long long vy = (gain * ry + (16 - gain) * (long long)vel[1] + 8) >> 4;
          const long long u = ((abs64(vx) + abs64(vy)) << 6) / (long long)det_size[d];
          const long long alpha = min(256ll, alpha_min + ((beta * u) >> 4));
          Qx = (int)min(max(px + ((alpha * ex + 128) >> 8), 0ll), PMAX);
          Qy = (int)min(max(py + ((alpha * ey + 128) >> 8), 0ll), PMAX);
          pos[0] = Qx;
          pos[1] = Qy;
          vel[0] = (int32_t)(uint32_t)(unsigned long long)vx;   // (an int32 store keeps the low word)
          vel[1] = (int32_t)(uint32_t)(unsigned long long)vy;
        }
      }
      const bool bad = det_bad[d] != 0;
      const unsigned int ox = bad ? QUIET_NAN : __float_as_uint((float)Qx / 64.f);
      const unsigned int oy = bad ? QUIET_NAN : __float_as_uint((float)Qy / 64.f);
      if (j < K) {
        unsigned int* o = reinterpret_cast<unsigned int*>(out_kpts) + 3 * (d * K + j);
        o[0] = ox;
        o[1] = oy;
        o[2] = reinterpret_cast<const unsigned int*>(kpts)[3 * (d * K + j) + 2];
      } else {
        unsigned int* o = reinterpret_cast<unsigned int*>(out_bboxes) + d * 5;
        o[2 * (j - K)] = ox;
        o[2 * (j - K) + 1] = oy;
        if (j == K) o[4] = reinterpret_cast<const unsigned int*>(bboxes)[d * 5 + 4];
      }
    }
  }
}

}  // namespace

extern "C" {

int pave_smooth_poses(const pave_smooth_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "smooth_poses: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: K outside 1 .. 32");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "smooth_poses: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "smooth_poses: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_pos || !plan->slot_vel || !plan->frame || !plan->dropped)
    return pave_internal_fail(PAVE_E_ARG, "smooth_poses: null state tensor");
  if (plan->alpha_min < 1 || plan->alpha_min > 256)
    return pave_internal_fail(PAVE_E_ARG, "smooth_poses: alpha_min outside 1 .. 256");
  if (plan->beta < 0 || plan->beta > 4096) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: beta outside 0 .. 4096");
  if (plan->velocity_gain < 1 || plan->velocity_gain > 16)
    return pave_internal_fail(PAVE_E_ARG, "smooth_poses: velocity_gain outside 1 .. 16");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "smooth_poses: null ids tensor");
    if (n > 0 && (!plan->out_kpts[i] || !plan->out_bboxes[i]))
      return pave_internal_fail(PAVE_E_ARG, "smooth_poses: null output tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "smooth_poses: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "smooth_poses: scale must be positive and finite");
  }
  return pave_launch<smooth_poses_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                          reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
