// Track ids for the live path: the poses of a frame linked to the poses of the frames before it, on the device, in
// one launch for up to 32 frames of any number of cameras (pave_track_poses).
//
// The rule is DESIGN section 14 and is integer-exact.  A coordinate becomes quarter pixels as in section 13,
//   X = clamp((int)rintf((x / sx) * 4.f), 0, 32767)     (correctly rounded division, no contraction),
// a detection is valid iff keep[p] != 0 (when keep is given), its box score is > score_thr and its 2 K + 4
// coordinates are finite; key point k is visible iff its score > kpt_thr; area = max(X2 - X1, 1) max(Y2 - Y1, 1).
// For a valid detection d and a live slot t, over the key points visible in both, in int64:
//   d2_k = dx^2 + dy^2;   k agrees iff (d2_k << 20) <= C[k] (area_d + area_t);   s = agreeing points, D = sum d2_k,
// the pair is a candidate iff s >= min_kpts, and candidates are taken greedily by larger s, smaller D, smaller slot,
// smaller detection.  The four are packed into one 64-bit key
//   s << 51 | (2^37 - 1 - D) << 14 | (127 - slot) << 7 | (127 - det)        (0: not a candidate)
// so that the order is a plain unsigned maximum and the winner's indices are read back from the key itself.
//
// One block of 256 threads per camera of the launch: block b works iff entry b is the first entry of its camera, and
// then takes that camera's entries in plan order (frame f + 1 reads the state frame f stored, through the same
// block).  No two blocks touch one camera's state.  Per frame: expire, quantise detections and live slots into LDS
// (x | y << 16, rows of 33 words), one key per (detection, slot) into the block's 128 KB of the scratch area
// (L2-resident), the best remaining key of every detection row (thread d keeps row d's), then the greedy rounds: a
// block-wide maximum over the row bests, after which only the rows whose best slot was just taken (found by a
// ballot) are reduced again, one wave per row.  Births are a serial scan by one lane; the stores are made by all.
// Every loop bound is from the plan, the exit of the greedy loop and every barrier are block-uniform, there are no
// global atomics and nothing waits on memory.
//
// With the motion model (pave_track_poses_motion; DESIGN section 14, "Motion") the same kernel, MOTION = true: a live
// slot goes into LDS where it is predicted to be, kpts + ((vel min(gap, max_predict) + 8) >> 4) clamped, with the
// factor of its agreement test beside it (new_gate while hits == 1), and after the greedy rounds thread t measures
// the velocity of matched slot t from the points the slot still holds in global memory -- a phase of its own, behind
// a barrier and two barriers before the stores that overwrite those points.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using pave_tracked::QMAX;
using pave_tracked::quant;
using pave_tracked::floor_div;

constexpr int NT = 256;                              // threads of a block
constexpr int WAVES = NT / 64;
constexpr int MAXP = PAVE_TRACK_MAX_POSES;
constexpr int MAXT = PAVE_TRACK_MAX_TRACKS;
constexpr int ROW = PAVE_TRACK_MAX_K + 1;            // words of a row of packed points (odd: no bank conflicts)
constexpr long long DMAX = (1ll << 37) - 1;

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

template <bool MOTION>
struct track_arg {
  typedef pave_track_plan type;
};
template <>
struct track_arg<true> {
  typedef pave_track_motion_plan type;
};
__device__ __forceinline__ const pave_track_plan& base_of(const pave_track_plan& p) { return p; }
__device__ __forceinline__ const pave_track_plan& base_of(const pave_track_motion_plan& p) { return p.base; }

template <bool MOTION>
__global__ __launch_bounds__(NT) void track_poses_kernel(const typename track_arg<MOTION>::type arg) {
  const pave_track_plan& plan = base_of(arg);
  __shared__ unsigned int det_xy[MAXP * ROW], trk_xy[MAXT * ROW];
  __shared__ unsigned int det_vis[MAXP], trk_vis[MAXT];
  __shared__ int det_area[MAXP], trk_area[MAXT];
  __shared__ int det_bad[MAXP];      // != 0: not a valid detection
  __shared__ int det_slot[MAXP];     // the slot this frame gave the detection, or -1
  __shared__ int trk_id[MAXT];       // 0: free
  __shared__ int trk_det[MAXT];      // the detection this frame gave the slot, or -1
  __shared__ u64 row_best[MAXP];     // the largest key of the row among the slots not yet taken
  __shared__ u64 wave_best[WAVES], lost_rows[WAVES];
  __shared__ int cam_state[3];       // frame, next_id, dropped
  // MOTION: the predicted shift of a live slot (quarter pixels, within +-32767) and the factor on C[k] of its test
  __shared__ int trk_shift[MOTION ? MAXT : 1][2], trk_gate[MOTION ? MAXT : 1];

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  for (int e = 0; e < b; ++e)
    if (plan.camera[e] == cam) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = plan.M, K = plan.K;
  int32_t* __restrict__ g_id = plan.track_id + (long long)cam * M;
  int32_t* __restrict__ g_last = plan.track_last + (long long)cam * M;
  int32_t* __restrict__ g_kpts = plan.track_kpts + (long long)cam * M * K * 2;
  uint32_t* __restrict__ g_vis = plan.track_vis + (long long)cam * M;
  int32_t* __restrict__ g_area = plan.track_area + (long long)cam * M;
  u64* __restrict__ keys = reinterpret_cast<u64*>(plan.scratch) + (long long)b * MAXP * MAXT;
  int32_t* __restrict__ g_vel = nullptr;
  int32_t* __restrict__ g_hits = nullptr;
  if constexpr (MOTION) {
    g_vel = arg.track_vel + (long long)cam * M * 2;
    g_hits = arg.track_hits + (long long)cam * M;
  }

  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.next_id[cam];
    cam_state[2] = plan.dropped[cam];
  }

  for (int e = b; e < plan.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; cam_state is written
    const int n = plan.n[e];
    const float sx = plan.scale[e][0], sy = plan.scale[e][1];
    const float* __restrict__ kpts = plan.kpts[e];
    const float* __restrict__ bboxes = plan.bboxes[e];
    const int32_t* __restrict__ keep = plan.keep[e];
    const int frame = cam_state[0] + 1;
    int my_gap = 1, my_hits = 1, my_vx = 0, my_vy = 0;   // MOTION: slot tid as the frame before left it

    // ---- 1, 2: expire the slots; the detections' validity and area ----
    if (tid < M) {
      int id = g_id[tid];
      if (id != 0 && frame - g_last[tid] > plan.max_age) {
        id = 0;
        g_id[tid] = 0;
      }
      trk_id[tid] = id;
      trk_det[tid] = -1;
      trk_vis[tid] = g_vis[tid];
      trk_area[tid] = g_area[tid];
      if constexpr (MOTION) {
        if (id != 0) {
          // ---- 3b: where the slot is predicted to be ----
          my_gap = frame - g_last[tid];
          my_hits = g_hits[tid];
          my_vx = g_vel[2 * tid];
          my_vy = g_vel[2 * tid + 1];
          const long long g = min(my_gap, arg.max_predict);
          const long long shx = ((long long)my_vx * g + 8) >> 4, shy = ((long long)my_vy * g + 8) >> 4;
          // (a stored point is within 0 .. 32767: a shift beyond +-32767 clamps to the same end)
          trk_shift[tid][0] = (int)min(max(shx, (long long)-QMAX), (long long)QMAX);
          trk_shift[tid][1] = (int)min(max(shy, (long long)-QMAX), (long long)QMAX);
          trk_gate[tid] = my_hits == 1 ? arg.new_gate : 1;
        }
      }
    }
    if (tid < n) {
      const float* bb = bboxes + tid * 5;
      const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
      const bool ok = (keep == nullptr || keep[tid] != 0) && bb[4] > plan.score_thr && isfinite(b0) && isfinite(b1) &&
                      isfinite(b2) && isfinite(b3);
      const int X1 = quant(b0, sx), Y1 = quant(b1, sy), X2 = quant(b2, sx), Y2 = quant(b3, sy);
      det_area[tid] = max(X2 - X1, 1) * max(Y2 - Y1, 1);
      det_bad[tid] = ok ? 0 : 1;
      det_vis[tid] = 0u;
      det_slot[tid] = -1;
    }
    __syncthreads();

    // ---- 3: quantise into LDS ----
    for (int i = tid; i < n * K; i += NT) {
      const int d = i / K, k = i - d * K;
      const float x = kpts[3 * i], y = kpts[3 * i + 1], sc = kpts[3 * i + 2];
      if (!(isfinite(x) && isfinite(y))) atomicOr(&det_bad[d], 1);
      if (sc > plan.kpt_thr) atomicOr(&det_vis[d], 1u << k);
      det_xy[d * ROW + k] = (unsigned)quant(x, sx) | ((unsigned)quant(y, sy) << 16);
    }
    for (int i = tid; i < M * K; i += NT) {
      const int t = i / K, k = i - t * K;
      if (trk_id[t] != 0) {
        if constexpr (MOTION) {
          const int px = min(max((int)((unsigned)g_kpts[2 * i] & QMAX) + trk_shift[t][0], 0), QMAX);
          const int py = min(max((int)((unsigned)g_kpts[2 * i + 1] & QMAX) + trk_shift[t][1], 0), QMAX);
          trk_xy[t * ROW + k] = (unsigned)px | ((unsigned)py << 16);
        } else {
          trk_xy[t * ROW + k] = ((unsigned)g_kpts[2 * i] & QMAX) | (((unsigned)g_kpts[2 * i + 1] & QMAX) << 16);
        }
      }
    }
    __syncthreads();

    // ---- 4: one key per (detection, slot) ----
    for (int p = tid; p < n * M; p += NT) {
      const int d = p / M, t = p - d * M;
      u64 key = 0;
      if (det_bad[d] == 0 && trk_id[t] != 0) {
        const unsigned both = det_vis[d] & trk_vis[t];
        long long area = (long long)det_area[d] + (long long)trk_area[t];
        if constexpr (MOTION) area *= trk_gate[t];   // (C[k] G (area_d + area_t) < 2^24 16 2^31)
        int s = 0;
        long long D = 0;
        for (int k = 0; k < K; ++k) {
          if (both >> k & 1u) {
            const unsigned a = det_xy[d * ROW + k], c = trk_xy[t * ROW + k];
            const int dx = (int)(a & 0xffffu) - (int)(c & 0xffffu), dy = (int)(a >> 16) - (int)(c >> 16);
            const long long d2 = (long long)(dx * dx) + (long long)(dy * dy);
            D += d2;
            s += (d2 << 20) <= (long long)plan.C[k] * area ? 1 : 0;
          }
        }
        if (s >= plan.min_kpts)
          key = (u64)s << 51 | (u64)(DMAX - D) << 14 | (u64)(MAXT - 1 - t) << 7 | (u64)(MAXP - 1 - d);
      }
      keys[d * MAXT + t] = key;
    }
    __syncthreads();

    // ---- 5: the best key of every row, then the greedy rounds ----
    for (int d = wave; d < n; d += WAVES) {
      u64 v = lane < M ? keys[d * MAXT + lane] : 0;
      const u64 w = lane + 64 < M ? keys[d * MAXT + lane + 64] : 0;
      v = wave_max(w > v ? w : v);
      if (lane == 0) row_best[d] = v;
    }
    __syncthreads();
    const int rounds = min(n, M);
    u64 rb = tid < n ? row_best[tid] : 0;   // thread d keeps row d's best (n <= 128: waves 0 and 1)
    for (int r = 0; r < rounds; ++r) {
      const u64 mine = wave_max(rb);
      if (lane == 0) wave_best[wave] = mine;
      __syncthreads();
      const u64 best = wave_best[0] > wave_best[1] ? wave_best[0] : wave_best[1];
      if (best == 0) break;   // (block-uniform: every lane read the same two words)
      const int bt = MAXT - 1 - (int)(best >> 7 & 127u), bd = MAXP - 1 - (int)(best & 127u);
      if (tid == bd) rb = 0;   // the winner's row is done
      // the rows that lose their best slot
      const bool lost = rb != 0 && MAXT - 1 - (int)(rb >> 7 & 127u) == bt;
      const u64 mask = __ballot(lost);
      if (lane == 0) lost_rows[wave] = mask;
      if (tid == 0) {
        det_slot[bd] = bt;
        trk_det[bt] = bd;
      }
      __syncthreads();
      const u64 m0 = lost_rows[0], m1 = lost_rows[1];
      if ((m0 | m1) == 0) continue;   // (block-uniform)
      // one wave per lost row: the largest key among the slots not yet taken (bt is among the taken)
      int j = 0;
      for (int half = 0; half < 2; ++half) {
        for (u64 mm = half ? m1 : m0; mm != 0; mm &= mm - 1, ++j) {
          if ((j & (WAVES - 1)) != wave) continue;   // (wave-uniform)
          const int d = half * 64 + __builtin_ctzll(mm);
          u64 v = (lane < M && trk_det[lane] < 0) ? keys[d * MAXT + lane] : 0;
          const u64 w = (lane + 64 < M && trk_det[lane + 64] < 0) ? keys[d * MAXT + lane + 64] : 0;
          v = wave_max(w > v ? w : v);
          if (lane == 0) row_best[d] = v;
        }
      }
      __syncthreads();
      if (lost) rb = row_best[tid];
    }
    __syncthreads();

    // ---- 6': the velocity of a matched slot, from the points it still holds (the stores below overwrite them) ----
    bool matched = false;
    if constexpr (MOTION) {
      const int d = tid < M ? trk_det[tid] : -1;   // (no birth yet: >= 0 is a match of step 5)
      if (d >= 0) {
        matched = true;
        const unsigned cov = det_vis[d] & trk_vis[tid];
        const long long cnt = __popc(cov);
        long long Sx = 0, Sy = 0;
        for (int k = 0; k < K; ++k) {
          if (cov >> k & 1u) {
            const unsigned a = det_xy[d * ROW + k];
            Sx += (int)(a & 0xffffu) - g_kpts[2 * (tid * K + k)];
            Sy += (int)(a >> 16) - g_kpts[2 * (tid * K + k) + 1];
          }
        }
        const long long ng = cnt * (long long)my_gap;
        if (ng > 0) {   // (a candidate has n >= min_kpts >= 1 and a live slot gap >= 1)
          const long long mx = floor_div(32 * Sx + ng, 2 * ng), my = floor_div(32 * Sy + ng, 2 * ng);
          const long long gn = arg.gain;
          const long long vx = my_hits == 1 ? mx : (gn * mx + (16 - gn) * (long long)my_vx + 8) >> 4;
          const long long vy = my_hits == 1 ? my : (gn * my + (16 - gn) * (long long)my_vy + 8) >> 4;
          my_vx = (int)min(max(vx, -32768ll), 32767ll);
          my_vy = (int)min(max(vy, -32768ll), 32767ll);
        }
        my_hits = my_hits >= 32767 ? 32767 : my_hits + 1;
      }
      __syncthreads();   // the births below write trk_det
    }

    // ---- 7: births, in ascending detection index into the lowest free slot ----
    if (tid == 0) {
      int free_t = 0, next_id = cam_state[1], dropped = cam_state[2];
      for (int d = 0; d < n; ++d) {
        if (det_bad[d] != 0 || det_slot[d] >= 0) continue;
        while (free_t < M && trk_id[free_t] != 0) ++free_t;
        if (free_t < M) {
          trk_id[free_t] = next_id++;
          trk_det[free_t] = d;
          det_slot[d] = free_t;
        } else {
          ++dropped;
        }
      }
      cam_state[0] = frame;
      cam_state[1] = next_id;
      cam_state[2] = dropped;
      plan.frame[cam] = frame;
      plan.next_id[cam] = next_id;
      plan.dropped[cam] = dropped;
    }
    __syncthreads();

    // ---- 6, 8: the stores ----
    if (tid < n) {
      const int t = det_slot[tid];
      plan.ids[e][tid] = t >= 0 ? trk_id[t] : 0;
    }
    if (tid < M) {
      const int d = trk_det[tid];
      if (d >= 0) {
        g_id[tid] = trk_id[tid];
        g_last[tid] = frame;
        g_vis[tid] = det_vis[d];
        g_area[tid] = det_area[d];
        if constexpr (MOTION) {   // 7': a birth starts at rest
          g_vel[2 * tid] = matched ? my_vx : 0;
          g_vel[2 * tid + 1] = matched ? my_vy : 0;
          g_hits[tid] = matched ? my_hits : 1;
        }
      }
    }
    for (int i = tid; i < M * K; i += NT) {
      const int t = i / K, k = i - t * K;
      const int d = trk_det[t];
      if (d >= 0) {
        const unsigned a = det_xy[d * ROW + k];
        g_kpts[2 * i] = (int)(a & 0xffffu);
        g_kpts[2 * i + 1] = (int)(a >> 16);
      }
    }
  }
}

// Everything a plan could get wrong, before any device call.
int track_check(const pave_track_plan* plan) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "track_poses: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "track_poses: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "track_poses: K outside 1 .. 32");
  if (plan->M < 1 || plan->M > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "track_poses: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "track_poses: cameras outside 1 .. 4096");
  if (!plan->track_id || !plan->track_last || !plan->track_kpts || !plan->track_vis || !plan->track_area ||
      !plan->frame || !plan->next_id || !plan->dropped)
    return pave_internal_fail(PAVE_E_ARG, "track_poses: null state tensor");
  if (!plan->scratch) return pave_internal_fail(PAVE_E_ARG, "track_poses: null scratch area");
  if (plan->min_kpts < 1 || plan->min_kpts > plan->K)
    return pave_internal_fail(PAVE_E_ARG, "track_poses: min_kpts outside 1 .. K");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "track_poses: max_age below 0");
  for (int k = 0; k < plan->K; ++k)
    if (plan->C[k] < 1 || plan->C[k] >= (1 << 24))
      return pave_internal_fail(PAVE_E_ARG, "track_poses: a pair constant C[k] outside [1, 2^24)");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "track_poses: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "track_poses: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "track_poses: null ids tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "track_poses: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "track_poses: scale must be positive and finite");
  }
  return PAVE_OK;
}

}  // namespace

extern "C" {

int pave_track_poses(const pave_track_plan* plan, void* stream) {
  const int st = track_check(plan);
  if (st != PAVE_OK) return st;
  return pave_launch<track_poses_kernel<false>>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                                reinterpret_cast<hipStream_t>(stream), *plan);
}

int pave_track_poses_motion(const pave_track_motion_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "track_poses_motion: null plan");
  const int st = track_check(&plan->base);
  if (st != PAVE_OK) return st;
  if (!plan->track_vel || !plan->track_hits)
    return pave_internal_fail(PAVE_E_ARG, "track_poses_motion: null velocity or hits tensor");
  if (plan->gain < 1 || plan->gain > 16) return pave_internal_fail(PAVE_E_ARG, "track_poses_motion: gain outside 1 .. 16");
  if (plan->max_predict < 0 || plan->max_predict > 255)
    return pave_internal_fail(PAVE_E_ARG, "track_poses_motion: max_predict outside 0 .. 255");
  if (plan->new_gate < 1 || plan->new_gate > 16)
    return pave_internal_fail(PAVE_E_ARG, "track_poses_motion: new_gate outside 1 .. 16");
  return pave_launch<track_poses_kernel<true>>(dim3((unsigned)plan->base.entries), dim3(NT), 0,
                                               reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
