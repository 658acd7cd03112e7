// Postures and falls for the live path: the class of every tracked pose from its trunk and legs (UPRIGHT, LOW, LEANING,
// LYING), debounced per track id, and the events that follow from it -- a posture change, a fall, a person who stays
// down, hands that go up or down -- on the device, in one launch for up to 32 frames of any number of cameras
// (pave_posture_events).
//
// The rule is DESIGN section 20 and is integer-exact.  Quarter pixels X, who takes part and the slots are
// pave_tracked.h's; everything after that is in 1/8 pixel: the centre of a part (shoulders, hips, ankles, wrists; at
// most 4 key points each) is floor(2 sum X / n) over its n visible key points, as the zones' anchor.  With (dx, dy) =
// hips - shoulders and all products in int64 the raw class of a frame is
//   UNKNOWN   no shoulder or no hip visible, or dx = dy = 0
//   LYING     16 |dy| <= flat |dx|                                  (tested first)
//   UPRIGHT   dy > 0 and 16 |dx| <= lean dy;  LOW instead iff squat > 0, an ankle is visible and
//             16 (ankles.y - hips.y) < squat dy
//   LEANING   everything else
// and wrist i sets bit i of the raw hands iff it is visible, hand_up is on, the class is UPRIGHT or LOW and
// 16 (shoulders.y - 2 Y) >= hand_up dy.
// A camera keeps S slots of (id, last, posture, since, upright, streak, alerted, hands, hand_streak), a clock, a drop
// count and 8 counters.  Per frame: the clock advances; a slot not seen for more than max_age frames is freed; poses
// find or take slots; a born slot takes the raw class and the raw hand bit without an event; a slot that was there
// follows the raw class once it has disagreed with the posture min_frames frames in a row (POSTURE, and FALL when the
// new posture is LYING within fall_window frames of the last UPRIGHT one), reports DOWN once per stay when frame -
// since >= down_frames, and debounces "any hand raised" the same way (HANDS_UP / HANDS_DOWN).  A raw UNKNOWN changes
// neither streak.  Events are rows (kind, index, id, pose, frame), per pose in ascending index POSTURE, FALL, DOWN,
// then the hands event.
//
// One block of 128 threads per camera of the launch (pave_tracked.h).  Its own (DESIGN section 20 has the
// measurements): thread d tests the finiteness of pose d's key points itself, eight at a time, where the other kernels
// sweep them with the whole block, and a block-wide vote skips the birth scan in a frame without a birth (the clock
// and the drop count are stored all the same).  After the births thread d does the whole of pose d: at most 16 key
// points, the class, the slot's stores and the pose's outputs.  What a thread found stays in a bit mask, so its event
// count is a popcount; an exclusive scan of the 128 counts in LDS gives every thread the row of its first event,
// whatever order the threads run in.  What a thread's slot and pose add to the 8 counters it adds to 8 words in LDS
// (integer adds: any order gives the same sum), and threads 0 .. 7 carry them to the camera's counters.  Every loop
// bound is from the plan or the maxima of the header, part counts and indices are clamped as they are read, every
// barrier is block-uniform, there are no global atomics and no scratch area.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using namespace pave_tracked;

constexpr int NT = 128;                              // threads of a block
constexpr int MAXP = PAVE_TRACK_MAX_POSES;
constexpr int MAXS = PAVE_TRACK_MAX_TRACKS;
constexpr int NPART = PAVE_POSTURE_PARTS;
constexpr int MAXK = PAVE_POSTURE_MAX_PART;
constexpr int EW = PAVE_POSTURE_EVENT_WORDS;
constexpr int M_POSTURE = 1, M_FALL = 2, M_DOWN = 4, M_HANDS_UP = 8, M_HANDS_DOWN = 16;   // the event bits of a pose
static_assert(MAXP == NT && MAXS == NT, "one scan item, one pose and one slot per thread");
static_assert(PAVE_POSTURE_COUNTER_WORDS <= NT && PAVE_POSTURE_CNT_NOW == 0, "thread roles");

__device__ __forceinline__ long long absll(const long long v) { return v < 0 ? -v : v; }

__device__ __forceinline__ void put(int32_t* __restrict__ events, int& row, const int max_events, const int kind,
                                    const int index, const int id, const int pose, const int frame) {
  if (row < max_events) {
    int32_t* r = events + (long long)row * EW;
    r[0] = kind;
    r[1] = index;
    r[2] = id;
    r[3] = pose;
    r[4] = frame;
  }
  ++row;
}

__global__ __launch_bounds__(NT) void posture_events_kernel(const pave_posture_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int det_id[MAXP];
  __shared__ int det_bad[MAXP];      // != 0: a coordinate that is not finite
  __shared__ int det_ok[MAXP];       // != 0: keep and a box score above the threshold
  __shared__ int det_slot[MAXP];     // the slot of a pose that takes part, or -1
  __shared__ int det_born[MAXP];     // != 0: the slot was born in this frame
  __shared__ int count_delta[PAVE_POSTURE_COUNTER_WORDS];   // what this frame adds to the camera's counters
  __shared__ int scan[2][NT];
  __shared__ int cam_state[2];       // frame, dropped

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S, K = plan.K;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_posture = plan.slot_posture + (long long)cam * S;
  int32_t* __restrict__ g_since = plan.slot_since + (long long)cam * S;
  int32_t* __restrict__ g_upright = plan.slot_upright + (long long)cam * S;
  int32_t* __restrict__ g_streak = plan.slot_streak + (long long)cam * S;
  int32_t* __restrict__ g_alerted = plan.slot_alerted + (long long)cam * S;
  int32_t* __restrict__ g_hands = plan.slot_hands + (long long)cam * S;
  int32_t* __restrict__ g_hstreak = plan.slot_hand_streak + (long long)cam * S;
  int32_t* __restrict__ g_count = plan.counters + (long long)cam * PAVE_POSTURE_COUNTER_WORDS;

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
    int32_t* __restrict__ out_events = plan.out_events[e];
    const int max_events = plan.max_events;
    const int frame = (int)((unsigned)cam_state[0] + 1u);

    // ---- 1, 2: expire the slots; the poses' boxes ----
    int gone = -1, gone_hand = 0;   // the posture and the hand bit of slot tid if it expires in this frame
    if (expire_slot(plan, g_id, g_last, slot_id, tid, S, frame) != 0) {
      gone = g_posture[tid];
      gone_hand = g_hands[tid] != 0 ? 1 : 0;
    }
    if (tid < PAVE_POSTURE_COUNTER_WORDS) count_delta[tid] = 0;
    if (tid < n) {
      int X1, Y1, X2, Y2;   // (unused: a posture is made of key points)
      int bad = classify_pose(bboxes, keep, ids, sx, sy, plan.score_thr, tid, det_id, det_bad, det_ok, det_born, X1, Y1,
                              X2, Y2);
      const float* kp = kpts + 3 * (tid * K);
      for (int k0 = 0; k0 < K; k0 += 8) {   // eight key points at a time: sixteen loads that do not wait for each other
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = min(k0 + j, K - 1);   // (past the last one: the last one again)
          const float x = kp[3 * k], y = kp[3 * k + 1];
          bad |= isfinite(x) && isfinite(y) ? 0 : 1;
        }
      }
      det_bad[tid] = bad;
    }
    __syncthreads();

    // ---- 2: the slot of every pose ----
    int slot = -1;
    if (tid < n) det_slot[tid] = slot = find_slot(det_id, det_ok, det_bad, slot_id, tid, S);
    const int births = __syncthreads_or(slot == NEEDS_BIRTH ? 1 : 0);   // (block-uniform: every thread votes)
    if (tid == 0)   // births, in ascending pose index into the lowest free slot; the clock, whatever was born
      commit_births(plan, cam, n, S, frame, births != 0, g_id, slot_id, det_id, det_slot, det_born, cam_state);
    __syncthreads();

    // ---- 3 .. 7: pose tid in its slot ----
    int ev = 0, ev_class = 0, ev_fall = 0, ev_down = 0, ev_hands = 0;
    int old_class = -1, new_class = -1, hand_delta = 0;
    if (tid < n) {
      const int t = det_slot[tid];   // (in 0 .. S - 1 or -1: a slot index is a loop counter of step 2)
      int out_posture = -1, out_raw = -1, out_hands = 0, out_since = 0;
      if (t >= 0) {
        // the centres of the parts, 1/8 pixel; the wrists one by one, quarter pixels
        long long cx[NPART], cy[NPART];
        int seen[NPART], wrist_y[MAXK], wrist_seen = 0;
        float px[NPART][MAXK], py[NPART][MAXK], ps[NPART][MAXK];   // (constant indices of unrolled loops: registers)
#pragma unroll
        for (int p = 0; p < NPART; ++p) {   // all 48 loads first, so that none waits for another (unused: key point 0)
          const int np = min(max(plan.n_part[p], 0), MAXK);
#pragma unroll
          for (int i = 0; i < MAXK; ++i) {
            const int k = i < np ? min(max(plan.part[p][i], 0), K - 1) : 0;
            const float* kp = kpts + 3 * (tid * K + k);
            px[p][i] = kp[0];
            py[p][i] = kp[1];
            ps[p][i] = kp[2];
          }
        }
#pragma unroll
        for (int p = 0; p < NPART; ++p) {
          const int np = min(max(plan.n_part[p], 0), MAXK);
          int sum_x = 0, sum_y = 0, count = 0;   // (at most 4 * 32767)
#pragma unroll
          for (int i = 0; i < MAXK; ++i) {
            if (p == PAVE_POSTURE_PART_WRISTS) wrist_y[i] = 0;
            if (i < np && ps[p][i] > plan.kpt_thr) {
              const int X = quant(px[p][i], sx), Y = quant(py[p][i], sy);
              sum_x += X;
              sum_y += Y;
              ++count;
              if (p == PAVE_POSTURE_PART_WRISTS) {
                wrist_y[i] = Y;
                wrist_seen |= 1 << i;
              }
            }
          }
          seen[p] = count;
          cx[p] = count > 0 ? 2 * sum_x / count : 0;   // (sums >= 0: / is floor)
          cy[p] = count > 0 ? 2 * sum_y / count : 0;
        }
        const long long dx = cx[PAVE_POSTURE_PART_HIPS] - cx[PAVE_POSTURE_PART_SHOULDERS];
        const long long dy = cy[PAVE_POSTURE_PART_HIPS] - cy[PAVE_POSTURE_PART_SHOULDERS];
        int raw = PAVE_POSTURE_LEANING;
        if (seen[PAVE_POSTURE_PART_SHOULDERS] == 0 || seen[PAVE_POSTURE_PART_HIPS] == 0 || (dx == 0 && dy == 0)) {
          raw = PAVE_POSTURE_UNKNOWN;
        } else if (16 * absll(dy) <= (long long)plan.flat * absll(dx)) {
          raw = PAVE_POSTURE_LYING;
        } else if (dy > 0 && 16 * absll(dx) <= (long long)plan.lean * dy) {
          raw = PAVE_POSTURE_UPRIGHT;
          if (plan.squat > 0 && seen[PAVE_POSTURE_PART_ANKLES] > 0 &&
              16 * (cy[PAVE_POSTURE_PART_ANKLES] - cy[PAVE_POSTURE_PART_HIPS]) < (long long)plan.squat * dy)
            raw = PAVE_POSTURE_LOW;
        }
        int raw_hands = 0;
        if (plan.hand_up >= 0 && (raw == PAVE_POSTURE_UPRIGHT || raw == PAVE_POSTURE_LOW)) {
#pragma unroll
          for (int i = 0; i < MAXK; ++i)
            if (((wrist_seen >> i) & 1) &&
                16 * (cy[PAVE_POSTURE_PART_SHOULDERS] - 2ll * wrist_y[i]) >= (long long)plan.hand_up * dy)
              raw_hands |= 1 << i;
        }
        const int raw_bit = raw_hands != 0 ? 1 : 0;

        int posture, since, upright, streak, alerted, hands, hstreak;
        if (det_born[tid] != 0) {
          posture = raw;
          since = frame;
          upright = 0;
          streak = 0;
          alerted = 0;
          hands = raw_bit;
          hstreak = 0;
          new_class = raw;
          hand_delta = raw_bit;
        } else {
          posture = g_posture[t];
          since = g_since[t];
          upright = g_upright[t];
          streak = g_streak[t];
          alerted = g_alerted[t];
          hands = g_hands[t] != 0 ? 1 : 0;
          hstreak = g_hstreak[t];
          old_class = new_class = posture;
          if (raw != PAVE_POSTURE_UNKNOWN) {
            if (raw == posture) {
              streak = 0;
            } else if (++streak >= plan.min_frames) {
              posture = raw;
              streak = 0;
              since = frame;
              alerted = 0;
              new_class = raw;
              ev |= M_POSTURE;
              ev_class = raw;
              if (raw == PAVE_POSTURE_LYING && upright != 0 && (long long)frame - upright <= plan.fall_window) {
                ev |= M_FALL;
                ev_fall = (int)((unsigned)frame - (unsigned)upright);
              }
            }
            if (raw_bit == hands) {
              hstreak = 0;
            } else if (++hstreak >= plan.min_frames) {
              hands = raw_bit;
              hstreak = 0;
              hand_delta = raw_bit ? 1 : -1;
              ev |= raw_bit ? M_HANDS_UP : M_HANDS_DOWN;
              ev_hands = raw_hands;
            }
          }
          if (posture == PAVE_POSTURE_LYING && alerted == 0 && plan.down_frames > 0 &&
              (long long)frame - since >= plan.down_frames) {
            alerted = 1;
            ev |= M_DOWN;
            ev_down = (int)((unsigned)frame - (unsigned)since);
          }
        }
        if (posture == PAVE_POSTURE_UPRIGHT) upright = frame;
        g_last[t] = frame;
        g_posture[t] = posture;
        g_since[t] = since;
        g_upright[t] = upright;
        g_streak[t] = streak;
        g_alerted[t] = alerted;
        g_hands[t] = hands;
        g_hstreak[t] = hstreak;
        out_posture = posture;
        out_raw = raw;
        out_hands = raw_hands;
        out_since = (int)((unsigned)frame - (unsigned)since);
      }
      plan.out_posture[e][tid] = out_posture;
      plan.out_raw[e][tid] = out_raw;
      plan.out_hands[e][tid] = out_hands;
      plan.out_since[e][tid] = out_since;
    }
    // what slot tid (if it expired) and pose tid add to the counters; a class from the state indexes only inside now[5]
    if (gone >= 0 && gone < PAVE_POSTURE_CLASSES) atomicAdd(&count_delta[gone], -1);
    if (gone_hand != 0) atomicAdd(&count_delta[PAVE_POSTURE_CNT_HANDS_UP], -1);
    if (new_class != old_class) {
      if (old_class >= 0 && old_class < PAVE_POSTURE_CLASSES) atomicAdd(&count_delta[old_class], -1);
      if (new_class >= 0 && new_class < PAVE_POSTURE_CLASSES) atomicAdd(&count_delta[new_class], 1);
    }
    if (hand_delta != 0) atomicAdd(&count_delta[PAVE_POSTURE_CNT_HANDS_UP], hand_delta);
    if (ev & M_FALL) atomicAdd(&count_delta[PAVE_POSTURE_CNT_FALLS], 1);
    if (ev & M_DOWN) atomicAdd(&count_delta[PAVE_POSTURE_CNT_DOWNS], 1);
    scan[0][tid] = __popc(ev);
    __syncthreads();

    // ---- 8: the row of every thread's first event; the counters ----
    int buf = 0;
    for (int step = 1; step < NT; step <<= 1) {   // an inclusive scan of the 128 counts
      const int v = scan[buf][tid] + (tid >= step ? scan[buf][tid - step] : 0);
      scan[buf ^ 1][tid] = v;
      __syncthreads();
      buf ^= 1;
    }
    const int total = scan[buf][NT - 1];
    if (ev != 0) {
      int row = scan[buf][tid] - __popc(ev);
      const int id = det_id[tid];
      if (ev & M_POSTURE) put(out_events, row, max_events, PAVE_POSTURE_EV_POSTURE, ev_class, id, tid, frame);
      if (ev & M_FALL) put(out_events, row, max_events, PAVE_POSTURE_EV_FALL, ev_fall, id, tid, frame);
      if (ev & M_DOWN) put(out_events, row, max_events, PAVE_POSTURE_EV_DOWN, ev_down, id, tid, frame);
      if (ev & M_HANDS_UP) put(out_events, row, max_events, PAVE_POSTURE_EV_HANDS_UP, ev_hands, id, tid, frame);
      if (ev & M_HANDS_DOWN) put(out_events, row, max_events, PAVE_POSTURE_EV_HANDS_DOWN, ev_hands, id, tid, frame);
    }
    if (tid < PAVE_POSTURE_COUNTER_WORDS) {   // one counter per thread (the sums are complete: the scan's barriers)
      const int delta = count_delta[tid];
      if (delta != 0) g_count[tid] = (int)((unsigned)g_count[tid] + (unsigned)delta);
    }
    if (tid == 0) plan.out_n_events[e][0] = total;
    for (int i = min(total, max_events) * EW + tid; i < max_events * EW; i += NT) out_events[i] = 0;
  }
}

}  // namespace

extern "C" {

int pave_posture_events(const pave_posture_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "posture_events: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "posture_events: K outside 1 .. 32");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_posture || !plan->slot_since || !plan->slot_upright ||
      !plan->slot_streak || !plan->slot_alerted || !plan->slot_hands || !plan->slot_hand_streak || !plan->frame ||
      !plan->dropped || !plan->counters)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: null state tensor");
  if (plan->min_frames < 1 || plan->min_frames > 255)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: min_frames outside 1 .. 255");
  if (plan->max_events < 1 || plan->max_events > PAVE_POSTURE_MAX_EVENTS)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: max_events outside 1 .. 4096");
  if (plan->lean < 1 || plan->lean > PAVE_POSTURE_MAX_SLOPE)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: lean outside 1 .. 255");
  if (plan->flat < 1 || plan->flat > PAVE_POSTURE_MAX_SLOPE)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: flat outside 1 .. 255");
  if (plan->squat < 0 || plan->squat > PAVE_POSTURE_MAX_SLOPE)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: squat outside 0 .. 255");
  if (plan->hand_up < PAVE_POSTURE_HANDS_OFF || plan->hand_up > PAVE_POSTURE_MAX_SLOPE)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: hand_up outside -1 .. 255");
  if (plan->fall_window < 0 || plan->fall_window > PAVE_POSTURE_MAX_WAIT)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: fall_window outside 0 .. 2^30");
  if (plan->down_frames < 0 || plan->down_frames > PAVE_POSTURE_MAX_WAIT)
    return pave_internal_fail(PAVE_E_ARG, "posture_events: down_frames outside 0 .. 2^30");
  for (int p = 0; p < PAVE_POSTURE_PARTS; ++p) {
    if (plan->n_part[p] < 0 || plan->n_part[p] > PAVE_POSTURE_MAX_PART)
      return pave_internal_fail(PAVE_E_ARG, "posture_events: n_part outside 0 .. 4");
    for (int i = 0; i < plan->n_part[p]; ++i)
      if (plan->part[p][i] < 0 || plan->part[p][i] >= plan->K)
        return pave_internal_fail(PAVE_E_ARG, "posture_events: a part key point outside [0, K)");
  }
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "posture_events: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "posture_events: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i]))
      return pave_internal_fail(PAVE_E_ARG, "posture_events: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "posture_events: null ids tensor");
    if (n > 0 && (!plan->out_posture[i] || !plan->out_raw[i] || !plan->out_hands[i] || !plan->out_since[i]))
      return pave_internal_fail(PAVE_E_ARG, "posture_events: null output tensor");
    if (!plan->out_events[i] || !plan->out_n_events[i])
      return pave_internal_fail(PAVE_E_ARG, "posture_events: null events tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "posture_events: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "posture_events: scale must be positive and finite");
  }
  return pave_launch<posture_events_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                            reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
