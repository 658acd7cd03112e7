// Zones and counting lines for the live path: which tracks stand inside which polygon and for how long, and which
// directed line a track crossed, on the device, in one launch for up to 32 frames of any number of cameras
// (pave_zone_events).
//
// The rule is DESIGN section 17 and is integer-exact.  Who takes part, the slots and the anchor of a pose in 1/8
// pixel are pave_tracked.h's; the geometry is in 1/8 pixel too, at most 8 polygons of at most 16 vertices and 8
// directed lines per camera.  All products are int64.
//   inside(P, polygon): even-odd; an edge (a, b) with (a.y > P.y) != (b.y > P.y) toggles iff, with dy = b.y - a.y and
//     t = (P.x - a.x) dy - (P.y - a.y)(b.x - a.x), dy > 0 ? t < 0 : t > 0
//   s(P) on A -> B: cross(B - A, P - A) >= 0; a move Q -> P, Q != P, crosses iff s(Q) != s(P) and A and B are on
//     different sides of Q -> P by the same test; forward iff s(Q) is false
// A camera keeps S slots of (id, last, pos [2], inside, alerted, streak [8], since [8]), a clock, a drop count and 56
// counters.  Per frame: the clock advances; a slot not seen for more than max_age frames is freed (VANISH for every
// zone it was inside); poses find or take slots; a born slot takes the raw test as its inside bits (APPEAR); a slot
// that was there flips bit z once the raw test has disagreed with it min_frames frames in a row (ENTER / EXIT), is
// reported once per stay when frame - since >= dwell_frames (DWELL), and is tested against every line on its move pos
// -> anchor (CROSS_FWD / CROSS_BACK).  Events are rows (kind, index, id, pose, frame) in a fixed order: VANISH by slot
// then zone, then per pose in ascending index its zones (flip or APPEAR, then DWELL), then its lines.
//
// One block of 256 threads per camera of the launch (pave_tracked.h).  The camera's geometry goes into LDS once.  Per
// frame thread t < S expires slot t, thread d < N classes pose d, finds its slot, and after the births does the whole
// of pose d: anchor, at most 128 edge tests, 8 line tests, the slot's stores and the pose's outputs.  What a thread
// found stays in bit masks, so its event count is a popcount; an exclusive scan of the 256 counts (the slots', then
// the poses') in LDS gives every thread the row of its first event, whatever order the threads run in.  Threads 128 ..
// 183 add the masks up into the counters, one counter each.  Every loop bound is from the plan or the maxima of the
// header, geometry counts are clamped as they are read, every barrier is block-uniform, there are no global atomics
// and no scratch area.
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
constexpr int MAXZ = PAVE_ZONE_MAX_ZONES;
constexpr int MAXL = PAVE_ZONE_MAX_LINES;
constexpr int MAXV = PAVE_ZONE_MAX_VERTICES;
constexpr int EW = PAVE_ZONE_EVENT_WORDS;
static_assert(MAXP + MAXS == NT, "one scan item per thread: the slots, then the poses");
static_assert(MAXP <= 128 && MAXS <= 128 && PAVE_ZONE_COUNTER_WORDS <= NT - 128, "thread roles");

// cross(u, v) >= 0
__device__ __forceinline__ bool left_of(const long long ux, const long long uy, const long long vx, const long long vy) {
  return ux * vy - uy * vx >= 0;
}

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

__global__ __launch_bounds__(NT) void zone_events_kernel(const pave_zone_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int det_id[MAXP];
  __shared__ int det_bad[MAXP];      // != 0: a coordinate that is not finite
  __shared__ int det_ok[MAXP];       // != 0: keep and a box score above the threshold
  __shared__ int det_slot[MAXP];     // the slot of a pose that takes part, or -1
  __shared__ int det_born[MAXP];     // != 0: the slot was born in this frame
  __shared__ int geom[PAVE_ZONE_GEOM_WORDS];
  __shared__ int m_vanish[MAXS];     // the zone bits of a slot that expired in this frame
  __shared__ int m_zone[MAXP];       // of a pose: ENTER bits | EXIT << 8 | APPEAR << 16 | DWELL << 24
  __shared__ int m_line[MAXP];       // of a pose: CROSS_FWD bits | CROSS_BACK << 8
  __shared__ int scan[2][NT];
  __shared__ int cam_state[2];       // frame, dropped

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S, K = plan.K;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_pos = plan.slot_pos + (long long)cam * S * 2;
  int32_t* __restrict__ g_inside = plan.slot_inside + (long long)cam * S;
  int32_t* __restrict__ g_alerted = plan.slot_alerted + (long long)cam * S;
  int32_t* __restrict__ g_streak = plan.slot_streak + (long long)cam * S * MAXZ;
  int32_t* __restrict__ g_since = plan.slot_since + (long long)cam * S * MAXZ;
  int32_t* __restrict__ g_count = plan.counters + (long long)cam * PAVE_ZONE_COUNTER_WORDS;
  const int32_t* __restrict__ g_geom = plan.geometry + (long long)cam * PAVE_ZONE_GEOM_WORDS;

  for (int i = tid; i < PAVE_ZONE_GEOM_WORDS; i += NT) {   // the geometry, its counts clamped to the maxima
    int v = g_geom[i];
    if (i == PAVE_ZONE_GEOM_NZONES) v = min(max(v, 0), MAXZ);
    if (i == PAVE_ZONE_GEOM_NLINES) v = min(max(v, 0), MAXL);
    if (i >= PAVE_ZONE_GEOM_NVERT && i < PAVE_ZONE_GEOM_NVERT + MAXZ) v = min(max(v, 0), MAXV);
    geom[i] = v;
  }
  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.dropped[cam];
  }

  for (int e = b; e < plan.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; geom and cam_state are written
    const int n = plan.n[e];
    const float sx = plan.scale[e][0], sy = plan.scale[e][1];
    const float* __restrict__ kpts = plan.kpts[e];
    const float* __restrict__ bboxes = plan.bboxes[e];
    const int32_t* __restrict__ keep = plan.keep[e];
    const int32_t* __restrict__ ids = plan.ids[e];
    int32_t* __restrict__ out_zones = plan.out_zones[e];
    int32_t* __restrict__ out_dwell = plan.out_dwell[e];
    int32_t* __restrict__ out_events = plan.out_events[e];
    const int max_events = plan.max_events;
    const int frame = (int)((unsigned)cam_state[0] + 1u);
    const int nz = geom[PAVE_ZONE_GEOM_NZONES], nl = geom[PAVE_ZONE_GEOM_NLINES];
    const int zmask = (1 << nz) - 1;

    // ---- 1, 2: expire the slots; the poses' boxes ----
    int vanish = 0, vanish_id = 0;
    if (tid < MAXS) {
      vanish_id = expire_slot(plan, g_id, g_last, slot_id, tid, S, frame);
      if (vanish_id != 0) vanish = g_inside[tid] & zmask;
      m_vanish[tid] = vanish;
    }
    int X1 = 0, Y1 = 0, X2 = 0, Y2 = 0;
    if (tid < n)
      classify_pose(bboxes, keep, ids, sx, sy, plan.score_thr, tid, det_id, det_bad, det_ok, det_born, X1, Y1, X2, Y2);
    __syncthreads();
    sweep_finite<NT>(kpts, n, K, tid, det_bad);
    __syncthreads();

    // ---- 2: the slot of every pose ----
    if (tid < n) det_slot[tid] = find_slot(det_id, det_ok, det_bad, slot_id, tid, S);
    __syncthreads();
    if (tid == 0)   // births, in ascending pose index into the lowest free slot; the clock
      commit_births(plan, cam, n, S, frame, true, g_id, slot_id, det_id, det_slot, det_born, cam_state);
    __syncthreads();

    // ---- 3, 4, 5: pose tid in its slot ----
    int mz = 0, ml = 0;
    if (tid < n) {
      const int t = det_slot[tid];   // (in 0 .. S - 1 or -1: a slot index is a loop counter of step 2)
      int inside = 0, dwell_of[MAXZ];   // (every index of it is a constant of an unrolled loop: registers)
#pragma unroll
      for (int z = 0; z < MAXZ; ++z) dwell_of[z] = 0;
      if (t >= 0) {
        long long ax, ay;
        anchor(plan, kpts, tid, K, sx, sy, X1, Y1, X2, Y2, ax, ay);
        int raw = 0;
        for (int z = 0; z < nz; ++z) {
          const int nv = geom[PAVE_ZONE_GEOM_NVERT + z];
          const int* v = geom + PAVE_ZONE_GEOM_ZONES + z * MAXV * 2;
          bool in = false;
          for (int i = 0; i < nv; ++i) {
            const int j = i + 1 < nv ? i + 1 : 0;
            const long long x0 = v[2 * i], y0 = v[2 * i + 1], x1 = v[2 * j], y1 = v[2 * j + 1];
            if ((y0 > ay) != (y1 > ay)) {
              const long long dy = y1 - y0;
              const long long w = (ax - x0) * dy - (ay - y0) * (x1 - x0);
              in = in != (dy > 0 ? w < 0 : w > 0);
            }
          }
          raw |= in ? 1 << z : 0;
        }
        int alerted = 0;
        if (det_born[tid] != 0) {
          inside = raw;
          mz = raw << 16;
#pragma unroll
          for (int z = 0; z < MAXZ; ++z) {
            g_streak[t * MAXZ + z] = 0;
            g_since[t * MAXZ + z] = frame;
          }
        } else {
          inside = g_inside[t];
          alerted = g_alerted[t];
#pragma unroll
          for (int z = 0; z < MAXZ; ++z) {
            if (z >= nz) continue;
            const int bit = 1 << z;
            int streak = g_streak[t * MAXZ + z], since = g_since[t * MAXZ + z];
            if (((raw ^ inside) & bit) == 0) {
              streak = 0;
            } else if (++streak >= plan.min_frames) {
              streak = 0;
              inside ^= bit;
              if (inside & bit) {
                since = frame;
                mz |= bit;
              } else {
                alerted &= ~bit;
                mz |= bit << 8;
              }
            }
            const int wait = geom[PAVE_ZONE_GEOM_DWELL + z];
            if ((inside & bit) && wait > 0 && (long long)frame - since >= wait && !(alerted & bit)) {
              alerted |= bit;
              mz |= bit << 24;
            }
            g_streak[t * MAXZ + z] = streak;
            g_since[t * MAXZ + z] = since;
            dwell_of[z] = (inside & bit) ? (int)((unsigned)frame - (unsigned)since) : 0;
          }
          const long long qx = g_pos[2 * t], qy = g_pos[2 * t + 1];
          if (qx != ax || qy != ay) {
            for (int l = 0; l < nl; ++l) {
              const int* ln = geom + PAVE_ZONE_GEOM_LINES + l * 4;
              const long long Ax = ln[0], Ay = ln[1], Bx = ln[2], By = ln[3];
              const bool sq = left_of(Bx - Ax, By - Ay, qx - Ax, qy - Ay);
              const bool sp = left_of(Bx - Ax, By - Ay, ax - Ax, ay - Ay);
              if (sq == sp) continue;
              const bool sa = left_of(ax - qx, ay - qy, Ax - qx, Ay - qy);
              const bool sb = left_of(ax - qx, ay - qy, Bx - qx, By - qy);
              if (sa == sb) continue;
              ml |= sq ? 1 << (8 + l) : 1 << l;
            }
          }
        }
        g_pos[2 * t] = (int32_t)ax;
        g_pos[2 * t + 1] = (int32_t)ay;
        g_last[t] = frame;
        g_inside[t] = inside;
        g_alerted[t] = alerted;
      }
      out_zones[tid] = inside;
#pragma unroll
      for (int z = 0; z < MAXZ; ++z) out_dwell[tid * MAXZ + z] = dwell_of[z];
    }
    if (tid < MAXP) {
      m_zone[tid] = mz;
      m_line[tid] = ml;
      scan[0][tid] = __popc(vanish);
      scan[0][MAXS + tid] = __popc(mz) + __popc(ml);
    }
    __syncthreads();

    // ---- 6: the row of every thread's first event; the counters ----
    int buf = 0;
    for (int step = 1; step < NT; step <<= 1) {   // an inclusive scan of the 256 counts
      const int v = scan[buf][tid] + (tid >= step ? scan[buf][tid - step] : 0);
      scan[buf ^ 1][tid] = v;
      __syncthreads();
      buf ^= 1;
    }
    const int total = scan[buf][NT - 1];
    if (tid < MAXP) {
      int row = scan[buf][tid] - __popc(vanish);
      for (int z = 0; z < MAXZ; ++z)
        if ((vanish >> z) & 1) put(out_events, row, max_events, PAVE_ZONE_VANISH, z, vanish_id, -1, frame);
      row = scan[buf][MAXS + tid] - (__popc(mz) + __popc(ml));
      if (mz != 0 || ml != 0) {
        const int id = det_id[tid];
        for (int z = 0; z < MAXZ; ++z) {
          if ((mz >> z) & 1) put(out_events, row, max_events, PAVE_ZONE_ENTER, z, id, tid, frame);
          if ((mz >> (8 + z)) & 1) put(out_events, row, max_events, PAVE_ZONE_EXIT, z, id, tid, frame);
          if ((mz >> (16 + z)) & 1) put(out_events, row, max_events, PAVE_ZONE_APPEAR, z, id, tid, frame);
          if ((mz >> (24 + z)) & 1) put(out_events, row, max_events, PAVE_ZONE_DWELL, z, id, tid, frame);
        }
        for (int l = 0; l < MAXL; ++l) {
          if ((ml >> l) & 1) put(out_events, row, max_events, PAVE_ZONE_CROSS_FWD, l, id, tid, frame);
          if ((ml >> (8 + l)) & 1) put(out_events, row, max_events, PAVE_ZONE_CROSS_BACK, l, id, tid, frame);
        }
      }
    } else if (tid - MAXP < PAVE_ZONE_COUNTER_WORDS) {   // one counter per thread, summed in a fixed order
      const int c = tid - MAXP;
      int delta = 0;
      if (c < PAVE_ZONE_CNT_CROSSED) {
        const int kind = c >> 3, z = c & 7;
        for (int d = 0; d < n; ++d) {
          const int m = m_zone[d];
          const int enter = (m >> z) & 1, exit = (m >> (8 + z)) & 1, appear = (m >> (16 + z)) & 1;
          delta += kind == 0 ? enter + appear - exit : kind == 1 ? enter : kind == 2 ? exit : kind == 3 ? appear : 0;
        }
        if (kind == 0 || kind == 4)
          for (int t = 0; t < S; ++t) delta += ((m_vanish[t] >> z) & 1) * (kind == 0 ? -1 : 1);
      } else {
        const int l = (c - PAVE_ZONE_CNT_CROSSED) >> 1, back = (c - PAVE_ZONE_CNT_CROSSED) & 1;
        for (int d = 0; d < n; ++d) delta += (m_line[d] >> (8 * back + l)) & 1;
      }
      if (delta != 0) g_count[c] = (int)((unsigned)g_count[c] + (unsigned)delta);
    }
    if (tid == 0) plan.out_n_events[e][0] = total;
    for (int i = min(total, max_events) * EW + tid; i < max_events * EW; i += NT) out_events[i] = 0;
  }
}

}  // namespace

extern "C" {

int pave_zone_events(const pave_zone_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "zone_events: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "zone_events: K outside 1 .. 32");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_pos || !plan->slot_inside || !plan->slot_alerted ||
      !plan->slot_streak || !plan->slot_since || !plan->frame || !plan->dropped || !plan->counters)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: null state tensor");
  if (!plan->geometry) return pave_internal_fail(PAVE_E_ARG, "zone_events: null geometry tensor");
  if (plan->min_frames < 1 || plan->min_frames > 255)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: min_frames outside 1 .. 255");
  if (plan->max_events < 1 || plan->max_events > PAVE_ZONE_MAX_EVENTS)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: max_events outside 1 .. 4096");
  if (plan->anchor < PAVE_ZONE_ANCHOR_FEET || plan->anchor > PAVE_ZONE_ANCHOR_CENTRE)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: anchor outside 0 .. 2");
  if (plan->n_anchor < 0 || plan->n_anchor > PAVE_ZONE_MAX_ANCHOR_KPTS)
    return pave_internal_fail(PAVE_E_ARG, "zone_events: n_anchor outside 0 .. 4");
  for (int i = 0; i < plan->n_anchor; ++i)
    if (plan->anchor_kpt[i] < 0 || plan->anchor_kpt[i] >= plan->K)
      return pave_internal_fail(PAVE_E_ARG, "zone_events: an anchor key point outside [0, K)");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "zone_events: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "zone_events: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "zone_events: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "zone_events: null ids tensor");
    if (n > 0 && (!plan->out_zones[i] || !plan->out_dwell[i]))
      return pave_internal_fail(PAVE_E_ARG, "zone_events: null output tensor");
    if (!plan->out_events[i] || !plan->out_n_events[i])
      return pave_internal_fail(PAVE_E_ARG, "zone_events: null events tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "zone_events: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "zone_events: scale must be positive and finite");
  }
  return pave_launch<zone_events_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                         reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
