// Contacts and groups on the floor for the live path: which tracks stand within a radius of each other, debounced with
// hysteresis, for how long, which parties they form and the MEET / PART / LONG events of the frame, on the device, in
// one launch for up to 32 frames of any number of cameras (pave_contact_update).  It reads what pave_floor_update
// wrote: a pose's `on` flag and its floor position in mm.
//
// The rule is DESIGN section 24 and is integer-exact.  A pose takes part iff it is on the floor, its id is >= 1 and no
// such pose before it has that id; it is followed iff it finds or takes a slot (pave_tracked.h's slots: the clock, the
// expiry after max_age frames, the serial births of one lane), and its slot then holds its position (clamped to
// +-PAVE_FLOOR_MAX_MM) and the frame.  A slot pair s < t has two words, link (bit 0: in contact, bits 8 ..: run) and
// since.  In one frame a pair goes through these steps, in this order:
//   expiry      one of the two slots was freed in this frame and the other was live before it: a contact gives PART
//               (frames = frame - since, the ids the slots held, poses -1); the words are cleared
//   birth       both slots are live now and one was born in this frame: the words are read as zero
//   evaluation  both are live and were seen in this frame: d2 = dx^2 + dy^2 in 64 bits, near = d2 <= (contact ?
//               release : radius)^2; near == contact: run = 0; else run += 1 and at run >= min_frames the bit flips
//               and run = 0: set, since = frame and MEET (frames 0); cleared, PART (frames = frame - since), since = 0
//   long        both are live and in contact, seen or not: frame - since == long_frames > 0 gives LONG
// The table holds the expiry PARTs in ascending (s, t), then the other events in ascending (s, t).  The groups are the
// connected components of the live slots under the contact bits; a component is named by its smallest track id.
//
// One block of 256 threads per camera of the launch (pave_tracked.h).  Thread t < S expires slot t, thread d < N finds
// the slot of pose d, one lane commits the births.  Only a pair of two slots that hold or held an id has words that
// mean something, so those M <= S slots are listed in ascending order (two ballots), and the M (M - 1) / 2 pairs of
// the list, counted row by row -- which is ascending (s, t) -- are dealt to the threads as contiguous ranges of at
// most 32: the work follows the people on the floor, not max_tracks.  A thread loads the words of its range into
// registers, all loads in flight at once (nobody else writes them), and then walks the range twice over those
// registers: once to count its events of both kinds, and, after a block scan of the (packed) counts has given it the
// rows of its first events, once more to store the words that changed and the events -- the same decision from the
// same words -- so the table's order does not depend on how the threads are scheduled.  What a walk needs of a slot
// is one LDS word of flags.  The second walk also sets the two bits of every contact in a 128-bit
// adjacency mask per slot in LDS.  Components: label = track id, then every slot takes the smallest label among itself
// and its neighbours until a round changes nothing (__syncthreads_or), at most S - 1 rounds: the longest path a label
// can travel.  Sizes are a count over the labels.  The counters are summed through LDS atomics of integers, whose
// result does not depend on their order.  Every loop bound is from the plan or the maxima of the header, every barrier
// is block-uniform, there are no global atomics and no scratch area.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using namespace pave_tracked;

constexpr int NT = 256;                              // threads of a block
constexpr int MAXP = PAVE_TRACK_MAX_POSES;
constexpr int MAXS = PAVE_TRACK_MAX_TRACKS;
constexpr int PER = (MAXS * (MAXS - 1) / 2 + NT - 1) / NT;   // the most pairs of one thread
constexpr int EW = PAVE_CONTACT_EVENT_WORDS;
constexpr int MM = PAVE_FLOOR_MAX_MM;
constexpr int FREE_LABEL = 0x7fffffff;               // the label of a free slot: above every id
static_assert(MAXP <= NT && MAXS <= NT && MAXS == 128, "thread roles; the adjacency mask is four 32-bit words");
static_assert(MAXS * (MAXS - 1) / 2 < 65536, "two event counts are packed into one word for the scan");
static_assert(PER == 32, "the registers of a thread's range");

enum : int {     // what a walk needs of a slot
  WAS = 1,       // it held an id before the expiry of this frame
  NOW = 2,       // it holds one now
  FREED = 4,     // it was freed in this frame
  BORN = 8,      // it was born in this frame
  SEEN = 16,     // a pose was followed into it in this frame
};

// What one frame does to the pair s < t, from the words as they were.
struct Step {
  int link, since;       // the words after the frame
  int expiry;            // != 0: an expiry PART, of `expiry_frames` frames
  int expiry_frames;
  int kind, frames;      // the event of the live pair, or kind 0
  bool touched;          // the words are to be stored
  bool contact;          // both slots are live and in contact after the frame
};

struct Frame {
  const int* flags;
  const int* slot_x;     // of a slot seen in this frame: its position in mm
  const int* slot_y;
  long long radius2, release2;
  int frame, min_frames, long_frames;
};

__device__ __forceinline__ Step pair_step(const Frame& f, const int s, const int t, const int fs, int link, int since) {
  Step r = {0, 0, 0, 0, 0, 0, false, false};
  const int ft = f.flags[t];
  const bool expiry = (fs & ft & WAS) != 0 && ((fs | ft) & FREED) != 0, are = (fs & ft & NOW) != 0;
  if (!expiry && !are) return r;   // (a pair with a free slot: its words mean nothing)
  const int link0 = link, since0 = since;
  if (expiry) {
    if (link & 1) r.expiry = 1, r.expiry_frames = (int)((unsigned)f.frame - (unsigned)since);
    link = 0, since = 0;
  }
  if (are) {
    if ((fs | ft) & BORN) link = 0, since = 0;
    int contact = link & 1, run = (int)((unsigned)link >> 8);
    if (fs & ft & SEEN) {
      const long long dx = (long long)f.slot_x[s] - f.slot_x[t], dy = (long long)f.slot_y[s] - f.slot_y[t];
      const long long d2 = dx * dx + dy * dy;   // (|d| < 2^21: below 2^43)
      const int near = d2 <= (contact ? f.release2 : f.radius2) ? 1 : 0;
      if (near == contact) {
        run = 0;
      } else if (++run >= f.min_frames) {
        run = 0;
        contact ^= 1;
        if (contact) {
          since = f.frame;
          r.kind = PAVE_CONTACT_MEET;
        } else {
          r.kind = PAVE_CONTACT_PART, r.frames = (int)((unsigned)f.frame - (unsigned)since);
          since = 0;
        }
      }
    }
    if (contact && f.long_frames > 0 && (int)((unsigned)f.frame - (unsigned)since) == f.long_frames)
      r.kind = PAVE_CONTACT_LONG, r.frames = f.long_frames;   // (a MEET of this frame has frame - since == 0)
    link = contact | (int)((unsigned)run << 8);
    r.contact = contact != 0;
  }
  r.link = link, r.since = since;
  r.touched = link != link0 || since != since0;
  return r;
}

__device__ __forceinline__ void put(int32_t* events, const int row, const int max_events, const int kind, int a, int b,
                                    const int frames, int pose_a, int pose_b, const int frame) {
  if (row >= max_events) return;
  if (a > b) {   // the smaller id first, its pose with it
    int v = a;
    a = b, b = v;
    v = pose_a, pose_a = pose_b, pose_b = v;
  }
  int32_t* r = events + (long long)row * EW;
  r[0] = kind, r[1] = a, r[2] = b, r[3] = frames, r[4] = pose_a, r[5] = pose_b, r[6] = frame;
}

__global__ __launch_bounds__(NT) void contact_update_kernel(const pave_contact_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int was_id[MAXS];       // before the expiry of this frame
  __shared__ int flags[MAXS];
  __shared__ int list[MAXS];         // the slots whose flags are not 0, ascending
  __shared__ int wave_held[NT / 64];
  __shared__ int born[MAXS];
  __shared__ int slot_pose[MAXS];    // the pose that was followed into the slot in this frame, or -1
  __shared__ int slot_x[MAXS];
  __shared__ int slot_y[MAXS];
  __shared__ int label[MAXS];
  __shared__ int size_of[MAXS];
  __shared__ unsigned adj[MAXS][4];  // bit u of slot t: t and u are live and in contact
  __shared__ int det_id[MAXP];
  __shared__ int det_ok[MAXP];       // != 0: on the floor
  __shared__ int det_slot[MAXP];     // the slot of a followed pose, or -1
  __shared__ int det_born[MAXP];
  __shared__ int det_x[MAXP];
  __shared__ int det_y[MAXP];
  __shared__ int scan[2][NT];        // expiry events | the other events << 16
  __shared__ int tally[PAVE_CONTACT_COUNTER_WORDS];
  __shared__ int cam_state[2];       // frame, dropped

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_pos = plan.slot_pos + (long long)cam * S * 2;
  int32_t* g_link = plan.link + (long long)cam * S * S;      // (since is read again after other threads wrote it)
  int32_t* g_since = plan.since + (long long)cam * S * S;
  int32_t* __restrict__ g_count = plan.counters + (long long)cam * PAVE_CONTACT_COUNTER_WORDS;

  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.dropped[cam];
  }

  Frame f;
  f.flags = flags, f.slot_x = slot_x, f.slot_y = slot_y;
  f.radius2 = (long long)plan.radius * plan.radius, f.release2 = (long long)plan.release * plan.release;
  f.min_frames = plan.min_frames, f.long_frames = plan.long_frames;

  for (int e = b; e < plan.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; cam_state is written
    const int n = plan.n[e];
    const int32_t* __restrict__ on = plan.on[e];
    const int32_t* __restrict__ xy = plan.xy[e];
    const int32_t* __restrict__ ids = plan.ids[e];
    int32_t* __restrict__ out = plan.out[e];
    int32_t* __restrict__ out_events = plan.out_events[e];
    const int max_events = plan.max_events;
    const int frame = (int)((unsigned)cam_state[0] + 1u);
    f.frame = frame;

    // ---- 1: expire the slots; the poses ----
    int flag = 0;
    if (tid < MAXS) {
      const int expired = expire_slot(plan, g_id, g_last, slot_id, tid, S, frame);
      was_id[tid] = expired != 0 ? expired : slot_id[tid];
      flag = (was_id[tid] != 0 ? WAS : 0) | (expired != 0 ? FREED : 0);
      born[tid] = 0;
      slot_pose[tid] = -1;
      adj[tid][0] = adj[tid][1] = adj[tid][2] = adj[tid][3] = 0u;
    }
    if (tid < PAVE_CONTACT_COUNTER_WORDS) tally[tid] = 0;
    if (tid < n) {
      det_id[tid] = ids[tid];
      det_ok[tid] = on[tid] != 0 ? 1 : 0;
      det_born[tid] = 0;
      det_x[tid] = min(max(xy[2 * tid], -MM), MM);
      det_y[tid] = min(max(xy[2 * tid + 1], -MM), MM);
    }
    __syncthreads();
    if (tid < n) det_slot[tid] = find_slot(det_id, det_ok, nullptr, slot_id, tid, S);
    __syncthreads();
    if (tid == 0)   // births, in ascending pose index into the lowest free slot; the clock
      commit_births(plan, cam, n, S, frame, true, g_id, slot_id, det_id, det_slot, det_born, cam_state);
    __syncthreads();
    if (tid < n) {
      const int t = det_slot[tid];   // (in 0 .. S - 1 or -1: a slot index is a loop counter)
      if (t >= 0) {
        born[t] = det_born[tid];
        slot_pose[t] = tid;
        slot_x[t] = det_x[tid];
        slot_y[t] = det_y[tid];
        g_pos[2 * t] = det_x[tid];
        g_pos[2 * t + 1] = det_y[tid];
        g_last[t] = frame;
      }
    }
    __syncthreads();
    if (tid < MAXS) {
      const int id = slot_id[tid];
      label[tid] = id != 0 ? id : FREE_LABEL;
      flag |= (id != 0 ? NOW : 0) | (born[tid] != 0 ? BORN : 0) | (slot_pose[tid] >= 0 ? SEEN : 0);
      flags[tid] = flag;
    }
    // the slots that hold or held an id, in ascending order: only their pairs have words that mean something
    const unsigned long long held = __ballot(flag != 0 ? 1 : 0);   // (flag is 0 for tid >= S)
    if ((tid & 63) == 0) wave_held[tid >> 6] = __popcll(held);
    __syncthreads();
    if (flag != 0) list[(tid >= 64 ? wave_held[0] : 0) + __popcll(held & ((1ull << (tid & 63)) - 1ull))] = tid;
    const int M = wave_held[0] + wave_held[1];   // (<= S: waves 2 and 3 hold no slot)
    __syncthreads();

    // this thread's pairs: [k0, k1) of the M (M - 1) / 2 pairs a < b of the list, counted row by row, and the (a, b)
    // of k0: the largest a with a (2 M - a - 1) / 2 <= k0, a float's guess put right
    const int pairs = M * (M - 1) / 2, per = (pairs + NT - 1) / NT;   // (per <= PER)
    const int k0 = min(tid * per, pairs), k1 = min(k0 + per, pairs);
    int a0 = 0, b0 = 1;
    if (k0 < k1) {   // (M >= 2)
      const int q = 2 * M - 1;
      a0 = min(max((int)(((float)q - sqrtf((float)(q * q - 8 * k0))) * 0.5f), 0), M - 2);
      while (a0 > 0 && a0 * (2 * M - a0 - 1) / 2 > k0) --a0;
      while (a0 < M - 2 && (a0 + 1) * (2 * M - a0 - 2) / 2 <= k0) ++a0;
      b0 = a0 + 1 + k0 - a0 * (2 * M - a0 - 1) / 2;
    }
    const int s0 = k0 < k1 ? list[a0] : 0;   // (a slot below S, as every entry of the list below M is)

    // ---- the words of this thread's pairs as the frame before left them: of the pairs that a step can touch ----
    int w_link[PER], w_since[PER];
    {
      int a = a0, c = b0, s = s0, fs = flags[s0];
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        w_link[i] = 0, w_since[i] = 0;
        if (k0 + i < k1) {
          const int t = list[c], ft = flags[t];
          if ((fs & ft & NOW) != 0 || ((fs & ft & WAS) != 0 && ((fs | ft) & FREED) != 0)) {
            w_link[i] = g_link[s * S + t];
            w_since[i] = g_since[s * S + t];
          }
          if (++c == M) ++a, c = a + 1, s = list[a], fs = flags[s];   // (a <= M - 1: after the last pair it is M - 1)
        }
      }
    }

    // ---- 2 .. 4, the first walk: this thread's events of both kinds ----
    int n_expiry = 0, n_other = 0;
    {
      int a = a0, c = b0, s = s0, fs = flags[s0];
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        if (k0 + i < k1) {
          const Step r = pair_step(f, s, list[c], fs, w_link[i], w_since[i]);
          n_expiry += r.expiry;
          n_other += r.kind != 0 ? 1 : 0;
          if (++c == M) ++a, c = a + 1, s = list[a], fs = flags[s];
        }
      }
    }
    scan[0][tid] = n_expiry | (n_other << 16);
    __syncthreads();
    int buf = 0;
    for (int step = 1; step < NT; step <<= 1) {   // an inclusive scan of the 256 packed counts (neither half carries)
      const int v = scan[buf][tid] + (tid >= step ? scan[buf][tid - step] : 0);
      scan[buf ^ 1][tid] = v;
      __syncthreads();
      buf ^= 1;
    }
    const int total_expiry = scan[buf][NT - 1] & 0xffff, total_other = (int)((unsigned)scan[buf][NT - 1] >> 16);
    const int total = total_expiry + total_other;

    // ---- the second walk: the words, the events, the adjacency ----
    {
      int row_expiry = (scan[buf][tid] & 0xffff) - n_expiry;
      int row_other = total_expiry + (int)((unsigned)scan[buf][tid] >> 16) - n_other;
      int meets = 0, parts = 0, longs = 0, contacts = 0;
      int a = a0, c = b0, s = s0, fs = flags[s0];
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        if (k0 + i < k1) {
          const int t = list[c];
          const Step r = pair_step(f, s, t, fs, w_link[i], w_since[i]);
          if (r.touched) {
            g_link[s * S + t] = r.link;
            g_since[s * S + t] = r.since;
          }
          if (r.expiry) {
            put(out_events, row_expiry++, max_events, PAVE_CONTACT_PART, was_id[s], was_id[t], r.expiry_frames, -1, -1, frame);
            ++parts;
          }
          if (r.kind != 0) {
            put(out_events, row_other++, max_events, r.kind, slot_id[s], slot_id[t], r.frames, slot_pose[s], slot_pose[t],
                frame);
            meets += r.kind == PAVE_CONTACT_MEET ? 1 : 0;
            parts += r.kind == PAVE_CONTACT_PART ? 1 : 0;
            longs += r.kind == PAVE_CONTACT_LONG ? 1 : 0;
          }
          if (r.contact) {
            ++contacts;
            atomicOr(&adj[s][t >> 5], 1u << (t & 31));
            atomicOr(&adj[t][s >> 5], 1u << (s & 31));
          }
          if (++c == M) ++a, c = a + 1, s = list[a], fs = flags[s];
        }
      }
      if (contacts != 0) atomicAdd(&tally[PAVE_CONTACT_CNT_CONTACTS], contacts);
      if (meets != 0) atomicAdd(&tally[PAVE_CONTACT_CNT_MEETS], meets);
      if (parts != 0) atomicAdd(&tally[PAVE_CONTACT_CNT_PARTS], parts);
      if (longs != 0) atomicAdd(&tally[PAVE_CONTACT_CNT_LONGS], longs);
    }
    if (tid == 0) plan.out_n_events[e][0] = total;
    for (int i = min(total, max_events) * EW + tid; i < max_events * EW; i += NT) out_events[i] = 0;
    __syncthreads();   // adj, tally and the words are written

    // ---- 5: the components ----
    const bool live = tid < S && slot_id[tid] != 0;
    for (int round = 0; round < S - 1; ++round) {   // (S is the plan's: block-uniform, as is the break)
      int m = FREE_LABEL;
      if (live) {
        m = label[tid];
        for (int w = 0; w < 4; ++w)
          for (unsigned bits = adj[tid][w]; bits != 0u; bits &= bits - 1u) m = min(m, label[w * 32 + __ffs(bits) - 1]);
      }
      const int changed = live && m != label[tid] ? 1 : 0;
      if (!__syncthreads_or(changed)) break;   // (every label of the round is read)
      if (changed) label[tid] = m;
      __syncthreads();
    }
    if (tid < MAXS) {
      int size = 0;
      if (live)
        for (int u = 0; u < S; ++u) size += label[u] == label[tid] ? 1 : 0;   // (a free slot's label is no id)
      size_of[tid] = size;
      if (live) {
        atomicMax(&tally[PAVE_CONTACT_CNT_LARGEST], size);
        if (size >= 2 && label[tid] == slot_id[tid]) {   // the slot that names its component
          atomicAdd(&tally[PAVE_CONTACT_CNT_GROUPS], 1);
          atomicAdd(&tally[PAVE_CONTACT_CNT_GROUPED], size);
        }
      }
    }
    __syncthreads();

    // ---- 6: the poses; 8: the counters ----
    if (tid < n) {
      const int t = det_slot[tid];
      int group = 0, size = 0, degree = 0, partner = 0, together = 0;
      if (t >= 0) {
        group = label[t], size = size_of[t];
        int best = 0;
        for (int w = 0; w < 4; ++w)
          for (unsigned bits = adj[t][w]; bits != 0u; bits &= bits - 1u) {   // (ascending u: the lower slot on a tie)
            const int u = w * 32 + __ffs(bits) - 1;
            const int since = g_since[min(t, u) * S + max(t, u)];
            if (degree == 0 || since < best) best = since, partner = slot_id[u];
            ++degree;
          }
        if (degree != 0) together = (int)((unsigned)frame - (unsigned)best);
      }
      out[tid] = group;
      out[n + tid] = size;
      out[2 * n + tid] = degree;
      out[3 * n + tid] = partner;
      out[4 * n + tid] = together;
    }
    if (tid < PAVE_CONTACT_COUNTER_WORDS) {
      const bool running = tid == PAVE_CONTACT_CNT_MEETS || tid == PAVE_CONTACT_CNT_PARTS || tid == PAVE_CONTACT_CNT_LONGS;
      g_count[tid] = running ? (int)((unsigned)g_count[tid] + (unsigned)tally[tid]) : tally[tid];
    }
  }
}

}  // namespace

extern "C" {

int pave_contact_update(const pave_contact_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "contact_update: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: 1 .. 32 frames per launch");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_pos || !plan->link || !plan->since || !plan->frame ||
      !plan->dropped || !plan->counters)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: null state tensor");
  if (plan->radius < 0 || plan->radius > PAVE_CONTACT_MAX_RADIUS)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: radius outside 0 .. 2^20");
  if (plan->release < plan->radius || plan->release > PAVE_CONTACT_MAX_RELEASE)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: release outside radius .. 2^21");
  if (plan->min_frames < 1 || plan->min_frames > 255)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: min_frames outside 1 .. 255");
  if (plan->long_frames < 0 || plan->long_frames > PAVE_CONTACT_MAX_LONG)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: long_frames outside 0 .. 2^30");
  if (plan->max_events < 1 || plan->max_events > PAVE_CONTACT_MAX_EVENTS)
    return pave_internal_fail(PAVE_E_ARG, "contact_update: max_events outside 1 .. 4096");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "contact_update: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "contact_update: N outside 0 .. 128");
    if (n > 0 && (!plan->on[i] || !plan->xy[i])) return pave_internal_fail(PAVE_E_ARG, "contact_update: null floor tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "contact_update: null ids tensor");
    if ((n > 0 && !plan->out[i]) || !plan->out_events[i] || !plan->out_n_events[i])
      return pave_internal_fail(PAVE_E_ARG, "contact_update: null output tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "contact_update: a camera index outside [0, cameras)");
  }
  return pave_launch<contact_update_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                            reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
