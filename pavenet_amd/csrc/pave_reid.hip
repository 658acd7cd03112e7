// The same person again: a colour descriptor per pose, read from the pixels under it, and a gallery per camera that
// maps track ids to person ids (pave_reid_describe_nv12 / _bgr, pave_reid_update_nv12 / _bgr).
//
// The rule is DESIGN section 18 and is integer-exact.  A coordinate becomes quarter pixels as in sections 13 .. 17,
//   X = clamp((int)rintf((x / sx) * 4.f), 0, 32767)     (correctly rounded division, no contraction).
// A pose has two regions, the torso (shoulders and hips) and the legs (hips and knees): the bounding rectangle of the
// visible key points of both parts (one of each at least), shrunk by (extent >> 3) on every side; a torso that cannot
// be formed is the box's central half in x and second quarter in y; a rectangle narrower than (box width >> 2) is
// widened about its centre to that.  A sample is a 2 x 2 pixel block (bx, by) = (X >> 3, Y >> 3), clipped to the
// picture's whole blocks; a region of w x h blocks is read at the smallest power-of-two stride s with
// ceil(w / s) ceil(h / s) <= 1024, and is invalid below 16 samples.  NV12: Y = (the four luma bytes + 2) >> 2, U and V
// the block's chroma bytes; BGR: the rounded mean per channel, (G, B, R) standing in for (Y, U, V).  A sample votes
// into a 4 x 8 x 8 histogram with soft bins: on an axis of n bins of width w = 256 / n, t = clamp(c - w / 2, 0,
// (n - 1) w), bins t / w and min(t / w + 1, n - 1) with weights 8 - f and f, f = (t % w) 8 / w; the product of the
// three weights goes to eight bins.  The descriptor is q[b] = (h[b] 128) / n.
//
// describe: one block of 256 threads per (entry, pose, region).  Thread 0 forms the region; the block reads the
// samples row by row -- at stride 1 a thread takes an aligned pair of blocks with dword loads (NV12: one dword per
// luma row and one of chroma; BGR: three per row) where the base and the pitch are multiples of 4 and both blocks
// are inside the picture, and byte loads otherwise -- votes with LDS atomics into 256 words and thread b writes
// bin b.  Integer adds commute, so the histogram does not depend on the order of the votes.
//
// link: one block of 256 threads per camera of the launch: block b works iff entry b is the first entry of its
// camera, and then takes that camera's entries in plan order, as zone_events_kernel does.  Per frame: thread t < S
// expires slot t; thread d < n classes pose d, forms its rectangles again (for the overlap guard) and finds the slot
// bound to its track id; the min-sums of (new pose, candidate slot) pairs are spread over the block's four waves, a thread
// taking one pair at a time with 16-byte loads (its 128 loads are independent, so they overlap); the greedy choice takes the largest key
// score * 2^14 + (127 - pose) * 2^7 + (127 - slot) by an LDS atomic max until none is left (a maximum does not depend
// on the order either); thread 0 gives the poses left over a free slot, or the oldest lost one; thread b then moves
// bin b of every region that was seen.  Every loop bound is from the plan or the maxima of the header, every barrier
// is block-uniform and there are no global atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using pave_tracked::QMAX;
using pave_tracked::quant;

constexpr int NT = 256;
constexpr int MAXP = PAVE_TRACK_MAX_POSES;
constexpr int MAXS = PAVE_TRACK_MAX_TRACKS;
constexpr int BINS = PAVE_REID_BINS;
constexpr int MAX_SIZE = 8192;
constexpr int PAIRS_PER_THREAD = MAXP * MAXS / NT;   // of the greedy choice
static_assert(BINS == NT, "one bin per thread");
static_assert(MAXP <= 128 && MAXS <= 128 && 2 * MAXP <= NT, "thread roles and the 7-bit fields of the greedy key");

// keep, a box score above the threshold and finite coordinates; B: the quantised box
__device__ bool pose_usable(const pave_reid_describe_plan& plan, const int e, const int d, int (&B)[4]) {
  const float* bb = plan.bboxes[e] + d * 5;
  const float sx = plan.scale[e][0], sy = plan.scale[e][1];
  const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
  B[0] = quant(b0, sx), B[1] = quant(b1, sy), B[2] = quant(b2, sx), B[3] = quant(b3, sy);
  bool ok = isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3);
  ok = ok && (plan.keep[e] == nullptr || plan.keep[e][d] != 0) && bb[4] > plan.score_thr;
  const float* kp = plan.kpts[e] + (long long)d * plan.K * 3;
  for (int k = 0; k < plan.K; ++k) ok = ok && isfinite(kp[3 * k]) && isfinite(kp[3 * k + 1]);
  return ok;
}

// region r of pose d in quarter pixels -> R = (x0, y0, x1, y1); false: it cannot be formed
__device__ bool region_rect(const pave_reid_describe_plan& plan, const int e, const int d, const int r, const int (&B)[4],
                            int (&R)[4]) {
  const float* kp = plan.kpts[e] + (long long)d * plan.K * 3;
  const float sx = plan.scale[e][0], sy = plan.scale[e][1];
  int x0 = QMAX + 1, y0 = QMAX + 1, x1 = -1, y1 = -1, seen[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h)
    for (int i = 0; i < plan.n_part[r][h]; ++i) {
      const float* p = kp + 3 * plan.part[r][h][i];
      if (p[2] > plan.kpt_thr) {
        const int X = quant(p[0], sx), Y = quant(p[1], sy);
        x0 = min(x0, X), x1 = max(x1, X), y0 = min(y0, Y), y1 = max(y1, Y);
        ++seen[h];
      }
    }
  if (seen[0] > 0 && seen[1] > 0) {
    const int dx = (x1 - x0) >> 3, dy = (y1 - y0) >> 3;
    x0 += dx, x1 -= dx, y0 += dy, y1 -= dy;
  } else if (r == 0) {
    const int w = B[2] - B[0], h = B[3] - B[1];   // (>> of a negative int is arithmetic: floor)
    x0 = B[0] + (w >> 2), x1 = B[2] - (w >> 2), y0 = B[1] + (h >> 2), y1 = B[1] + (h >> 1);
  } else {
    return false;
  }
  const int min_w = (B[2] - B[0]) >> 2;
  if (x1 - x0 < min_w) {
    x0 = (x0 + x1 - min_w) >> 1;
    x1 = x0 + min_w;
  }
  R[0] = x0, R[1] = y0, R[2] = x1, R[3] = y1;
  return true;
}

// one sample's eight votes
__device__ __forceinline__ void vote(int* hist, const int Y, const int U, const int V) {
  const int ty = min(max(Y - 32, 0), 192), tu = min(max(U - 16, 0), 224), tv = min(max(V - 16, 0), 224);
  const int by = ty >> 6, bu = tu >> 5, bv = tv >> 5;
  const int fy = (ty & 63) >> 3, fu = (tu & 31) >> 2, fv = (tv & 31) >> 2;
  const int by1 = min(by + 1, 3), bu1 = min(bu + 1, 7), bv1 = min(bv + 1, 7);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int w = ((i & 4) ? fy : 8 - fy) * ((i & 2) ? fu : 8 - fu) * ((i & 1) ? fv : 8 - fv);
    const int b = (((i & 4) ? by1 : by) * 8 + ((i & 2) ? bu1 : bu)) * 8 + ((i & 1) ? bv1 : bv);
    if (w != 0) atomicAdd(&hist[b], w);
  }
}

// NB bytes from p: dwords when `wide` (p is then 4-byte aligned), bytes otherwise
template <int NB>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ p, const bool wide, int (&out)[NB]) {
  if (wide) {
#pragma unroll
    for (int k = 0; k < NB / 4; ++k) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(p + 4 * k);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[4 * k + j] = (int)((v >> (8 * j)) & 255u);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NB; ++k) out[k] = p[k];
  }
}

template <bool BGR>
__global__ __launch_bounds__(NT) void reid_describe_kernel(const pave_reid_describe_plan plan) {
  __shared__ int hist[BINS];
  __shared__ int geo[6];   // valid, bx0, by0, nx, ny, s
  const int e = blockIdx.y, d = blockIdx.x >> 1, r = blockIdx.x & 1, tid = threadIdx.x;
  if (d >= plan.n[e]) return;   // (block-uniform, before any barrier)
  const int W = plan.width[e], H = plan.height[e], pitch = plan.pitch[e];
  hist[tid] = 0;
  if (tid == 0) {
    int B[4], R[4], ok = 0;
    if (pose_usable(plan, e, d, B) && region_rect(plan, e, d, r, B, R)) {
      const int bx0 = max(R[0] >> 3, 0), by0 = max(R[1] >> 3, 0);
      const int bx1 = min(R[2] >> 3, (W >> 1) - 1), by1 = min(R[3] >> 3, (H >> 1) - 1);
      if (bx0 <= bx1 && by0 <= by1) {
        const int w = bx1 - bx0 + 1, h = by1 - by0 + 1;
        int s = 1;
        while (((w + s - 1) / s) * ((h + s - 1) / s) > PAVE_REID_CAP) s <<= 1;   // (w, h <= 4096: s <= 256)
        const int nx = (w + s - 1) / s, ny = (h + s - 1) / s;
        if (nx * ny >= PAVE_REID_MIN_SAMPLES) {
          ok = 1;
          geo[1] = bx0, geo[2] = by0, geo[3] = nx, geo[4] = ny, geo[5] = s;
        }
      }
    }
    geo[0] = ok;
  }
  __syncthreads();
  int32_t* __restrict__ out = plan.hist[e] + ((long long)d * 2 + r) * BINS;
  if (geo[0] == 0) {   // (block-uniform)
    out[tid] = 0;
    if (tid == 0) plan.count[e][d * 2 + r] = 0;
    return;
  }
  const int bx0 = geo[1], by0 = geo[2], nx = geo[3], ny = geo[4], s = geo[5];
  const uint8_t* __restrict__ src = plan.src[e];
  constexpr int BB = BGR ? 6 : 2;   // bytes of a block in one row
  const bool aligned = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)pitch) & 3u) == 0;
  if (s == 1) {
    // an item is the aligned pair of blocks (2 i, 2 i + 1) of one block row: 2 BB bytes from a multiple of 4
    const int bx1 = bx0 + nx - 1, p0 = bx0 >> 1, np = (bx1 >> 1) - p0 + 1;
    for (int item = tid; item < ny * np; item += NT) {
      const int by = by0 + item / np, bx = 2 * (p0 + item % np);
      const bool lo = bx >= bx0, hi = bx + 1 <= bx1;
      const bool wide = aligned && hi;   // (bx + 1 <= bx1 <= W / 2 - 1: both blocks are inside the picture)
      const uint8_t* r0 = src + (long long)(2 * by) * pitch + (long long)bx * BB;
      int a[2 * BB], b[2 * BB], c[4] = {0, 0, 0, 0};
      if (wide) {
        load_row<2 * BB>(r0, true, a);
        load_row<2 * BB>(r0 + pitch, true, b);
        if (!BGR) load_row<4>(src + (long long)(H + by) * pitch + 2 * bx, true, c);
      } else {
        // the blocks of the pair that are wanted, byte by byte
#pragma unroll
        for (int k = 0; k < 2 * BB; ++k) a[k] = b[k] = 0;
        if (lo) {
#pragma unroll
          for (int k = 0; k < BB; ++k) a[k] = r0[k], b[k] = r0[pitch + k];
          if (!BGR) c[0] = src[(long long)(H + by) * pitch + 2 * bx], c[1] = src[(long long)(H + by) * pitch + 2 * bx + 1];
        }
        if (hi) {
#pragma unroll
          for (int k = BB; k < 2 * BB; ++k) a[k] = r0[k], b[k] = r0[pitch + k];
          if (!BGR) c[2] = src[(long long)(H + by) * pitch + 2 * bx + 2], c[3] = src[(long long)(H + by) * pitch + 2 * bx + 3];
        }
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (!(k == 0 ? lo : hi)) continue;
        if (BGR) {
          const int o = 6 * k;
          const int mb = (a[o] + a[o + 3] + b[o] + b[o + 3] + 2) >> 2, mg = (a[o + 1] + a[o + 4] + b[o + 1] + b[o + 4] + 2) >> 2;
          const int mr = (a[o + 2] + a[o + 5] + b[o + 2] + b[o + 5] + 2) >> 2;
          vote(hist, mg, mb, mr);
        } else {
          const int o = 2 * k;
          vote(hist, (a[o] + a[o + 1] + b[o] + b[o + 1] + 2) >> 2, c[o], c[o + 1]);
        }
      }
    }
  } else {
    for (int item = tid; item < ny * nx; item += NT) {
      const int by = by0 + (item / nx) * s, bx = bx0 + (item % nx) * s;   // (inside the clipped region)
      const uint8_t* r0 = src + (long long)(2 * by) * pitch + (long long)bx * BB;
      int a[BB], b[BB];
#pragma unroll
      for (int k = 0; k < BB; ++k) a[k] = r0[k], b[k] = r0[pitch + k];
      if (BGR) {
        vote(hist, (a[1] + a[4] + b[1] + b[4] + 2) >> 2, (a[0] + a[3] + b[0] + b[3] + 2) >> 2, (a[2] + a[5] + b[2] + b[5] + 2) >> 2);
      } else {
        const uint8_t* c = src + (long long)(H + by) * pitch + 2 * bx;
        vote(hist, (a[0] + a[1] + b[0] + b[1] + 2) >> 2, c[0], c[1]);
      }
    }
  }
  __syncthreads();
  const int n = nx * ny;
  out[tid] = (hist[tid] * 128) / n;   // (hist <= 512 * 1024: the product is below 2^27)
  if (tid == 0) plan.count[e][d * 2 + r] = n;
}

__global__ __launch_bounds__(NT) void reid_link_kernel(const pave_reid_plan plan) {
  __shared__ int s_person[MAXS], s_track[MAXS], s_last[MAXS], s_hits[MAXS][2], s_cand[MAXS], s_born[MAXS];
  __shared__ int d_id[MAXP], d_part[MAXP], d_slot[MAXP], d_sim[MAXP], d_count[MAXP][2], d_box[MAXP][4];
  __shared__ int d_rect[MAXP][2][4], d_skip[MAXP][2];
  __shared__ int cam_state[3];   // frame, next, dropped
  __shared__ int s_best;

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  for (int e = 0; e < b; ++e)
    if (plan.camera[e] == cam) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S;
  int32_t* __restrict__ g_person = plan.person + (long long)cam * S;
  int32_t* __restrict__ g_track = plan.track + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.last + (long long)cam * S;
  int32_t* __restrict__ g_hits = plan.hits + (long long)cam * S * 2;
  int32_t* g_hist = plan.hist + (long long)cam * S * 2 * BINS;
  int32_t* pairs = plan.pairs + (long long)b * MAXP * MAXS;
  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.next[cam];
    cam_state[2] = plan.dropped[cam];
  }

  for (int e = b; e < plan.d.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; cam_state is written
    const int n = plan.d.n[e];
    const int32_t* q_hist = plan.d.hist[e];
    const int frame = (int)((unsigned)cam_state[0] + 1u);

    // ---- 1: expire the slots; the poses ----
    if (tid < MAXS) {
      int person = 0, track = 0, last = 0, h0 = 0, h1 = 0;
      if (tid < S) {
        person = g_person[tid], track = g_track[tid], last = g_last[tid], h0 = g_hits[2 * tid], h1 = g_hits[2 * tid + 1];
        if (person != 0 && (long long)frame - last > plan.max_lost) person = 0;
      }
      s_person[tid] = person, s_track[tid] = track, s_last[tid] = last, s_hits[tid][0] = h0, s_hits[tid][1] = h1;
      s_born[tid] = 0;
    }
    if (tid < n) {
      int B[4], R[4];
      const bool ok = pose_usable(plan.d, e, tid, B);
      d_id[tid] = plan.ids[e][tid];
      d_part[tid] = ok ? 1 : 0;   // (usable; step 2 narrows it to the poses that take part)
#pragma unroll
      for (int i = 0; i < 4; ++i) d_box[tid][i] = B[i];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int count = plan.d.count[e][tid * 2 + r];
        d_count[tid][r] = count;
        if (count > 0 && ok && region_rect(plan.d, e, tid, r, B, R)) {
#pragma unroll
          for (int i = 0; i < 4; ++i) d_rect[tid][r][i] = R[i];
        } else {
          d_count[tid][r] = 0;
        }
      }
    }
    __syncthreads();

    // ---- 2: who takes part, and the slot bound to its track id ----
    int part = 0, slot = -1;
    if (tid < n) {
      const int id = d_id[tid];
      part = d_part[tid] != 0 && id >= 1;
      for (int p = 0; p < tid; ++p) part = part && !(d_id[p] == id && d_part[p] != 0);
      if (part)
        for (int t = S - 1; t >= 0; --t) slot = (s_person[t] != 0 && s_track[t] == id) ? t : slot;
    }
    __syncthreads();   // (every thread has read the usable flags)
    if (tid < n) {
      d_part[tid] = part;
      d_slot[tid] = slot;
      d_sim[tid] = 0;
      if (slot >= 0) s_last[slot] = frame;   // (track ids are bound once: one pose per slot)
    }
    __syncthreads();

    // ---- 3: candidates, pair scores, the greedy choice ----
    if (tid < MAXS) {
      int cand = tid < S && s_person[tid] != 0 && s_last[tid] < frame && s_hits[tid][0] >= plan.min_hits;
      for (int p = 0; p < n; ++p) cand = cand && !(d_part[p] != 0 && d_id[p] == s_track[tid]);
      s_cand[tid] = cand;
    }
    if (tid < 2 * n) {   // the overlap guard of (pose, region)
      const int p = tid >> 1, r = tid & 1;
      int skip = 0;
      if (d_count[p][r] > 0)
        for (int o = 0; o < n; ++o)
          skip |= o != p && d_part[o] != 0 && d_rect[p][r][0] <= d_box[o][2] && d_box[o][0] <= d_rect[p][r][2] &&
                  d_rect[p][r][1] <= d_box[o][3] && d_box[o][1] <= d_rect[p][r][3];
      d_skip[p][r] = skip;
    }
    __syncthreads();
    for (int i = tid; i < n * S; i += NT) {   // one pair per thread: its loads do not wait for another pair's sum
      const int p = i / S, t = i - p * S;
      int score = -1;
      if (d_part[p] != 0 && d_slot[p] < 0 && d_count[p][0] > 0 && s_cand[t] != 0) {
        const int regions = d_count[p][1] > 0 && s_hits[t][1] > 0 ? 2 : 1;
        int sum0 = 0, sum1 = 0;
        for (int r = 0; r < regions; ++r) {
          const int4* a = reinterpret_cast<const int4*>(q_hist + ((long long)p * 2 + r) * BINS);
          const int4* g = reinterpret_cast<const int4*>(g_hist + ((long long)t * 2 + r) * BINS);
          int acc = 0;
#pragma unroll 8
          for (int k = 0; k < BINS / 4; ++k) {
            const int4 x = a[k], y = g[k];
            acc += min(x.x, y.x) + min(x.y, y.y) + min(x.z, y.z) + min(x.w, y.w);
          }
          if (r == 0) sum0 = acc; else sum1 = acc;
        }
        score = regions == 2 ? (sum0 + sum1) >> 1 : sum0;
        score = min(max(score, 0), 65536);   // (a stored descriptor is whatever the state holds)
        if (score < plan.match_thr) score = -1;
      }
      pairs[p * MAXS + t] = score;
    }
    // the keys of this thread's pairs stay in registers: a round reads no global memory (a thread reads back what
    // it wrote itself), and a key whose pose or slot is taken is dead for good
    int keys[PAIRS_PER_THREAD];
#pragma unroll
    for (int k = 0; k < PAIRS_PER_THREAD; ++k) {
      const int i = tid + k * NT;
      keys[k] = -1;
      if (i < n * S) {
        const int p = i / S, t = i - p * S;
        const int score = pairs[p * MAXS + t];
        if (score >= 0) keys[k] = score * 16384 + (127 - p) * 128 + (127 - t);
      }
    }
    __syncthreads();
    for (int round = 0; round < MAXP; ++round) {
      if (tid == 0) s_best = -1;
      __syncthreads();
      int best = -1;
#pragma unroll
      for (int k = 0; k < PAIRS_PER_THREAD; ++k) {
        const int key = keys[k];
        if (key < 0) continue;
        if (d_slot[127 - ((key >> 7) & 127)] < 0 && s_cand[127 - (key & 127)] != 0) best = max(best, key);
        else keys[k] = -1;
      }
      if (best >= 0) atomicMax(&s_best, best);
      __syncthreads();
      const int key = s_best;
      if (key < 0) break;   // (block-uniform)
      __syncthreads();      // (every thread has read s_best before thread 0 of the next round resets it)
      if (tid == 0) {
        const int p = 127 - ((key >> 7) & 127), t = 127 - (key & 127);   // (a key is made of p < n and t < S)
        d_slot[p] = t;
        d_sim[p] = key >> 14;
        s_cand[t] = 0;
        s_track[t] = d_id[p];
        s_last[t] = frame;
      }
      __syncthreads();
    }
    __syncthreads();

    // ---- 4: the poses left over ----
    if (tid == 0) {
      int next = cam_state[1], dropped = cam_state[2];
      for (int p = 0; p < n; ++p) {
        if (d_part[p] == 0 || d_slot[p] >= 0) continue;
        int t = -1;
        for (int i = S - 1; i >= 0; --i) t = s_person[i] == 0 ? i : t;
        if (t < 0) {
          for (int i = 0; i < S; ++i)
            if (s_last[i] < frame && (t < 0 || s_last[i] < s_last[t])) t = i;   // (every slot is occupied here)
        }
        if (t < 0) {
          dropped = (int)((unsigned)dropped + 1u);
          continue;
        }
        d_slot[p] = t;
        s_person[t] = next;
        next = (int)((unsigned)next + 1u);
        s_track[t] = d_id[p];
        s_last[t] = frame;
        s_hits[t][0] = s_hits[t][1] = 0;
        s_born[t] = 1;
      }
      cam_state[0] = frame;
      cam_state[1] = next;
      cam_state[2] = dropped;
      plan.frame[cam] = frame;
      plan.next[cam] = next;
      plan.dropped[cam] = dropped;
    }
    __syncthreads();

    // ---- the descriptors: thread b moves bin b ----
    for (int p = 0; p < n; ++p) {
      const int t = d_slot[p];   // (in 0 .. S - 1 or -1: a loop counter of steps 2 .. 4)
      if (t < 0) continue;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        int32_t* g = g_hist + ((long long)t * 2 + r) * BINS + tid;
        if (d_count[p][r] > 0 && d_skip[p][r] == 0) {
          const int q = q_hist[((long long)p * 2 + r) * BINS + tid];
          if (s_hits[t][r] == 0) {
            *g = q;
          } else {
            const long long old = *g;
            *g = (int32_t)(old + ((((long long)q - old) * plan.gain + 8) >> 4));
          }
        } else if (s_born[t] != 0) {
          *g = 0;
        }
      }
    }
    __syncthreads();   // (s_hits was read by every thread)
    if (tid < n) {
      const int t = d_slot[tid];
      if (t >= 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (d_count[tid][r] > 0 && d_skip[tid][r] == 0) s_hits[t][r] = min(s_hits[t][r] + 1, PAVE_REID_MAX_HITS);
      }
      plan.out_ids[e][tid] = t >= 0 ? s_person[t] : 0;
      plan.out_sim[e][tid] = d_sim[tid];
    }
    __syncthreads();
    if (tid < S) {
      g_person[tid] = s_person[tid];
      g_track[tid] = s_track[tid];
      g_last[tid] = s_last[tid];
      g_hits[2 * tid] = s_hits[tid][0];
      g_hits[2 * tid + 1] = s_hits[tid][1];
    }
  }
}

int check_describe(const pave_reid_describe_plan* plan, const bool bgr, const char* who) {
  static thread_local char msg[96];
  const char* bad = nullptr;
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES) bad = "1 .. 32 entries per launch";
  else if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) bad = "K outside 1 .. 32";
  for (int r = 0; r < 2 && !bad; ++r)
    for (int h = 0; h < 2 && !bad; ++h) {
      if (plan->n_part[r][h] < 0 || plan->n_part[r][h] > PAVE_REID_MAX_PART) bad = "n_part outside 0 .. 4";
      for (int i = 0; !bad && i < plan->n_part[r][h]; ++i)
        if (plan->part[r][h][i] < 0 || plan->part[r][h][i] >= plan->K) bad = "a part key point outside [0, K)";
    }
  for (int i = 0; !bad && i < plan->entries; ++i) {
    const int n = plan->n[i], W = plan->width[i], H = plan->height[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) bad = "N outside 0 .. 128";
    else if (!plan->src[i]) bad = "null surface";
    else if (!plan->hist[i] || !plan->count[i]) bad = "null hist or count tensor";
    else if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) bad = "null pose tensor";
    else if (W < 1 || W > MAX_SIZE || H < 1 || H > MAX_SIZE) bad = "width or height outside 1 .. 8192";
    else if (!bgr && ((W | H) & 1)) bad = "odd NV12 sizes";
    else if (bgr ? plan->pitch[i] != 3 * W : plan->pitch[i] < W) bad = "a pitch that does not fit a row's bytes";
    else if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      bad = "scale must be positive and finite";
  }
  if (!bad) return PAVE_OK;
  snprintf(msg, sizeof msg, "%s: %s", who, bad);
  return pave_internal_fail(PAVE_E_ARG, msg);
}

int check_update(const pave_reid_plan* plan, const char* who) {
  static thread_local char msg[96];
  const char* bad = nullptr;
  if (!plan->person || !plan->track || !plan->last || !plan->hits || !plan->hist || !plan->frame || !plan->next || !plan->dropped)
    bad = "null gallery tensor";
  else if (!plan->pairs) bad = "null pairs area";
  else if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS) bad = "max_people outside 1 .. 128";
  else if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS) bad = "cameras outside 1 .. 4096";
  else if (plan->max_lost < 0) bad = "max_lost below 0";
  else if (plan->match_thr < 0 || plan->match_thr > PAVE_REID_NEVER) bad = "match_thr outside 0 .. 65537";
  else if (plan->min_hits < 1 || plan->min_hits > PAVE_REID_MAX_HITS) bad = "min_hits outside 1 .. 32767";
  else if (plan->gain < 1 || plan->gain > 16) bad = "gain outside 1 .. 16";
  for (int i = 0; !bad && i < plan->d.entries; ++i) {
    if (plan->d.n[i] > 0 && (!plan->ids[i] || !plan->out_ids[i] || !plan->out_sim[i])) bad = "null ids or output tensor";
    else if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras) bad = "a camera index outside [0, cameras)";
  }
  if (!bad) return PAVE_OK;
  snprintf(msg, sizeof msg, "%s: %s", who, bad);
  return pave_internal_fail(PAVE_E_ARG, msg);
}

template <bool BGR>
int describe(const pave_reid_describe_plan* plan, void* stream, const char* who) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "reid: null plan");
  if (const int st = check_describe(plan, BGR, who)) return st;
  int most = 0;
  for (int i = 0; i < plan->entries; ++i) most = plan->n[i] > most ? plan->n[i] : most;
  if (most == 0) return PAVE_OK;
  return pave_launch<reid_describe_kernel<BGR>>(dim3(2u * (unsigned)most, (unsigned)plan->entries), dim3(NT), 0,
                                                reinterpret_cast<hipStream_t>(stream), *plan);
}

template <bool BGR>
int update(const pave_reid_plan* plan, void* stream, const char* who) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "reid: null plan");
  if (const int st = check_describe(&plan->d, BGR, who)) return st;
  if (const int st = check_update(plan, who)) return st;
  if (const int st = describe<BGR>(&plan->d, stream, who)) return st;
  return pave_launch<reid_link_kernel>(dim3((unsigned)plan->d.entries), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream),
                                       *plan);
}

}  // namespace

extern "C" {

int pave_reid_describe_nv12(const pave_reid_describe_plan* plan, void* stream) {
  return describe<false>(plan, stream, "reid_describe_nv12");
}
int pave_reid_describe_bgr(const pave_reid_describe_plan* plan, void* stream) {
  return describe<true>(plan, stream, "reid_describe_bgr");
}
int pave_reid_update_nv12(const pave_reid_plan* plan, void* stream) { return update<false>(plan, stream, "reid_update_nv12"); }
int pave_reid_update_bgr(const pave_reid_plan* plan, void* stream) { return update<true>(plan, stream, "reid_update_bgr"); }

}  // extern "C"
