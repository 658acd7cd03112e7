// Track trails for the live path: the recent path of every tracked person, kept per camera in a ring of points per
// slot on the device, in one launch for up to 32 frames of any number of cameras (pave_trail_update), and the paths as
// tapered lines drawn into decoder-style surfaces (pave_draw_trails_nv12: pitched NV12; pave_draw_trails_bgr: [H, W,
// 3] BGR).
//
// Both rules are DESIGN section 22 and are integer-exact.
//   update: section 17's poses, slots and 1/8-pixel anchor (pave_tracked.h).  Per frame: the clock advances and slots not
//     seen for more than max_age frames are freed; poses find or take slots; a birth starts the ring with the anchor
//     (head 0, count 1); a slot that was there takes the anchor as pos and, when the newest committed point is at
//     least `stride` frames old and at least min_step away (Chebyshev), commits it: head = (head + 1) % L, count =
//     min(count + 1, L).  box is the min / max over the committed points and pos.  The outputs are the slot's count,
//     the frames since its oldest committed point, floor |pos - oldest| and the sum of floor |step| along the
//     committed points to pos.
//   draw: a point in quarter pixels is clamp(p >> 1, 0, 32767); with n = count and p_0 .. p_{n-1} the committed points,
//     oldest first, p_n = pos, capsule j runs from p_j to p_{j+1} with radius 2 T_tail + floor(2 (T - T_tail)(j + 1) /
//     n), and (head_radius > 0) disc j = n lies at pos; pave_draw.hip's coverage rule; a pixel takes the colour of the
//     covering primitive with the largest (id, j), an NV12 chroma sample the largest over its 2 x 2 luma pixels.
//
// Update: one block of 256 threads per camera of the launch (pave_tracked.h), which takes that camera's entries in
// plan order with a block barrier between them; launches on one stream follow each other.  A slot has at most one
// pose per frame (the first valid pose of its id), so its ring has one writer.  head and count live in device memory:
// wherever they index the ring they are first reduced, (unsigned)head % L and count clamped to 1 .. L, and the walk
// over the ring is bounded by that count: no bit pattern in the state can make an access leave the ring.
//
// Draw: pave_draw.hip's tile scheme: 256 threads own a 32 x 32 pixel tile, a thread one 2 x 2 block of it (and, NV12,
// its chroma sample), so every output byte has one writer and a byte no primitive covers is never written.  One lane
// per slot culls by box >> 1 grown by the largest radius into an LDS list; a tile no slot touches returns before any
// write.  The block then walks slots-on-the-tile x (L + 1) primitives 256 at a time: a lane builds one primitive from
// the ring, culls it against the tile and appends it to a 256-entry LDS list of 16-byte candidates, and after a
// barrier every lane tests its four pixels against the list (all lanes read one entry: an LDS broadcast of one
// 128-bit read).  The round count is bounded by S (L + 1) / 256 from the plan, at most 33.  Every loop bound is from
// the plan or the header's maxima, every barrier is block-uniform, and there are no global atomics and no scratch.
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
constexpr int MAXL = PAVE_TRAIL_MAX_POINTS;
constexpr int TILE = 32;                             // pixels per tile edge of the draw kernels
static_assert(MAXP <= NT && MAXS <= NT && MAXL < 128, "thread roles; the key (id, j) as id * 128 + j");

// floor(sqrt(dx^2 + dy^2)).  The rule's own operands are below 2^34, where the double square root is exact enough
// for its floor to be right; the two corrections make the result the floor whatever the rounding, and the unsigned
// arithmetic is defined for any words a state could hold.
__device__ __forceinline__ int step_length(const int ax, const int ay, const int bx, const int by) {
  const unsigned long long dx = (unsigned long long)((long long)ax - bx), dy = (unsigned long long)((long long)ay - by);
  const unsigned long long d2 = dx * dx + dy * dy;
  unsigned long long r = (unsigned long long)sqrt((double)d2);
  if (r * r > d2) --r;
  if ((r + 1) * (r + 1) <= d2) ++r;
  return (int)r;
}

__global__ __launch_bounds__(NT) void trail_update_kernel(const pave_trail_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int det_id[MAXP];
  __shared__ int det_bad[MAXP];      // != 0: a coordinate that is not finite
  __shared__ int det_ok[MAXP];       // != 0: keep and a box score above the threshold
  __shared__ int det_slot[MAXP];     // the slot of a pose that takes part, or -1
  __shared__ int det_born[MAXP];     // != 0: the slot was born in this frame
  __shared__ int cam_state[2];       // frame, dropped

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S, K = plan.K, L = plan.L;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_pos = plan.slot_pos + (long long)cam * S * 2;
  int32_t* __restrict__ g_head = plan.slot_head + (long long)cam * S;
  int32_t* __restrict__ g_count = plan.slot_count + (long long)cam * S;
  int32_t* __restrict__ g_box = plan.slot_box + (long long)cam * S * 4;
  int32_t* g_pts = plan.pts + (long long)cam * S * L * 2;
  int32_t* g_when = plan.when + (long long)cam * S * L;

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
    const int frame = (int)((unsigned)cam_state[0] + 1u);

    // ---- 1: expire the slots; the poses' boxes ----
    if (tid < MAXS) expire_slot(plan, g_id, g_last, slot_id, tid, S, frame);
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

    // ---- 3, 4, 5: pose tid in its slot: anchor, commit, box, outputs ----
    if (tid < n) {
      int o_count = 0, o_span = 0, o_dist = 0, o_path = 0;
      const int t = det_slot[tid];   // (in 0 .. S - 1 or -1: a slot index is a loop counter of step 2)
      if (t >= 0) {
        long long lx, ly;
        anchor(plan, kpts, tid, K, sx, sy, X1, Y1, X2, Y2, lx, ly);
        const int ax = (int)lx, ay = (int)ly;   // (0 .. 65534)
        int32_t* ring = g_pts + (long long)t * L * 2;
        int32_t* ring_when = g_when + (long long)t * L;
        int head = 0, count = 1;
        if (det_born[tid] != 0) {
          ring[0] = ax;
          ring[1] = ay;
          ring_when[0] = frame;
        } else {
          head = (int)((unsigned)g_head[t] % (unsigned)L);
          count = min(max(g_count[t], 1), L);
          const long long ddx = (long long)ax - ring[2 * head], ddy = (long long)ay - ring[2 * head + 1];
          const long long step = max(ddx < 0 ? -ddx : ddx, ddy < 0 ? -ddy : ddy);
          if ((long long)frame - ring_when[head] >= plan.stride && step >= plan.min_step) {
            head = head + 1 == L ? 0 : head + 1;
            ring[2 * head] = ax;
            ring[2 * head + 1] = ay;
            ring_when[head] = frame;
            count = min(count + 1, L);
          }
        }
        // the committed points, oldest first: the box, the path
        int i = (head + L - count + 1) % L;   // (head < L, 1 <= count <= L: the sum is in 1 .. 2 L - 1)
        o_count = count;
        o_span = (int)((unsigned)frame - (unsigned)ring_when[i]);
        o_dist = step_length(ax, ay, ring[2 * i], ring[2 * i + 1]);
        int bx0 = ax, by0 = ay, bx1 = ax, by1 = ay, qx = 0, qy = 0;
        for (int j = 0; j < count; ++j) {
          const int cx = ring[2 * i], cy = ring[2 * i + 1];
          bx0 = min(bx0, cx), by0 = min(by0, cy), bx1 = max(bx1, cx), by1 = max(by1, cy);
          if (j > 0) o_path = (int)((unsigned)o_path + (unsigned)step_length(cx, cy, qx, qy));
          qx = cx, qy = cy;
          i = i + 1 == L ? 0 : i + 1;
        }
        o_path = (int)((unsigned)o_path + (unsigned)step_length(ax, ay, qx, qy));
        g_head[t] = head;
        g_count[t] = count;
        g_pos[2 * t] = ax;
        g_pos[2 * t + 1] = ay;
        g_box[4 * t] = bx0, g_box[4 * t + 1] = by0, g_box[4 * t + 2] = bx1, g_box[4 * t + 3] = by1;
        g_last[t] = frame;
      }
      plan.out_count[e][tid] = o_count;
      plan.out_span[e][tid] = o_span;
      plan.out_dist[e][tid] = o_dist;
      plan.out_path[e][tid] = o_path;
    }
  }
}

// ---- the trails in the picture ----

struct alignas(16) Cand {        // one candidate of the tile's list: one 128-bit LDS read
  short ax, ay, bx, by;          // quarter pixels
  int id;
  short r;                       // quarter pixels
  unsigned char j, col;          // the primitive's index in its trail; the palette row
};
static_assert(sizeof(Cand) == 16, "one ds_read_b128 per candidate");

// pave_draw.hip's coverage rule, all terms in int64 (|w x d| <= 2^31, its square < 2^63).
__device__ __forceinline__ bool covers(const int X, const int Y, const int ax, const int ay, const int dx, const int dy,
                                       const long long L2, const long long r2, const long long r2L2) {
  const int wx = X - ax, wy = Y - ay;
  const long long t = (long long)wx * dx + (long long)wy * dy;
  if (t <= 0) return (long long)wx * wx + (long long)wy * wy <= r2;
  if (t >= L2) {
    const int ex = wx - dx, ey = wy - dy;
    return (long long)ex * ex + (long long)ey * ey <= r2;
  }
  const long long c = (long long)wx * dy - (long long)wy * dx;
  return c * c <= r2L2;
}

// 1/8 pixel -> quarter pixels; the clamp changes nothing for a point the update wrote (0 .. 65534).
__device__ __forceinline__ int quarter(const int p) { return min(max(p >> 1, 0), QMAX); }

// BGR = 0: NV12 (dst = H rows of Y, then H / 2 rows of interleaved U, V; pitch bytes per row).
// BGR = 1: [H, W, 3] bytes, pitch bytes per row.  The surface is blockIdx.z.
template <int BGR>
__global__ __launch_bounds__(256) void draw_trails_kernel(const pave_trail_draw_plan plan) {
  __shared__ unsigned char slot_list[MAXS];
  __shared__ Cand cand[256];
  __shared__ int n_slot, n_cand[2];
  __shared__ unsigned char color[PAVE_DRAW_PALETTE][4];

  const int s = blockIdx.z;
  const int W = plan.width[s], H = plan.height[s];
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  if (x0 >= W || y0 >= H) return;   // (block-uniform: before any barrier)
  const int tid = threadIdx.x;
  const int cam = plan.camera[s], S = plan.S, L = plan.L;
  const int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  const int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  const int32_t* __restrict__ g_pos = plan.slot_pos + (long long)cam * S * 2;
  const int32_t* __restrict__ g_head = plan.slot_head + (long long)cam * S;
  const int32_t* __restrict__ g_count = plan.slot_count + (long long)cam * S;
  const int32_t* __restrict__ g_box = plan.slot_box + (long long)cam * S * 4;
  const int32_t* __restrict__ g_pts = plan.pts + (long long)cam * S * L * 2;
  const int32_t* __restrict__ g_when = plan.when + (long long)cam * S * L;
  const int frame = plan.frame[cam];
  const int T = plan.thickness, Tt = plan.thickness_tail;
  const int rk = 4 * plan.head_radius, rmax = max(2 * T, rk);
  // the tile's pixels as points, clipped to the surface
  const int tx0 = 4 * x0, ty0 = 4 * y0, tx1 = 4 * (min(x0 + TILE, W) - 1), ty1 = 4 * (min(y0 + TILE, H) - 1);

  if (tid == 0) { n_slot = 0; n_cand[0] = 0; n_cand[1] = 0; }
  __syncthreads();

  // ---- slots on the tile: one lane per slot ----
  if (tid < S) {
    const bool drawn = g_id[tid] != 0 && (plan.linger < 0 || (long long)frame - g_last[tid] <= plan.linger);
    const int bx0 = g_box[4 * tid] >> 1, by0 = g_box[4 * tid + 1] >> 1;
    const int bx1 = g_box[4 * tid + 2] >> 1, by1 = g_box[4 * tid + 3] >> 1;
    if (drawn && (long long)bx0 - rmax <= tx1 && (long long)bx1 + rmax >= tx0 && (long long)by0 - rmax <= ty1 &&
        (long long)by1 + rmax >= ty0)
      slot_list[atomicAdd(&n_slot, 1)] = (unsigned char)tid;   // (tid < S <= 128 entries)
  }
  __syncthreads();
  const int ns = n_slot;
  if (ns == 0) return;   // (block-uniform)

  if (tid < PAVE_DRAW_PALETTE) {
    const int tab = plan.table[s];
    color[tid][0] = plan.palette[tab][tid][0];
    color[tid][1] = plan.palette[tab][tid][1];
    color[tid][2] = plan.palette[tab][tid][2];
  }

  // this lane's 2 x 2 pixels
  const int px = x0 + 2 * (tid & 15), py = y0 + 2 * (tid >> 4);
  constexpr long long NONE = INT64_MIN;
  long long best00 = NONE, best01 = NONE, best10 = NONE, best11 = NONE;   // [row][column]: keys id * 128 + j
  int col00 = 0, col01 = 0, col10 = 0, col11 = 0;

  const int PW = L + 1;                            // primitives walked per slot: L capsules at the most and the disc
  const int total = ns * PW;
  const int max_rounds = (S * PW + 255) / 256;     // from the plan alone
  for (int round = 0; round < max_rounds; ++round) {
    const int base = round * 256;
    if (base >= total) break;   // (block-uniform)
    const int cur = round & 1;
    if (tid == 0) n_cand[cur ^ 1] = 0;   // next round's counter: last read before this round's first barrier
    // -- build and cull one primitive --
    const int k = base + tid;
    if (k < total) {
      const int si = k / PW, local = k - si * PW;
      const int t = slot_list[si];                                     // (< S)
      const int head = (int)((unsigned)g_head[t] % (unsigned)L);
      const int n = min(max(g_count[t], 1), L);
      const int32_t* ring = g_pts + (long long)t * L * 2;
      const int hx = quarter(g_pos[2 * t]), hy = quarter(g_pos[2 * t + 1]);
      int ax = hx, ay = hy, bx = hx, by = hy, r = rk;
      bool on = local == n && rk > 0;
      if (local < n) {
        const int i = (head + L - n + 1 + local) % L;                  // (the sum is in 1 .. 3 L - 2)
        ax = quarter(ring[2 * i]);
        ay = quarter(ring[2 * i + 1]);
        if (local + 1 < n) {
          const int i1 = i + 1 == L ? 0 : i + 1;
          bx = quarter(ring[2 * i1]);
          by = quarter(ring[2 * i1 + 1]);
        }
        r = 2 * Tt + 2 * (T - Tt) * (local + 1) / n;
        on = plan.tail_frames == 0 || (long long)frame - g_when[(long long)t * L + i] <= plan.tail_frames;
      }
      if (on && min(ax, bx) - r <= tx1 && max(ax, bx) + r >= tx0 && min(ay, by) - r <= ty1 && max(ay, by) + r >= ty0) {
        Cand c;
        c.ax = (short)ax; c.ay = (short)ay; c.bx = (short)bx; c.by = (short)by;
        c.id = g_id[t];
        c.r = (short)r;
        c.j = (unsigned char)local;
        c.col = (unsigned char)(((unsigned)c.id - 1u) % PAVE_DRAW_PALETTE);
        cand[atomicAdd(&n_cand[cur], 1)] = c;   // (a round appends at most 256)
      }
    }
    __syncthreads();
    // -- every lane's four pixels against the round's list --
    const int nc = n_cand[cur];
    for (int i = 0; i < nc; ++i) {
      const Cand c = cand[i];
      const long long key = (long long)c.id * 128 + c.j;
      const int dx = c.bx - c.ax, dy = c.by - c.ay;
      const long long L2 = (long long)dx * dx + (long long)dy * dy;
      const long long r2 = (long long)c.r * c.r, r2L2 = r2 * L2;
      const int X = 4 * px, Y = 4 * py;
      if (key > best00 && covers(X, Y, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best00 = key; col00 = c.col; }
      if (key > best01 && covers(X + 4, Y, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best01 = key; col01 = c.col; }
      if (key > best10 && covers(X, Y + 4, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best10 = key; col10 = c.col; }
      if (key > best11 && covers(X + 4, Y + 4, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best11 = key; col11 = c.col; }
    }
    __syncthreads();
  }

  // ---- the stores: covered bytes only ----
  unsigned char* __restrict__ dst = static_cast<unsigned char*>(plan.dst[s]);
  const long long pitch = plan.pitch[s];
  if (BGR) {
    if (px < W && py < H && best00 != NONE) {
      unsigned char* o = dst + py * pitch + 3 * px;
      o[0] = color[col00][0]; o[1] = color[col00][1]; o[2] = color[col00][2];
    }
    if (px + 1 < W && py < H && best01 != NONE) {
      unsigned char* o = dst + py * pitch + 3 * (px + 1);
      o[0] = color[col01][0]; o[1] = color[col01][1]; o[2] = color[col01][2];
    }
    if (px < W && py + 1 < H && best10 != NONE) {
      unsigned char* o = dst + (py + 1) * pitch + 3 * px;
      o[0] = color[col10][0]; o[1] = color[col10][1]; o[2] = color[col10][2];
    }
    if (px + 1 < W && py + 1 < H && best11 != NONE) {
      unsigned char* o = dst + (py + 1) * pitch + 3 * (px + 1);
      o[0] = color[col11][0]; o[1] = color[col11][1]; o[2] = color[col11][2];
    }
  } else if (px < W && py < H) {   // W and H are even: the 2 x 2 block is inside or outside as a whole
    unsigned char* y = dst + py * pitch + px;
    if (best00 != NONE) y[0] = color[col00][0];
    if (best01 != NONE) y[1] = color[col01][0];
    if (best10 != NONE) y[pitch] = color[col10][0];
    if (best11 != NONE) y[pitch + 1] = color[col11][0];
    long long m = best00;
    int mc = col00;
    if (best01 > m) { m = best01; mc = col01; }
    if (best10 > m) { m = best10; mc = col10; }
    if (best11 > m) { m = best11; mc = col11; }
    if (m != NONE) {
      unsigned char* uv = dst + ((long long)H + (py >> 1)) * pitch + px;
      uv[0] = color[mc][1];
      uv[1] = color[mc][2];
    }
  }
}

// Everything a draw plan could get wrong, before any device call.  bpp: bytes per pixel of a row (1 = NV12, 3 = BGR).
int trail_draw_check(const pave_trail_draw_plan* plan, const int bpp, int* max_w, int* max_h) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "draw_trails: null plan");
  if (plan->n < 1 || plan->n > PAVE_DRAW_MAX_SURFACES)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: 1 .. 32 surfaces per launch");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_pos || !plan->slot_head || !plan->slot_count || !plan->slot_box ||
      !plan->pts || !plan->when || !plan->frame)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: null state tensor");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: cameras outside 1 .. 4096");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: max_tracks outside 1 .. 128");
  if (plan->L < 1 || plan->L > PAVE_TRAIL_MAX_POINTS) return pave_internal_fail(PAVE_E_ARG, "draw_trails: length outside 1 .. 64");
  if (plan->thickness < 1 || plan->thickness > PAVE_TRAIL_MAX_THICKNESS || plan->thickness_tail < 1 ||
      plan->thickness_tail > plan->thickness)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: thickness in 1 .. 32 and thickness_tail in 1 .. thickness");
  if (plan->head_radius < 0 || plan->head_radius > PAVE_TRAIL_MAX_RADIUS)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: head_radius outside 0 .. 32");
  if (plan->tail_frames < 0 || plan->tail_frames > PAVE_TRAIL_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: tail_frames outside 0 .. 2^30");
  if (plan->linger < -1 || plan->linger > PAVE_TRAIL_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "draw_trails: linger outside -1 .. 2^30");
  *max_w = *max_h = 0;
  for (int i = 0; i < plan->n; ++i) {
    const int w = plan->width[i], h = plan->height[i];
    if (!plan->dst[i]) return pave_internal_fail(PAVE_E_ARG, "draw_trails: null surface");
    if (w < 1 || h < 1 || w > PAVE_DRAW_MAX_SIZE || h > PAVE_DRAW_MAX_SIZE)
      return pave_internal_fail(PAVE_E_ARG, "draw_trails: width and height in 1 .. 8192");
    if (bpp == 1 && ((w | h) & 1)) return pave_internal_fail(PAVE_E_ARG, "draw_trails: NV12 width and height must be even");
    if (plan->pitch[i] < bpp * w) return pave_internal_fail(PAVE_E_ARG, "draw_trails: pitch below the bytes of a row");
    if (plan->table[i] >= PAVE_DRAW_MAX_TABLES) return pave_internal_fail(PAVE_E_ARG, "draw_trails: palette table index >= 4");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "draw_trails: a camera index outside [0, cameras)");
    *max_w = w > *max_w ? w : *max_w;
    *max_h = h > *max_h ? h : *max_h;
  }
  return PAVE_OK;
}

template <int BGR>
int trail_draw_launch(const pave_trail_draw_plan* plan, void* stream) {
  int w = 0, h = 0;
  const int st = trail_draw_check(plan, BGR ? 3 : 1, &w, &h);
  if (st != PAVE_OK) return st;
  return pave_launch<draw_trails_kernel<BGR>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                    (unsigned)plan->n),
                                               dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // namespace

extern "C" {

int pave_trail_update(const pave_trail_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "trail_update: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "trail_update: K outside 1 .. 32");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_pos || !plan->slot_head || !plan->slot_count || !plan->slot_box ||
      !plan->pts || !plan->when || !plan->frame || !plan->dropped)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: null state tensor");
  if (plan->L < 1 || plan->L > PAVE_TRAIL_MAX_POINTS) return pave_internal_fail(PAVE_E_ARG, "trail_update: length outside 1 .. 64");
  if (plan->stride < 1 || plan->stride > PAVE_TRAIL_MAX_STRIDE)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: stride outside 1 .. 255");
  if (plan->min_step < 0 || plan->min_step > PAVE_TRAIL_MAX_STEP)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: min_step outside 0 .. 65535");
  if (plan->anchor < PAVE_ZONE_ANCHOR_FEET || plan->anchor > PAVE_ZONE_ANCHOR_CENTRE)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: anchor outside 0 .. 2");
  if (plan->n_anchor < 0 || plan->n_anchor > PAVE_ZONE_MAX_ANCHOR_KPTS)
    return pave_internal_fail(PAVE_E_ARG, "trail_update: n_anchor outside 0 .. 4");
  for (int i = 0; i < plan->n_anchor; ++i)
    if (plan->anchor_kpt[i] < 0 || plan->anchor_kpt[i] >= plan->K)
      return pave_internal_fail(PAVE_E_ARG, "trail_update: an anchor key point outside [0, K)");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "trail_update: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "trail_update: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "trail_update: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "trail_update: null ids tensor");
    if (n > 0 && (!plan->out_count[i] || !plan->out_span[i] || !plan->out_dist[i] || !plan->out_path[i]))
      return pave_internal_fail(PAVE_E_ARG, "trail_update: null output tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "trail_update: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "trail_update: scale must be positive and finite");
  }
  return pave_launch<trail_update_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                          reinterpret_cast<hipStream_t>(stream), *plan);
}

int pave_draw_trails_nv12(const pave_trail_draw_plan* plan, void* stream) { return trail_draw_launch<0>(plan, stream); }

int pave_draw_trails_bgr(const pave_trail_draw_plan* plan, void* stream) { return trail_draw_launch<1>(plan, stream); }

}  // extern "C"
