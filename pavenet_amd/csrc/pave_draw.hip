// The way back out of the live path: poses drawn into decoder-style surfaces on the device, in one launch for up
// to 32 separately allocated surfaces (pave_draw_poses_nv12: pitched NV12; pave_draw_poses_bgr: [H, W, 3] BGR).
//
// The rule is DESIGN section 13 and is integer-exact.  A coordinate becomes quarter pixels,
//   X = clamp((int)rintf((x / sx) * 4.f), 0, 32767)     (correctly rounded division, no contraction),
// pixel (px, py) is the point (4 px, 4 py).  Pose p is drawn iff keep[p] != 0 (when keep is given), its box score is
// > score_thr and its 2 K + 4 coordinates are finite; its primitives are, in this local order, the 4 box edges
// (draw_boxes; radius 2 thickness), the E limbs (both ends' scores > kpt_thr; radius 2 thickness) and the K discs
// (score > kpt_thr; A = B, radius 4 radius), with id = p (4 + E + K) + local index.  A capsule (A, B, r) covers P
// iff, in int64 with d = B - A, w = P - A, L2 = d.d, t = w.d:
//   t <= 0: |w|^2 <= r^2;   t >= L2: |P - B|^2 <= r^2;   else (w x d)^2 <= r^2 L2,
// and a pixel takes the colour of the covering primitive with the LARGEST id: a painter's order that does not depend
// on the order of evaluation.  An NV12 chroma sample takes the largest id over its 2 x 2 luma pixels.  The kernel
// does no colour arithmetic: the plan carries the bytes to store.
//
// 256 threads own a 32 x 32 pixel tile, a thread one 2 x 2 block of it (and, NV12, its chroma sample): every output
// byte has exactly one writer and a byte no primitive covers is never written.  The block culls poses by the
// bounding box of their quantised points grown by the larger radius (one lane per pose) into an LDS list, then walks
// poses-on-the-tile x primitives 256 at a time: a lane builds one primitive, culls it against the tile and appends
// the survivors to a 256-entry LDS list (append order is irrelevant under the max-id rule), and after a barrier
// every lane tests its four pixels against that list (all lanes read one entry: an LDS broadcast).  A round appends
// at most 256 entries, so the list cannot overflow; the round count is bounded by N (4 + E + K) / 256 from the plan
// and every loop bound and barrier is block-uniform.  No global atomics, no scratch; a tile no pose touches ends
// after the pose cull without a write.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"

namespace {

constexpr int TILE = 32;        // pixels per tile edge
constexpr int QMAX = 32767;     // the largest quarter-pixel coordinate

struct Prim {                   // one candidate of the tile's list
  short ax, ay, bx, by;
  int id;
  short r;                      // quarter pixels
  short col;                    // row of the plan's colour table
};

// A coordinate in quarter pixels.  The clamp is made in float, where it is the same function for every finite
// quotient and defined for an infinite one (a finite x over a tiny scale).
__device__ __forceinline__ int quant(const float x, const float s) {
#pragma clang fp contract(off)
  const float q = __fdiv_rn(x, s);
  const float v = q * 4.f;
  return (int)fminf(fmaxf(rintf(v), 0.f), (float)QMAX);
}

__device__ __forceinline__ bool finite4(const float a, const float b, const float c, const float d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

// The coverage rule, all terms in int64 (|w x d| <= 2^31, its square < 2^63).
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

// BGR = 0: NV12 (dst = H rows of Y, then H / 2 rows of interleaved U, V; pitch bytes per row).
// BGR = 1: [H, W, 3] bytes, pitch bytes per row.
// The surface is blockIdx.z: what a block reads from the by-value plan by surface is wave-uniform (scalar loads
// from the kernel arguments).  The two tables a lane indexes by itself (edges, colours) are read once per block,
// one entry per lane, into LDS: vector loads from the kernel-argument segment, no copy of the plan to scratch.
template <int BGR>
__global__ __launch_bounds__(256) void draw_poses_kernel(const pave_draw_plan plan) {
  __shared__ unsigned short pose_list[PAVE_DRAW_MAX_POSES];
  __shared__ Prim cand[256];
  __shared__ int n_pose, n_cand[2];
  __shared__ unsigned char edge[PAVE_DRAW_MAX_E][2];
  __shared__ unsigned char color[PAVE_DRAW_COLORS][4];

  const int s = blockIdx.z;
  const int W = plan.width[s], H = plan.height[s], N = plan.n_poses[s];
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  if (x0 >= W || y0 >= H || N <= 0) return;   // (block-uniform: before any barrier)
  const int tid = threadIdx.x;
  const int K = plan.K, E = plan.E, PP = 4 + E + K;
  const float sx = plan.scale[s][0], sy = plan.scale[s][1];
  const float* __restrict__ kpts = plan.kpts[s];
  const float* __restrict__ bboxes = plan.bboxes[s];
  const int32_t* __restrict__ keep = plan.keep[s];
  const int rl = 2 * plan.thickness, rk = 4 * plan.radius, rmax = max(rl, rk);
  const int boxes = plan.draw_boxes;
  // the tile's pixels as points, clipped to the surface
  const int tx0 = 4 * x0, ty0 = 4 * y0, tx1 = 4 * (min(x0 + TILE, W) - 1), ty1 = 4 * (min(y0 + TILE, H) - 1);

  if (tid == 0) { n_pose = 0; n_cand[0] = 0; n_cand[1] = 0; }
  __syncthreads();

  // ---- poses on the tile: one lane per pose ----
  for (int base = 0; base < N; base += 256) {
    const int p = base + tid;
    if (p < N) {
      const float* bb = bboxes + (long long)p * 5;
      const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
      bool drawn = (keep == nullptr || keep[p] != 0) && bb[4] > plan.score_thr && finite4(b0, b1, b2, b3);
      if (drawn) {
        int lox = QMAX, loy = QMAX, hix = 0, hiy = 0;
        const float* kp = kpts + (long long)p * K * 3;
        for (int k = 0; k < K; ++k) {
          const float x = kp[3 * k], y = kp[3 * k + 1];
          drawn = drawn && isfinite(x) && isfinite(y);
          const int X = quant(x, sx), Y = quant(y, sy);
          lox = min(lox, X); hix = max(hix, X);
          loy = min(loy, Y); hiy = max(hiy, Y);
        }
        if (boxes) {
          const int X1 = quant(b0, sx), Y1 = quant(b1, sy), X2 = quant(b2, sx), Y2 = quant(b3, sy);
          lox = min(lox, min(X1, X2)); hix = max(hix, max(X1, X2));
          loy = min(loy, min(Y1, Y2)); hiy = max(hiy, max(Y1, Y2));
        }
        if (drawn && lox - rmax <= tx1 && hix + rmax >= tx0 && loy - rmax <= ty1 && hiy + rmax >= ty0)
          pose_list[atomicAdd(&n_pose, 1)] = (unsigned short)p;
      }
    }
  }
  __syncthreads();
  const int np = n_pose;
  if (np == 0) return;   // (block-uniform)

  // ---- the tables a lane indexes by itself ----
  const int tab = plan.table[s];
  if (tid < E) { edge[tid][0] = plan.edge[tid][0]; edge[tid][1] = plan.edge[tid][1]; }
  if (tid >= 64 && tid < 64 + PAVE_DRAW_COLORS) {
    const int i = tid - 64;
    color[i][0] = plan.color[tab][i][0];
    color[i][1] = plan.color[tab][i][1];
    color[i][2] = plan.color[tab][i][2];
  }
  __syncthreads();

  // this lane's 2 x 2 pixels
  const int px = x0 + 2 * (tid & 15), py = y0 + 2 * (tid >> 4);
  int best00 = -1, best01 = -1, best10 = -1, best11 = -1;   // [row][column]
  int col00 = 0, col01 = 0, col10 = 0, col11 = 0;

  const int total = np * PP;
  const int max_rounds = (N * PP + 255) / 256;   // from the plan alone
  for (int round = 0; round < max_rounds; ++round) {
    const int base = round * 256;
    if (base >= total) break;   // (block-uniform)
    const int cur = round & 1;
    if (tid == 0) n_cand[cur ^ 1] = 0;   // next round's counter: last read before this round's first barrier
    // -- build and cull one primitive --
    const int j = base + tid;
    if (j < total) {
      const int slot = j / PP, local = j - slot * PP;
      const int p = pose_list[slot];
      int ax, ay, bx, by, r, col;
      bool on = true;
      if (local < 4) {
        const float* bb = bboxes + (long long)p * 5;
        const int X1 = quant(bb[0], sx), Y1 = quant(bb[1], sy), X2 = quant(bb[2], sx), Y2 = quant(bb[3], sy);
        // top, right, bottom, left
        ax = (local == 0 || local == 3) ? X1 : X2;
        ay = (local < 2) ? Y1 : Y2;
        bx = (local < 2) ? X2 : X1;
        by = (local == 0 || local == 3) ? Y1 : Y2;
        r = rl;
        col = 0;
        on = boxes != 0;
      } else {
        const float* kp = kpts + (long long)p * K * 3;
        int a, b;
        if (local < 4 + E) {
          a = edge[local - 4][0];
          b = edge[local - 4][1];
          r = rl;
          col = 1 + (local - 4);
        } else {
          a = b = local - 4 - E;
          r = rk;
          col = 1 + PAVE_DRAW_MAX_E + a;
          on = rk > 0;
        }
        const float* ka = kp + 3 * a;
        const float* kb = kp + 3 * b;
        on = on && ka[2] > plan.kpt_thr && kb[2] > plan.kpt_thr;
        ax = quant(ka[0], sx); ay = quant(ka[1], sy);
        bx = quant(kb[0], sx); by = quant(kb[1], sy);
      }
      if (on && min(ax, bx) - r <= tx1 && max(ax, bx) + r >= tx0 && min(ay, by) - r <= ty1 && max(ay, by) + r >= ty0) {
        Prim c;
        c.ax = (short)ax; c.ay = (short)ay; c.bx = (short)bx; c.by = (short)by;
        c.id = p * PP + local;
        c.r = (short)r;
        c.col = (short)col;
        cand[atomicAdd(&n_cand[cur], 1)] = c;
      }
    }
    __syncthreads();
    // -- every lane's four pixels against the round's list --
    const int nc = n_cand[cur];
    for (int i = 0; i < nc; ++i) {
      const Prim c = cand[i];
      const int dx = c.bx - c.ax, dy = c.by - c.ay;
      const long long L2 = (long long)dx * dx + (long long)dy * dy;
      const long long r2 = (long long)c.r * c.r, r2L2 = r2 * L2;
      const int X = 4 * px, Y = 4 * py;
      if (c.id > best00 && covers(X, Y, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best00 = c.id; col00 = c.col; }
      if (c.id > best01 && covers(X + 4, Y, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best01 = c.id; col01 = c.col; }
      if (c.id > best10 && covers(X, Y + 4, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best10 = c.id; col10 = c.col; }
      if (c.id > best11 && covers(X + 4, Y + 4, c.ax, c.ay, dx, dy, L2, r2, r2L2)) { best11 = c.id; col11 = c.col; }
    }
    __syncthreads();
  }

  // ---- the stores: covered bytes only ----
  unsigned char* __restrict__ dst = static_cast<unsigned char*>(plan.dst[s]);
  const long long pitch = plan.pitch[s];
  if (BGR) {
    if (px < W && py < H && best00 >= 0) {
      unsigned char* o = dst + py * pitch + 3 * px;
      o[0] = color[col00][0]; o[1] = color[col00][1]; o[2] = color[col00][2];
    }
    if (px + 1 < W && py < H && best01 >= 0) {
      unsigned char* o = dst + py * pitch + 3 * (px + 1);
      o[0] = color[col01][0]; o[1] = color[col01][1]; o[2] = color[col01][2];
    }
    if (px < W && py + 1 < H && best10 >= 0) {
      unsigned char* o = dst + (py + 1) * pitch + 3 * px;
      o[0] = color[col10][0]; o[1] = color[col10][1]; o[2] = color[col10][2];
    }
    if (px + 1 < W && py + 1 < H && best11 >= 0) {
      unsigned char* o = dst + (py + 1) * pitch + 3 * (px + 1);
      o[0] = color[col11][0]; o[1] = color[col11][1]; o[2] = color[col11][2];
    }
  } else if (px < W && py < H) {   // W and H are even: the 2 x 2 block is inside or outside as a whole
    unsigned char* y = dst + py * pitch + px;
    if (best00 >= 0) y[0] = color[col00][0];
    if (best01 >= 0) y[1] = color[col01][0];
    if (best10 >= 0) y[pitch] = color[col10][0];
    if (best11 >= 0) y[pitch + 1] = color[col11][0];
    int m = best00, mc = col00;
    if (best01 > m) { m = best01; mc = col01; }
    if (best10 > m) { m = best10; mc = col10; }
    if (best11 > m) { m = best11; mc = col11; }
    if (m >= 0) {
      unsigned char* uv = dst + ((long long)H + (py >> 1)) * pitch + px;
      uv[0] = color[mc][1];
      uv[1] = color[mc][2];
    }
  }
}

// Everything a plan could get wrong, before any device call.  bpp: bytes per pixel of a row (1 = NV12, 3 = BGR).
int draw_check(const pave_draw_plan* plan, const int bpp, int* max_w, int* max_h, int* poses) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "draw_poses: null plan");
  if (plan->n < 1 || plan->n > PAVE_DRAW_MAX_SURFACES)
    return pave_internal_fail(PAVE_E_ARG, "draw_poses: 1 .. 32 surfaces per launch");
  if (plan->K < 1 || plan->K > PAVE_DRAW_MAX_K) return pave_internal_fail(PAVE_E_ARG, "draw_poses: K outside 1 .. 32");
  if (plan->E < 0 || plan->E > PAVE_DRAW_MAX_E) return pave_internal_fail(PAVE_E_ARG, "draw_poses: E outside 0 .. 32");
  for (int e = 0; e < plan->E; ++e)
    if (plan->edge[e][0] >= plan->K || plan->edge[e][1] >= plan->K)
      return pave_internal_fail(PAVE_E_ARG, "draw_poses: an edge index >= K");
  if (plan->thickness < 1 || plan->thickness > 32)
    return pave_internal_fail(PAVE_E_ARG, "draw_poses: thickness outside 1 .. 32");
  if (plan->radius < 0 || plan->radius > 32) return pave_internal_fail(PAVE_E_ARG, "draw_poses: radius outside 0 .. 32");
  *max_w = *max_h = *poses = 0;
  for (int i = 0; i < plan->n; ++i) {
    const int w = plan->width[i], h = plan->height[i], N = plan->n_poses[i];
    if (!plan->dst[i]) return pave_internal_fail(PAVE_E_ARG, "draw_poses: null surface");
    if (w < 1 || h < 1 || w > PAVE_DRAW_MAX_SIZE || h > PAVE_DRAW_MAX_SIZE)
      return pave_internal_fail(PAVE_E_ARG, "draw_poses: width and height in 1 .. 8192");
    if (bpp == 1 && ((w | h) & 1)) return pave_internal_fail(PAVE_E_ARG, "draw_poses: NV12 width and height must be even");
    if (plan->pitch[i] < bpp * w) return pave_internal_fail(PAVE_E_ARG, "draw_poses: pitch below the bytes of a row");
    if (N < 0 || N > PAVE_DRAW_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "draw_poses: N outside 0 .. 4096");
    if (N > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "draw_poses: null pose tensor");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "draw_poses: scale must be positive and finite");
    if (plan->table[i] >= PAVE_DRAW_MAX_TABLES) return pave_internal_fail(PAVE_E_ARG, "draw_poses: colour table index >= 4");
    *max_w = w > *max_w ? w : *max_w;
    *max_h = h > *max_h ? h : *max_h;
    *poses += N;
  }
  return PAVE_OK;
}

template <int BGR>
int draw_launch(const pave_draw_plan* plan, void* stream) {
  int w = 0, h = 0, poses = 0;
  const int st = draw_check(plan, BGR ? 3 : 1, &w, &h, &poses);
  if (st != PAVE_OK) return st;
  if (poses == 0) return PAVE_OK;   // nothing to draw: no launch
  return pave_launch<draw_poses_kernel<BGR>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                   (unsigned)plan->n),
                                              dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // namespace

extern "C" {

int pave_draw_poses_nv12(const pave_draw_plan* plan, void* stream) { return draw_launch<0>(plan, stream); }

int pave_draw_poses_bgr(const pave_draw_plan* plan, void* stream) { return draw_launch<1>(plan, stream); }

}  // extern "C"
