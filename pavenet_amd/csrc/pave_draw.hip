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
//
// Track ids in the picture (IDS = 1: pave_draw_tracks_nv12 / _bgr, the same kernel source).  With ids[p] = v >= 1 the
// box edges and limbs of pose p take palette row (v - 1) % 32 (the discs keep their colours), and with label_scale
// g >= 1 the pose has two more primitives above every skeleton of the surface: a plate of g (6 n + 1) x 9 g pixels
// from (ax, ay) = (min(X1, X2) >> 2, max((min(Y1, Y2) >> 2) - 9 g, 0)), id N (4 + E + K) + 2 p, and on it the n decimal
// digits of v in the plan's 5 x 7 face, a font pixel g x g picture pixels, id + 1.  They are pixel rectangles: culled
// against the tile as such and tested per pixel by integer compares, no capsule arithmetic.  v <= 0 is section 13
// alone, or nothing under untracked_skip; a surface without ids is section 13 alone.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using pave_tracked::QMAX;
using pave_tracked::quant;

constexpr int TILE = 32;        // pixels per tile edge

struct Prim {                   // one candidate of the tile's list
  short ax, ay, bx, by;
  int id;
  short r;                      // quarter pixels
  short col;                    // row of the plan's colour table
};
// IDS = 1: a label is r = PLATE | INK, (ax, ay) the plate's corner in pixels, bx = n digits, by = g, v the id value
struct PrimIds : Prim { int v; };
constexpr int PLATE = -1, INK = -2;
constexpr int PALETTE0 = PAVE_DRAW_COLORS;                    // LDS colour rows 65 .. 96: the palette; 97: the ink
constexpr int COLORS_IDS = PAVE_DRAW_COLORS + PAVE_DRAW_PALETTE + 1;

template <int IDS> struct DrawTypes { using plan = pave_draw_plan; using prim = Prim; };
template <> struct DrawTypes<1> { using plan = pave_draw_ids_plan; using prim = PrimIds; };
__device__ __forceinline__ const pave_draw_plan& base_of(const pave_draw_plan& p) { return p; }
__device__ __forceinline__ const pave_draw_plan& base_of(const pave_draw_ids_plan& p) { return p.base; }

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

// The decimal digits of v >= 1: 1 .. 10.
__device__ __forceinline__ int digits_of(const int v) {
  return 1 + (v >= 10) + (v >= 100) + (v >= 1000) + (v >= 10000) + (v >= 100000) + (v >= 1000000) + (v >= 10000000) +
         (v >= 100000000) + (v >= 1000000000);
}

// The label rule for pixel (qx, qy): the plate's rectangle, or a set bit of the digit faces on it.
__device__ __forceinline__ bool label_covers(const int kind, const int qx, const int qy, const int ax, const int ay,
                                             const int g, const int n, const int v, const unsigned char* font) {
  if (kind == PLATE) return (unsigned)(qx - ax) < (unsigned)(g * (6 * n + 1)) && (unsigned)(qy - ay) < (unsigned)(9 * g);
  const int u = qx - ax - g, w = qy - ay - g;
  if ((unsigned)u >= (unsigned)(6 * g * n) || (unsigned)w >= (unsigned)(7 * g)) return false;
  const int cell = u / (6 * g), uu = u - cell * 6 * g;
  if (uu >= 5 * g) return false;
  unsigned q = (unsigned)v;                                   // digit `cell`, the most significant first
  for (int k = n - 1 - cell; k > 0; --k) q /= 10u;
  return (font[(q % 10u) * 7 + w / g] >> (4 - uu / g)) & 1;
}

// BGR = 0: NV12 (dst = H rows of Y, then H / 2 rows of interleaved U, V; pitch bytes per row).
// BGR = 1: [H, W, 3] bytes, pitch bytes per row.
// The surface is blockIdx.z: what a block reads from the by-value plan by surface is wave-uniform (scalar loads
// from the kernel arguments).  The two tables a lane indexes by itself (edges, colours) are read once per block,
// one entry per lane, into LDS: vector loads from the kernel-argument segment, no copy of the plan to scratch.
// IDS = 1 takes pave_draw_ids_plan: the palette joins the colour table in LDS and the font goes there the same way.
template <int BGR, int IDS>
__global__ __launch_bounds__(256) void draw_poses_kernel(const typename DrawTypes<IDS>::plan full) {
  using PrimT = typename DrawTypes<IDS>::prim;
  __shared__ unsigned short pose_list[PAVE_DRAW_MAX_POSES];
  __shared__ PrimT cand[256];
  __shared__ int n_pose, n_cand[2];
  __shared__ unsigned char edge[PAVE_DRAW_MAX_E][2];
  __shared__ unsigned char color[IDS ? COLORS_IDS : PAVE_DRAW_COLORS][4];
  __shared__ unsigned char font[IDS ? 70 : 1];

  const pave_draw_plan& plan = base_of(full);
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
  const int32_t* __restrict__ ids = nullptr;
  int g = 0, skip = 0;          // (constants of the IDS = 0 instantiations)
  if constexpr (IDS) { ids = full.ids[s]; g = full.label_scale; skip = full.untracked_skip; }
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
      int v = 0;
      if (IDS && drawn && ids != nullptr) {
        v = ids[p];
        drawn = !(skip && v <= 0);
      }
      const bool labelled = IDS && v >= 1 && g >= 1;
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
        if (boxes || labelled) {
          const int X1 = quant(b0, sx), Y1 = quant(b1, sy), X2 = quant(b2, sx), Y2 = quant(b3, sy);
          lox = min(lox, min(X1, X2)); hix = max(hix, max(X1, X2));
          loy = min(loy, min(Y1, Y2)); hiy = max(hiy, max(Y1, Y2));
          if (labelled) {   // the label's rectangle, as points: a tile only a label touches must not end below
            const int ax = min(X1, X2) >> 2, ay = max((min(Y1, Y2) >> 2) - 9 * g, 0);
            lox = min(lox, 4 * ax); hix = max(hix, 4 * (ax + g * (6 * digits_of(v) + 1) - 1));
            loy = min(loy, 4 * ay); hiy = max(hiy, 4 * (ay + 9 * g - 1));
          }
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
  if constexpr (IDS) {
    if (tid >= 160 && tid < 160 + PAVE_DRAW_PALETTE + 1) {
      const int i = tid - 160;
      color[PALETTE0 + i][0] = full.palette[tab][i][0];
      color[PALETTE0 + i][1] = full.palette[tab][i][1];
      color[PALETTE0 + i][2] = full.palette[tab][i][2];
    }
    if (tid < 70) font[tid] = full.font[tid / 7][tid % 7];
  }
  __syncthreads();

  // this lane's 2 x 2 pixels
  const int px = x0 + 2 * (tid & 15), py = y0 + 2 * (tid >> 4);
  int best00 = -1, best01 = -1, best10 = -1, best11 = -1;   // [row][column]
  int col00 = 0, col01 = 0, col10 = 0, col11 = 0;

  const int PW = IDS ? PP + 2 : PP;              // primitives walked per pose: IDS adds the plate and the ink
  const int total = np * PW;
  const int max_rounds = (N * PW + 255) / 256;   // from the plan alone
  const int xe = min(x0 + TILE, W), ye = min(y0 + TILE, H);
  for (int round = 0; round < max_rounds; ++round) {
    const int base = round * 256;
    if (base >= total) break;   // (block-uniform)
    const int cur = round & 1;
    if (tid == 0) n_cand[cur ^ 1] = 0;   // next round's counter: last read before this round's first barrier
    // -- build and cull one primitive --
    const int j = base + tid;
    if (j < total) {
      const int slot = j / PW, local = j - slot * PW;
      const int p = pose_list[slot];
      int ax, ay, bx, by, r, col;
      bool on = true;
      int v = 0;
      if (IDS && ids != nullptr) v = ids[p];
      const int pal = PALETTE0 + (int)(((unsigned)v - 1u) % PAVE_DRAW_PALETTE);   // read only where v >= 1
      if (IDS && local >= PP) {
        if constexpr (IDS) {
          const float* bb = bboxes + (long long)p * 5;
          const int X1 = quant(bb[0], sx), Y1 = quant(bb[1], sy), X2 = quant(bb[2], sx), Y2 = quant(bb[3], sy);
          const int kind = local == PP ? PLATE : INK, n = v >= 1 ? digits_of(v) : 1;
          const int lx = min(X1, X2) >> 2, ly = max((min(Y1, Y2) >> 2) - 9 * g, 0);
          // the rectangle that can be covered, in pixels: the plate, or the ink's field inside it
          const int rx0 = kind == PLATE ? lx : lx + g, rx1 = kind == PLATE ? lx + g * (6 * n + 1) : lx + g + 6 * g * n;
          const int ry0 = kind == PLATE ? ly : ly + g, ry1 = kind == PLATE ? ly + 9 * g : ly + 8 * g;
          if (v >= 1 && g >= 1 && rx0 < xe && rx1 > x0 && ry0 < ye && ry1 > y0) {
            PrimT c;
            c.ax = (short)lx; c.ay = (short)ly; c.bx = (short)n; c.by = (short)g;
            c.id = N * PP + 2 * p + (kind == INK);
            c.r = (short)kind;
            c.col = (short)(kind == PLATE ? pal : PALETTE0 + PAVE_DRAW_PALETTE);
            c.v = v;
            cand[atomicAdd(&n_cand[cur], 1)] = c;
          }
        }
        on = false;
        ax = ay = bx = by = r = col = 0;
      } else if (local < 4) {
        const float* bb = bboxes + (long long)p * 5;
        const int X1 = quant(bb[0], sx), Y1 = quant(bb[1], sy), X2 = quant(bb[2], sx), Y2 = quant(bb[3], sy);
        // top, right, bottom, left
        ax = (local == 0 || local == 3) ? X1 : X2;
        ay = (local < 2) ? Y1 : Y2;
        bx = (local < 2) ? X2 : X1;
        by = (local == 0 || local == 3) ? Y1 : Y2;
        r = rl;
        col = (IDS && v >= 1) ? pal : 0;
        on = boxes != 0;
      } else {
        const float* kp = kpts + (long long)p * K * 3;
        int a, b;
        if (local < 4 + E) {
          a = edge[local - 4][0];
          b = edge[local - 4][1];
          r = rl;
          col = (IDS && v >= 1) ? pal : 1 + (local - 4);
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
        PrimT c;
        c.ax = (short)ax; c.ay = (short)ay; c.bx = (short)bx; c.by = (short)by;
        c.id = p * PP + local;
        c.r = (short)r;
        c.col = (short)col;
        if constexpr (IDS) c.v = v;
        cand[atomicAdd(&n_cand[cur], 1)] = c;
      }
    }
    __syncthreads();
    // -- every lane's four pixels against the round's list --
    const int nc = n_cand[cur];
    for (int i = 0; i < nc; ++i) {
      const PrimT c = cand[i];
      if constexpr (IDS) {
        if (c.r < 0) {   // a label (the same entry in every lane: no divergence on this branch)
          if (c.id > best00 && label_covers(c.r, px, py, c.ax, c.ay, c.by, c.bx, c.v, font)) { best00 = c.id; col00 = c.col; }
          if (c.id > best01 && label_covers(c.r, px + 1, py, c.ax, c.ay, c.by, c.bx, c.v, font)) { best01 = c.id; col01 = c.col; }
          if (c.id > best10 && label_covers(c.r, px, py + 1, c.ax, c.ay, c.by, c.bx, c.v, font)) { best10 = c.id; col10 = c.col; }
          if (c.id > best11 && label_covers(c.r, px + 1, py + 1, c.ax, c.ay, c.by, c.bx, c.v, font)) { best11 = c.id; col11 = c.col; }
          continue;
        }
      }
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

// What the ids plan adds to draw_check, also before any device call.
int draw_ids_check(const pave_draw_ids_plan* plan, const int bpp, int* max_w, int* max_h, int* poses) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "draw_tracks: null plan");
  const int st = draw_check(&plan->base, bpp, max_w, max_h, poses);
  if (st != PAVE_OK) return st;
  if (plan->label_scale < 0 || plan->label_scale > 8)
    return pave_internal_fail(PAVE_E_ARG, "draw_tracks: label_scale outside 0 .. 8");
  if (plan->untracked_skip != 0 && plan->untracked_skip != 1)
    return pave_internal_fail(PAVE_E_ARG, "draw_tracks: untracked_skip is 0 or 1");
  for (int d = 0; d < 10; ++d)
    for (int row = 0; row < 7; ++row)
      if (plan->font[d][row] & ~0x1f) return pave_internal_fail(PAVE_E_ARG, "draw_tracks: a font row has bits above the low 5");
  return PAVE_OK;
}

template <int BGR>
int draw_launch(const pave_draw_plan* plan, void* stream) {
  int w = 0, h = 0, poses = 0;
  const int st = draw_check(plan, BGR ? 3 : 1, &w, &h, &poses);
  if (st != PAVE_OK) return st;
  if (poses == 0) return PAVE_OK;   // nothing to draw: no launch
  return pave_launch<draw_poses_kernel<BGR, 0>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                      (unsigned)plan->n),
                                                 dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

template <int BGR>
int draw_tracks_launch(const pave_draw_ids_plan* plan, void* stream) {
  int w = 0, h = 0, poses = 0;
  const int st = draw_ids_check(plan, BGR ? 3 : 1, &w, &h, &poses);
  if (st != PAVE_OK) return st;
  if (poses == 0) return PAVE_OK;   // nothing to draw: no launch
  return pave_launch<draw_poses_kernel<BGR, 1>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                      (unsigned)plan->base.n),
                                                 dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // namespace

extern "C" {

int pave_draw_poses_nv12(const pave_draw_plan* plan, void* stream) { return draw_launch<0>(plan, stream); }

int pave_draw_poses_bgr(const pave_draw_plan* plan, void* stream) { return draw_launch<1>(plan, stream); }

int pave_draw_tracks_nv12(const pave_draw_ids_plan* plan, void* stream) { return draw_tracks_launch<0>(plan, stream); }

int pave_draw_tracks_bgr(const pave_draw_ids_plan* plan, void* stream) { return draw_tracks_launch<1>(plan, stream); }

}  // extern "C"
