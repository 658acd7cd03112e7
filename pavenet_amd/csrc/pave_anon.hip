// People hidden in frames on the device: the heads or the whole persons of the poses pixelated or filled, in place, in
// one launch for up to 32 separately allocated surfaces (pave_anonymize_nv12: pitched NV12; pave_anonymize_bgr:
// [H, W, 3] BGR).
//
// The rule is DESIGN section 15 and is integer-exact.  Which poses count, which key points are visible and the quarter
// pixel X = clamp((int)rintf((x / sx) * 4.f), 0, 32767) of a coordinate are section 13's.  A pose has a region: a
// rectangle A in quarter pixels and a radius r, the points within r of A.  With (x1, y1, x2, y2) the sorted quantised
// box and s its larger side:
//   person: A = the box,  r = 4 margin + ((s grow) >> 4);
//   head:   A = the bounding rectangle of the visible head key points, e its larger side,
//           r = 4 margin + max((e head_scale) >> 4, (s head_min) >> 4);  none visible: the person region, or none.
// The picture is cut into cell x cell pixel cells from its origin (clipped right and bottom); a cell of pixels
// x0 .. x1 - 1, y0 .. y1 - 1 is the rectangle C = [4 x0, 4 (x1 - 1)] x [4 y0, 4 (y1 - 1)] and is masked iff for some
// region gx^2 + gy^2 <= r^2 in int64, gx = max(0, A.x1 - C.x2, C.x1 - A.x2), gy the same in y.  Every sample of a
// plane in a masked cell becomes (2 sum + n) / (2 n) of the cell's n original samples of that plane (pixelate), or
// the plan's fill bytes (fill).  The kernel does no colour arithmetic.
//
// 256 threads own a 64 x 64 pixel tile: whole cells for every cell size, so a cell has one block that reads it and
// then writes it, which is what makes the call safe in place.  The block walks the poses 256 at a time, one lane per
// pose: a lane builds its pose's region, tests it against the tile's rectangle by the rule itself (a cell's gaps are
// never smaller than its tile's) and appends a survivor to a 256-entry LDS list -- a round appends at most 256, so
// the list cannot overflow whatever N is -- and after a barrier every lane tests its cells (up to 4 at cell = 2)
// against the list and sets their flags; the flags are a union, so no order matters.  A tile without a flagged cell
// ends there without a write.  Then the planes are walked in 4-byte groups, 256 per step along the rows: a group in a
// flagged cell is read and added, per channel, to the cell's integer sums in LDS (a lane keeps the sums of
// consecutive groups of one cell in registers and adds them with one LDS atomic per channel: integer sums, any order
// gives the same bits), a barrier, one lane per cell makes the bytes to store, a barrier, and the same walk stores
// them.  A group is one 32-bit access only where the surface's base and pitch are multiples of 4, the cell is at least
// 4 pixels (then its byte width is a multiple of 4 and a group never crosses a cell border) and the group ends inside
// the row; everywhere else it is single bytes, so no store ever covers a byte outside a masked cell.  Every loop
// bound comes from the plan, every barrier is block-uniform, there are no global atomics and no scratch.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using pave_tracked::QMAX;
using pave_tracked::quant;

constexpr int TILE = PAVE_ANON_MAX_CELL;          // pixels per tile edge
constexpr int MAX_CELLS = (TILE / 2) * (TILE / 2);   // cells of a tile at cell = 2

struct Region { int x1, y1, x2, y2, r; };         // quarter pixels

__device__ __forceinline__ bool finite4(const float a, const float b, const float c, const float d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

// Is the rectangle [cx1, cx2] x [cy1, cy2] within r of the region's rectangle?
__device__ __forceinline__ bool touches(const Region& g, const int cx1, const int cy1, const int cx2, const int cy2) {
  const long long gx = max(0, max(g.x1 - cx2, cx1 - g.x2)), gy = max(0, max(g.y1 - cy2, cy1 - g.y2));
  return gx * gx + gy * gy <= (long long)g.r * g.r;
}

// The sums of one lane: those of the cell it is in, handed to LDS when the cell changes.
struct Sums {
  int cell = -1, a0 = 0, a1 = 0, a2 = 0;
  __device__ __forceinline__ void flush(int* sum) {
    if (cell >= 0) {
      if (a0) atomicAdd(&sum[3 * cell], a0);
      if (a1) atomicAdd(&sum[3 * cell + 1], a1);
      if (a2) atomicAdd(&sum[3 * cell + 2], a2);
    }
    a0 = a1 = a2 = 0;
  }
  __device__ __forceinline__ void add(int* sum, const int c, const int ch, const int v) {
    if (c != cell) { flush(sum); cell = c; }
    a0 += ch == 0 ? v : 0;
    a1 += ch == 1 ? v : 0;
    a2 += ch == 2 ? v : 0;
  }
};

// One plane of the tile: rows r0 .. of `trows`, bytes xb0 .. of 4 QPR per row, C interleaved channels whose sums and
// bytes are at channel CH0 + (byte % C) of a cell; a cell is 2^lg pixels wide, a pixel C bytes, and 2^lg_rows rows
// high.  WRITE = 0 adds the flagged cells' bytes to `sum`, WRITE = 1 stores `val` into them.
template <int C, int CH0, int QPR, int WRITE>
__device__ __forceinline__ void walk(unsigned char* __restrict__ plane, const long long pitch, const int row_bytes,
                                     const int rows, const int xb0, const int r0, const int trows, const int lg,
                                     const int lg_rows, const int cpt, const bool wide,
                                     const unsigned char* flag, int* sum, const unsigned char* val, const int tid) {
  Sums acc;
  for (int q = tid; q < QPR * trows; q += 256) {
    const int rl = q / QPR, xl = 4 * (q - rl * QPR);
    const int row = r0 + rl, xb = xb0 + xl;
    if (row >= rows || xb >= row_bytes) continue;
    unsigned char* p = plane + row * pitch + xb;
    const int crow = (rl >> lg_rows) * cpt;
    if (wide && xb + 4 <= row_bytes) {   // inside one cell: the cell's byte width is a multiple of 4, as xl is
      const int c = crow + ((C == 3 ? xl / 3 : xl / C) >> lg);
      if (!flag[c]) continue;
      const int ch = C == 3 ? xb % 3 : 0;   // the channel of byte 0 (xb is a multiple of 4: 0 for C = 1, 2)
      const int ch1 = (ch + 1) % C, ch2 = (ch + 2) % C, ch3 = (ch + 3) % C;
      if (WRITE) {
        const unsigned char* v = val + 4 * c + CH0;
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[ch] | ((uint32_t)v[ch1] << 8) | ((uint32_t)v[ch2] << 16) |
                                          ((uint32_t)v[ch3] << 24);
      } else {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        acc.add(sum, c, CH0 + ch, (int)(w & 255u));
        acc.add(sum, c, CH0 + ch1, (int)((w >> 8) & 255u));
        acc.add(sum, c, CH0 + ch2, (int)((w >> 16) & 255u));
        acc.add(sum, c, CH0 + ch3, (int)(w >> 24));
      }
    } else {
      for (int j = 0; j < 4 && xb + j < row_bytes; ++j) {
        const int c = crow + (((xl + j) / C) >> lg);
        if (!flag[c]) continue;
        const int ch = CH0 + (xb + j) % C;
        if (WRITE) p[j] = val[4 * c + ch];
        else acc.add(sum, c, ch, p[j]);
      }
    }
  }
  if (!WRITE) acc.flush(sum);
}

// BGR = 0: NV12 (dst = H rows of Y, then H / 2 rows of interleaved U, V; pitch bytes per row).
// BGR = 1: [H, W, 3] bytes, pitch bytes per row.
// The surface is blockIdx.z: what a block reads from the by-value plan is wave-uniform (scalar loads from the kernel
// arguments), the head indices and the fill bytes included.
template <int BGR>
__global__ __launch_bounds__(256) void anonymize_kernel(const pave_anon_plan plan) {
  __shared__ Region reg[256];
  __shared__ int n_reg[2], any_flag;
  __shared__ unsigned char flag[MAX_CELLS];
  __shared__ int sum[3 * MAX_CELLS];
  __shared__ unsigned char val[4 * MAX_CELLS];

  const int s = blockIdx.z;
  const int W = plan.width[s], H = plan.height[s], N = plan.n_poses[s];
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  if (x0 >= W || y0 >= H || N <= 0) return;   // (block-uniform: before any barrier)
  const int tid = threadIdx.x;
  const int K = plan.K, cell = plan.cell, lg = 31 - __clz(cell), cpt = TILE >> lg, cells = cpt * cpt;
  const float sx = plan.scale[s][0], sy = plan.scale[s][1];
  const float* __restrict__ kpts = plan.kpts[s];
  const float* __restrict__ bboxes = plan.bboxes[s];
  const int32_t* __restrict__ keep = plan.keep[s];
  const int xe = min(x0 + TILE, W), ye = min(y0 + TILE, H);
  const int ncx = (xe - x0 + cell - 1) >> lg, ncy = (ye - y0 + cell - 1) >> lg;   // the cells the picture has here

  for (int c = tid; c < cells; c += 256) flag[c] = 0;
  if (tid == 0) { n_reg[0] = 0; n_reg[1] = 0; any_flag = 0; }
  __syncthreads();

  // ---- regions on the tile, one lane per pose, and the cells they mask ----
  for (int base = 0, round = 0; base < N; base += 256, ++round) {
    const int cur = round & 1;
    if (tid == 0) n_reg[cur ^ 1] = 0;   // next round's counter: last read before the barrier that ended the last round
    const int p = base + tid;
    if (p < N) {
      const float* bb = bboxes + (long long)p * 5;
      const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
      bool counts = (keep == nullptr || keep[p] != 0) && bb[4] > plan.score_thr && finite4(b0, b1, b2, b3);
      if (counts) {
        const float* kp = kpts + (long long)p * K * 3;
        for (int k = 0; k < K; ++k) counts = counts && isfinite(kp[3 * k]) && isfinite(kp[3 * k + 1]);
        const int X1 = quant(b0, sx), Y1 = quant(b1, sy), X2 = quant(b2, sx), Y2 = quant(b3, sy);
        Region g;
        g.x1 = min(X1, X2); g.x2 = max(X1, X2);
        g.y1 = min(Y1, Y2); g.y2 = max(Y1, Y2);
        const int side = max(g.x2 - g.x1, g.y2 - g.y1);
        g.r = 4 * plan.margin + ((side * plan.grow) >> 4);
        if (plan.region == 0) {
          int lox = QMAX, loy = QMAX, hix = 0, hiy = 0, seen = 0;
          for (int h = 0; h < plan.n_head; ++h) {
            const float* kh = kp + 3 * plan.head[h];
            if (kh[2] > plan.kpt_thr) {
              const int X = quant(kh[0], sx), Y = quant(kh[1], sy);
              lox = min(lox, X); hix = max(hix, X);
              loy = min(loy, Y); hiy = max(hiy, Y);
              ++seen;
            }
          }
          if (seen) {
            g.x1 = lox; g.x2 = hix; g.y1 = loy; g.y2 = hiy;
            g.r = 4 * plan.margin + max((max(hix - lox, hiy - loy) * plan.head_scale) >> 4, (side * plan.head_min) >> 4);
          } else if (plan.fallback_skip) {
            counts = false;
          }
        }
        if (counts && touches(g, 4 * x0, 4 * y0, 4 * (xe - 1), 4 * (ye - 1))) reg[atomicAdd(&n_reg[cur], 1)] = g;
      }
    }
    __syncthreads();
    const int nr = n_reg[cur];
    for (int c = tid; c < cells; c += 256) {
      const int cyl = c >> (6 - lg), cxl = c & (cpt - 1);
      if (cxl >= ncx || cyl >= ncy || flag[c]) continue;
      const int cx0 = x0 + (cxl << lg), cy0 = y0 + (cyl << lg);
      const int cx1 = min(cx0 + cell, W), cy1 = min(cy0 + cell, H);
      for (int i = 0; i < nr; ++i)
        if (touches(reg[i], 4 * cx0, 4 * cy0, 4 * (cx1 - 1), 4 * (cy1 - 1))) {
          flag[c] = 1;
          any_flag = 1;
          break;
        }
    }
    __syncthreads();
  }
  if (!any_flag) return;   // (block-uniform)

  unsigned char* __restrict__ dst = static_cast<unsigned char*>(plan.dst[s]);
  const long long pitch = plan.pitch[s];
  const bool wide = cell >= 4 && ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)pitch) & 3) == 0;
  const int fill = plan.mode;

  // ---- the flagged cells' sums ----
  if (!fill) {
    for (int i = tid; i < 3 * cells; i += 256) sum[i] = 0;
    __syncthreads();
    if (BGR) {
      walk<3, 0, 3 * TILE / 4, 0>(dst, pitch, 3 * W, H, 3 * x0, y0, TILE, lg, lg, cpt, wide, flag, sum, val, tid);
    } else {
      walk<1, 0, TILE / 4, 0>(dst, pitch, W, H, x0, y0, TILE, lg, lg, cpt, wide, flag, sum, val, tid);
      walk<2, 1, TILE / 4, 0>(dst + H * pitch, pitch, W, H / 2, x0, y0 / 2, TILE / 2, lg - 1, lg - 1, cpt, wide, flag,
                              sum, val, tid);
    }
    __syncthreads();
  }

  // ---- the bytes to store, one lane per cell ----
  const int tab = plan.table[s];
  for (int c = tid; c < cells; c += 256) {
    if (!flag[c]) continue;
    if (fill) {
      val[4 * c] = plan.fill[tab][0];
      val[4 * c + 1] = plan.fill[tab][1];
      val[4 * c + 2] = plan.fill[tab][2];
    } else {
      const int cx0 = x0 + ((c & (cpt - 1)) << lg), cy0 = y0 + ((c >> (6 - lg)) << lg);
      const int w = min(cx0 + cell, W) - cx0, h = min(cy0 + cell, H) - cy0;
      const int n0 = w * h, n12 = BGR ? n0 : (w >> 1) * (h >> 1);   // (NV12 sizes and cells are even)
      val[4 * c] = (unsigned char)((2 * sum[3 * c] + n0) / (2 * n0));
      val[4 * c + 1] = (unsigned char)((2 * sum[3 * c + 1] + n12) / (2 * n12));
      val[4 * c + 2] = (unsigned char)((2 * sum[3 * c + 2] + n12) / (2 * n12));
    }
  }
  __syncthreads();

  // ---- the stores: bytes of flagged cells only ----
  if (BGR) {
    walk<3, 0, 3 * TILE / 4, 1>(dst, pitch, 3 * W, H, 3 * x0, y0, TILE, lg, lg, cpt, wide, flag, sum, val, tid);
  } else {
    walk<1, 0, TILE / 4, 1>(dst, pitch, W, H, x0, y0, TILE, lg, lg, cpt, wide, flag, sum, val, tid);
    walk<2, 1, TILE / 4, 1>(dst + H * pitch, pitch, W, H / 2, x0, y0 / 2, TILE / 2, lg - 1, lg - 1, cpt, wide, flag, sum,
                            val, tid);
  }
}

// Everything a plan could get wrong, before any device call.  bpp: bytes per pixel of a row (1 = NV12, 3 = BGR).
int anon_check(const pave_anon_plan* plan, const int bpp, int* max_w, int* max_h, int* poses) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "anonymize: null plan");
  if (plan->n < 1 || plan->n > PAVE_DRAW_MAX_SURFACES)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: 1 .. 32 surfaces per launch");
  if (plan->K < 1 || plan->K > PAVE_DRAW_MAX_K) return pave_internal_fail(PAVE_E_ARG, "anonymize: K outside 1 .. 32");
  if (plan->region != 0 && plan->region != 1) return pave_internal_fail(PAVE_E_ARG, "anonymize: region is 0 or 1");
  if (plan->mode != 0 && plan->mode != 1) return pave_internal_fail(PAVE_E_ARG, "anonymize: mode is 0 or 1");
  if (plan->fallback_skip != 0 && plan->fallback_skip != 1)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: fallback_skip is 0 or 1");
  if (plan->n_head < 0 || plan->n_head > PAVE_ANON_MAX_HEAD)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: n_head outside 0 .. 8");
  if (plan->region == 0 && plan->n_head == 0)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: the head region needs head indices");
  for (int h = 0; h < plan->n_head; ++h)
    if (plan->head[h] >= plan->K) return pave_internal_fail(PAVE_E_ARG, "anonymize: a head index >= K");
  const int cell = plan->cell;
  if (cell < 2 || cell > PAVE_ANON_MAX_CELL || (cell & (cell - 1)))
    return pave_internal_fail(PAVE_E_ARG, "anonymize: cell is 2, 4, 8, 16, 32 or 64");
  if (plan->margin < 0 || plan->margin > PAVE_ANON_MAX_MARGIN)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: margin outside 0 .. 64");
  if (plan->grow < 0 || plan->grow > PAVE_ANON_MAX_SIXTEENTHS)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: grow outside 0 .. 32");
  if (plan->head_scale < 0 || plan->head_scale > PAVE_ANON_MAX_SIXTEENTHS)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: head_scale outside 0 .. 32");
  if (plan->head_min < 0 || plan->head_min > PAVE_ANON_MAX_SIXTEENTHS)
    return pave_internal_fail(PAVE_E_ARG, "anonymize: head_min outside 0 .. 32");
  *max_w = *max_h = *poses = 0;
  for (int i = 0; i < plan->n; ++i) {
    const int w = plan->width[i], h = plan->height[i], N = plan->n_poses[i];
    if (!plan->dst[i]) return pave_internal_fail(PAVE_E_ARG, "anonymize: null surface");
    if (w < 1 || h < 1 || w > PAVE_DRAW_MAX_SIZE || h > PAVE_DRAW_MAX_SIZE)
      return pave_internal_fail(PAVE_E_ARG, "anonymize: width and height in 1 .. 8192");
    if (bpp == 1 && ((w | h) & 1)) return pave_internal_fail(PAVE_E_ARG, "anonymize: NV12 width and height must be even");
    if (plan->pitch[i] < bpp * w) return pave_internal_fail(PAVE_E_ARG, "anonymize: pitch below the bytes of a row");
    if (N < 0 || N > PAVE_DRAW_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "anonymize: N outside 0 .. 4096");
    if (N > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "anonymize: null pose tensor");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "anonymize: scale must be positive and finite");
    if (plan->table[i] >= PAVE_DRAW_MAX_TABLES) return pave_internal_fail(PAVE_E_ARG, "anonymize: fill table index >= 4");
    *max_w = w > *max_w ? w : *max_w;
    *max_h = h > *max_h ? h : *max_h;
    *poses += N;
  }
  return PAVE_OK;
}

template <int BGR>
int anon_launch(const pave_anon_plan* plan, void* stream) {
  int w = 0, h = 0, poses = 0;
  const int st = anon_check(plan, BGR ? 3 : 1, &w, &h, &poses);
  if (st != PAVE_OK) return st;
  if (poses == 0) return PAVE_OK;   // nobody to hide: no launch
  return pave_launch<anonymize_kernel<BGR>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                 (unsigned)plan->n),
                                            dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // namespace

extern "C" {

int pave_anonymize_nv12(const pave_anon_plan* plan, void* stream) { return anon_launch<0>(plan, stream); }

int pave_anonymize_bgr(const pave_anon_plan* plan, void* stream) { return anon_launch<1>(plan, stream); }

}  // extern "C"
