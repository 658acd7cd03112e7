// Footfall heat maps for the live path: where tracked people stood (dwell) and which cells they entered (visits),
// accumulated per camera on a grid of cells on the device, in one launch for up to 32 frames of any number of cameras
// (pave_heat_update), and the map as a colour overlay composited into decoder-style surfaces (pave_draw_heat_nv12:
// pitched NV12; pave_draw_heat_bgr: [H, W, 3] BGR).
//
// Both rules are DESIGN section 21 and are integer-exact.
//   update: section 17's poses, slots and 1/8-pixel anchor (pave_tracked.h).  Per frame: the clock advances and slots not
//     seen for more than max_age frames are freed; every half_life frames both maps and peak are halved (v >> 1);
//     poses find or take slots; a pose that takes part with its anchor a on the map (0 <= a < 8 size) stands in cell
//     (a.x >> (3 + log2 cell), a.y >> (3 + log2 cell)) and adds (r + 1 - |dx|)(r + 1 - |dy|) to dwell at the cells
//     within r of it that the grid has, and 1 to visits at its own cell iff its slot was born in this frame or stood in
//     another cell (or off the map, cell -1) before; peak[m] is the maximum of map m; the outputs are the pose's cell
//     and the two maps at it after the whole frame.
//   draw: level(cell) = min(255, 255 max(v, 0) / scale) in int64, scale = full_scale or max(peak, 1); a pixel takes the
//     level of its own cell, or (smooth) the bilinear mean of the four cells about it in half pixels, edge cells
//     replicated: u = 2 p + 1 (a chroma sample: 2 b + 2), t = u - cell, i0 = floor(t / (2 cell)), f = t - 2 cell i0,
//     weights 2 cell - f and f, level = (sum wx wy L + 2 cell^2) >> (2 + 2 log2 cell).  a = level < floor ? 0 :
//     (alpha_max level + 128) >> 8 and out = (src (256 - a) + palette[level] a + 128) >> 8 per byte.
//
// Update: one block of 256 threads per camera of the launch (pave_tracked.h), which takes that camera's entries in
// plan order, so the forget pass of a frame runs between the splats of the frame before and of its own frame, with a
// block barrier on either side; launches on one stream follow each other.  The splat is global integer atomics, which
// commute: 128 poses on one cell come out exact.  An atomic add returns the word before it, so the largest (returned +
// added) over a frame's adds is the largest word the frame touched, and peak is maintained through an LDS atomic max
// without a pass over the map.  The maps are read and written with device-scope atomic loads and stores wherever a
// plain access could meet a line the block's own vector cache still holds from before the atomics (the forget pass,
// the outputs).  slot_cell is only ever compared, never used as an index; every cell index is formed from an anchor
// that has passed the on-the-map test and is clipped to the grid per neighbour.
//
// Draw: pave_draw.hip's tile scheme: 256 threads own a 32 x 32 pixel tile, a thread one 2 x 2 block of it (and, NV12,
// its chroma sample), so every output byte has one writer.  The tile's cells (plus one ring for smooth; at most 10 x 10
// at cell 4) are staged in LDS as levels, their indices clamped to the grid; a tile whose largest level gives alpha 0
// returns before it touches the surface or the palette.  Every loop bound is from the plan or the header's maxima, every
// barrier is block-uniform, and there is no scratch area.
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
constexpr int TILE = 32;                             // pixels per tile edge of the draw kernels
constexpr int MAXC = TILE / 4 + 2;                   // cells a tile spans per axis at cell 4, with the ring
static_assert(MAXP <= NT && MAXS <= NT && MAXC * MAXC <= NT, "thread roles");

__device__ __forceinline__ int map_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void map_store(int32_t* p, const int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int log2_cell(const int cell) { return 31 - __clz(cell); }

__global__ __launch_bounds__(NT) void heat_update_kernel(const pave_heat_plan plan) {
  __shared__ int slot_id[MAXS];      // 0: free
  __shared__ int det_id[MAXP];
  __shared__ int det_bad[MAXP];      // != 0: a coordinate that is not finite
  __shared__ int det_ok[MAXP];       // != 0: keep and a box score above the threshold
  __shared__ int det_slot[MAXP];     // the slot of a pose that takes part, or -1
  __shared__ int det_born[MAXP];     // != 0: the slot was born in this frame
  __shared__ int cam_state[2];       // frame, dropped
  __shared__ int peak[2];

  const int b = blockIdx.x;
  const int cam = plan.camera[b];
  if (!owns_camera(plan, b, cam)) return;   // (block-uniform, before any barrier: an earlier block has this camera)
  const int tid = threadIdx.x;
  const int S = plan.S, K = plan.K;
  const int lc = log2_cell(plan.cell), r = plan.radius;
  const int Gw = (plan.width + plan.cell - 1) >> lc, Gh = (plan.height + plan.cell - 1) >> lc;
  const int cells = Gw * Gh;
  int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  int32_t* __restrict__ g_last = plan.slot_last + (long long)cam * S;
  int32_t* __restrict__ g_cell = plan.slot_cell + (long long)cam * S;
  int32_t* g_dwell = plan.dwell + (long long)cam * cells;
  int32_t* g_visits = plan.visits + (long long)cam * cells;

  if (tid == 0) {
    cam_state[0] = plan.frame[cam];
    cam_state[1] = plan.dropped[cam];
  }
  if (tid < 2) peak[tid] = plan.peak[2 * cam + tid];

  for (int e = b; e < plan.entries; ++e) {
    if (plan.camera[e] != cam) continue;   // (block-uniform)
    __syncthreads();                       // the frame before is stored; cam_state and peak are written
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

    // ---- 2: forget (the splats of the frame before are behind the barrier at the loop's head) ----
    if (plan.half_life > 0 && frame % plan.half_life == 0) {   // (block-uniform)
      for (int i = tid; i < cells; i += NT) {
        map_store(g_dwell + i, map_load(g_dwell + i) >> 1);
        map_store(g_visits + i, map_load(g_visits + i) >> 1);
      }
      if (tid < 2) peak[tid] >>= 1;
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

    // ---- 4, 5: pose tid in its slot: anchor, cell, splat ----
    int my_cell = -1;
    if (tid < n) {
      const int t = det_slot[tid];   // (in 0 .. S - 1 or -1: a slot index is a loop counter of step 3)
      if (t >= 0) {
        long long ax, ay;
        anchor(plan, kpts, tid, K, sx, sy, X1, Y1, X2, Y2, ax, ay);
        if (ax >= 0 && ay >= 0 && ax < 8ll * plan.width && ay < 8ll * plan.height) {
          const int gx = (int)(ax >> (3 + lc)), gy = (int)(ay >> (3 + lc));   // < Gw, < Gh by the test above
          my_cell = gy * Gw + gx;
          int top = 0;
          for (int dy = -r; dy <= r; ++dy) {
            const int y = gy + dy;
            if (y < 0 || y >= Gh) continue;
            for (int dx = -r; dx <= r; ++dx) {
              const int x = gx + dx;
              if (x < 0 || x >= Gw) continue;
              const int w = (r + 1 - abs(dx)) * (r + 1 - abs(dy));
              top = max(top, (int)((unsigned)atomicAdd(g_dwell + y * Gw + x, w) + (unsigned)w));
            }
          }
          atomicMax(&peak[PAVE_HEAT_DWELL], top);
          if (det_born[tid] != 0 || g_cell[t] != my_cell)
            atomicMax(&peak[PAVE_HEAT_VISITS], (int)((unsigned)atomicAdd(g_visits + my_cell, 1) + 1u));
        }
        g_cell[t] = my_cell;
        g_last[t] = frame;
      }
    }
    __syncthreads();   // every add of the frame is done

    // ---- 6: the outputs; peak ----
    if (tid < n) {
      plan.out_cell[e][tid] = my_cell;
      plan.out_dwell[e][tid] = my_cell >= 0 ? map_load(g_dwell + my_cell) : 0;
      plan.out_visits[e][tid] = my_cell >= 0 ? map_load(g_visits + my_cell) : 0;
    }
    if (tid < 2) plan.peak[2 * cam + tid] = peak[tid];
  }
}

// ---- the overlay ----

__device__ __forceinline__ int blend(const int src, const int col, const int a) {
  return (src * (256 - a) + col * a + 128) >> 8;
}

// One axis of the smooth rule at half-pixel coordinate u: the staged index of cell i0 (the tile's first staged cell is
// `lo`) and the weight f of the cell after it, of 2 cell.
__device__ __forceinline__ void axis(const int u, const int cell, const int lc, const int lo, int& j, int& f) {
  const int t = u - cell;
  const int i0 = t >> (1 + lc);   // (arithmetic: floor)
  f = t - (i0 << (1 + lc));
  j = i0 - lo;
}

// BGR = 0: NV12 (dst = H rows of Y, then H / 2 rows of interleaved U, V; pitch bytes per row).
// BGR = 1: [H, W, 3] bytes, pitch bytes per row.  The surface is blockIdx.z.
template <int BGR>
__global__ __launch_bounds__(256) void draw_heat_kernel(const pave_heat_draw_plan plan) {
  __shared__ int level[MAXC * MAXC];
  __shared__ int top_level;
  __shared__ unsigned char pal[256][3];

  const int s = blockIdx.z;
  const int W = min(plan.width[s], plan.map_width), H = min(plan.height[s], plan.map_height);   // what may be written
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  if (x0 >= W || y0 >= H) return;   // (block-uniform: before any barrier)
  const int tid = threadIdx.x;
  const int cam = plan.camera[s], cell = plan.cell, lc = log2_cell(cell), smooth = plan.smooth;
  const int Gw = (plan.map_width + cell - 1) >> lc, Gh = (plan.map_height + cell - 1) >> lc;
  const int32_t* __restrict__ g_map = plan.map + (long long)cam * Gw * Gh;
  const int xe = min(x0 + TILE, W), ye = min(y0 + TILE, H);
  // the cells the tile's pixels read, unclamped: lo .. lo + n - 1 per axis
  const int lox = smooth ? (2 * x0 + 1 - cell) >> (1 + lc) : x0 >> lc;
  const int loy = smooth ? (2 * y0 + 1 - cell) >> (1 + lc) : y0 >> lc;
  // (the largest u of the tile is 2 xe: the chroma sample of a block whose second column is clipped away)
  const int hix = smooth ? ((2 * xe - cell) >> (1 + lc)) + 1 : (xe - 1) >> lc;
  const int hiy = smooth ? ((2 * ye - cell) >> (1 + lc)) + 1 : (ye - 1) >> lc;
  const int ncx = min(hix - lox + 1, MAXC), ncy = min(hiy - loy + 1, MAXC);   // (<= MAXC by construction)

  if (tid == 0) top_level = 0;
  __syncthreads();
  if (tid < ncx * ncy) {
    const int gx = min(max(lox + tid % ncx, 0), Gw - 1), gy = min(max(loy + tid / ncx, 0), Gh - 1);
    long long scale = plan.full_scale;
    if (scale <= 0) scale = max(plan.peak[2 * cam + plan.source], 1);
    const long long v = max(g_map[gy * Gw + gx], 0);
    const int L = (int)min(255ll, 255ll * v / scale);
    level[tid] = L;
    if (L > 0) atomicMax(&top_level, L);
  }
  __syncthreads();
  const int top = top_level, a_max = plan.alpha_max, floor_ = plan.floor;
  if (top < floor_ || ((a_max * top + 128) >> 8) == 0) return;   // (block-uniform: no pixel of the tile has an alpha)
  {
    const unsigned char* __restrict__ g_pal = plan.palette + (long long)plan.table[s] * 768;
    pal[tid][0] = g_pal[3 * tid];
    pal[tid][1] = g_pal[3 * tid + 1];
    pal[tid][2] = g_pal[3 * tid + 2];
  }
  __syncthreads();

  const int px = x0 + 2 * (tid & 15), py = y0 + 2 * (tid >> 4);
  int lv[5];   // the four pixels [row][column], then the block's centre (the chroma sample)
  if (smooth) {
    int jx[3], fx[3], jy[3], fy[3];   // pixel px, pixel px + 1, the centre
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      axis(2 * px + (k == 0 ? 1 : k == 1 ? 3 : 2), cell, lc, lox, jx[k], fx[k]);
      axis(2 * py + (k == 0 ? 1 : k == 1 ? 3 : 2), cell, lc, loy, jy[k], fy[k]);
    }
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      const int kx = p == 4 ? 2 : p & 1, ky = p == 4 ? 2 : p >> 1;
      // (a lane past the tile's clipped edge may form an index past the staged cells: clamped, its value is not used)
      const int ja = min(max(jx[kx], 0), ncx - 1), jb = min(max(jx[kx] + 1, 0), ncx - 1);
      const int ia = min(max(jy[ky], 0), ncy - 1), ib = min(max(jy[ky] + 1, 0), ncy - 1);
      const int wx1 = fx[kx], wx0 = 2 * cell - wx1, wy1 = fy[ky], wy0 = 2 * cell - wy1;
      const int sum = wy0 * (wx0 * level[ia * ncx + ja] + wx1 * level[ia * ncx + jb]) +
                      wy1 * (wx0 * level[ib * ncx + ja] + wx1 * level[ib * ncx + jb]);
      lv[p] = (sum + 2 * cell * cell) >> (2 + 2 * lc);
    }
  } else {
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      const int qx = px + (p == 4 ? 0 : p & 1), qy = py + (p == 4 ? 0 : p >> 1);
      const int j = min(max((qx >> lc) - lox, 0), ncx - 1), i = min(max((qy >> lc) - loy, 0), ncy - 1);
      lv[p] = level[i * ncx + j];
    }
  }
  int al[5];
#pragma unroll
  for (int p = 0; p < 5; ++p) al[p] = lv[p] < floor_ ? 0 : (a_max * lv[p] + 128) >> 8;

  unsigned char* __restrict__ dst = static_cast<unsigned char*>(plan.dst[s]);
  const long long pitch = plan.pitch[s];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int qx = px + (p & 1), qy = py + (p >> 1);
    if (qx >= W || qy >= H || al[p] == 0) continue;
    if (BGR) {
      unsigned char* o = dst + qy * pitch + 3 * qx;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)blend(o[ch], pal[lv[p]][ch], al[p]);
    } else {
      unsigned char* o = dst + qy * pitch + qx;
      o[0] = (unsigned char)blend(o[0], pal[lv[p]][0], al[p]);
    }
  }
  if (!BGR && px < W && py < H && al[4] != 0) {   // the sample of a block whose first pixel is on the map
    unsigned char* uv = dst + ((long long)plan.height[s] + (py >> 1)) * pitch + px;
    uv[0] = (unsigned char)blend(uv[0], pal[lv[4]][1], al[4]);
    uv[1] = (unsigned char)blend(uv[1], pal[lv[4]][2], al[4]);
  }
}

// A map's size, cell and grid: what both plans share.
int heat_grid_check(const char* who, const int width, const int height, const int cell) {
  if (width < 1 || height < 1 || width > PAVE_DRAW_MAX_SIZE || height > PAVE_DRAW_MAX_SIZE)
    return pave_internal_fail(PAVE_E_ARG, who);
  if (cell != 4 && cell != 8 && cell != 16 && cell != 32 && cell != 64) return pave_internal_fail(PAVE_E_ARG, who);
  if ((width + cell - 1) / cell > PAVE_HEAT_MAX_GRID || (height + cell - 1) / cell > PAVE_HEAT_MAX_GRID)
    return pave_internal_fail(PAVE_E_ARG, who);
  return PAVE_OK;
}

// Everything a draw plan could get wrong, before any device call.  bpp: bytes per pixel of a row (1 = NV12, 3 = BGR).
int heat_draw_check(const pave_heat_draw_plan* plan, const int bpp, int* max_w, int* max_h) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "draw_heat: null plan");
  if (plan->n < 1 || plan->n > PAVE_DRAW_MAX_SURFACES)
    return pave_internal_fail(PAVE_E_ARG, "draw_heat: 1 .. 32 surfaces per launch");
  if (!plan->map || !plan->peak) return pave_internal_fail(PAVE_E_ARG, "draw_heat: null map tensor");
  if (!plan->palette) return pave_internal_fail(PAVE_E_ARG, "draw_heat: null palette");
  if (plan->tables < 1 || plan->tables > PAVE_HEAT_MAX_TABLES)
    return pave_internal_fail(PAVE_E_ARG, "draw_heat: tables outside 1 .. 8");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "draw_heat: cameras outside 1 .. 4096");
  if (heat_grid_check("draw_heat: a map of 1 .. 8192 pixels, a cell of 4, 8, 16, 32 or 64, a grid of at most 512 x 512",
                      plan->map_width, plan->map_height, plan->cell) != PAVE_OK)
    return PAVE_E_ARG;
  if (plan->source < PAVE_HEAT_DWELL || plan->source > PAVE_HEAT_VISITS)
    return pave_internal_fail(PAVE_E_ARG, "draw_heat: source outside 0 .. 1");
  if (plan->full_scale < 0) return pave_internal_fail(PAVE_E_ARG, "draw_heat: full_scale below 0");
  if (plan->alpha_max < 0 || plan->alpha_max > 256) return pave_internal_fail(PAVE_E_ARG, "draw_heat: alpha_max outside 0 .. 256");
  if (plan->floor < 0 || plan->floor > 255) return pave_internal_fail(PAVE_E_ARG, "draw_heat: floor outside 0 .. 255");
  if (plan->smooth < 0 || plan->smooth > 1) return pave_internal_fail(PAVE_E_ARG, "draw_heat: smooth outside 0 .. 1");
  *max_w = *max_h = 0;
  for (int i = 0; i < plan->n; ++i) {
    const int w = plan->width[i], h = plan->height[i];
    if (!plan->dst[i]) return pave_internal_fail(PAVE_E_ARG, "draw_heat: null surface");
    if (w < 1 || h < 1 || w > PAVE_DRAW_MAX_SIZE || h > PAVE_DRAW_MAX_SIZE)
      return pave_internal_fail(PAVE_E_ARG, "draw_heat: width and height in 1 .. 8192");
    if (bpp == 1 && ((w | h) & 1)) return pave_internal_fail(PAVE_E_ARG, "draw_heat: NV12 width and height must be even");
    if (plan->pitch[i] < bpp * w) return pave_internal_fail(PAVE_E_ARG, "draw_heat: pitch below the bytes of a row");
    if (plan->table[i] >= plan->tables) return pave_internal_fail(PAVE_E_ARG, "draw_heat: palette table index >= tables");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "draw_heat: a camera index outside [0, cameras)");
    const int cw = w < plan->map_width ? w : plan->map_width, ch = h < plan->map_height ? h : plan->map_height;
    *max_w = cw > *max_w ? cw : *max_w;
    *max_h = ch > *max_h ? ch : *max_h;
  }
  return PAVE_OK;
}

template <int BGR>
int heat_draw_launch(const pave_heat_draw_plan* plan, void* stream) {
  int w = 0, h = 0;
  const int st = heat_draw_check(plan, BGR ? 3 : 1, &w, &h);
  if (st != PAVE_OK) return st;
  return pave_launch<draw_heat_kernel<BGR>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                  (unsigned)plan->n),
                                             dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // namespace

extern "C" {

int pave_heat_update(const pave_heat_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "heat_update: null plan");
  if (plan->entries < 1 || plan->entries > PAVE_TRACK_MAX_FRAMES)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: 1 .. 32 frames per launch");
  if (plan->K < 1 || plan->K > PAVE_TRACK_MAX_K) return pave_internal_fail(PAVE_E_ARG, "heat_update: K outside 1 .. 32");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: max_tracks outside 1 .. 128");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: cameras outside 1 .. 4096");
  if (!plan->slot_id || !plan->slot_last || !plan->slot_cell || !plan->frame || !plan->dropped)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: null state tensor");
  if (!plan->peak || !plan->dwell || !plan->visits) return pave_internal_fail(PAVE_E_ARG, "heat_update: null map tensor");
  if (heat_grid_check("heat_update: a map of 1 .. 8192 pixels, a cell of 4, 8, 16, 32 or 64, a grid of at most 512 x 512",
                      plan->width, plan->height, plan->cell) != PAVE_OK)
    return PAVE_E_ARG;
  if (plan->radius < 0 || plan->radius > PAVE_HEAT_MAX_RADIUS)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: radius outside 0 .. 3");
  if (plan->half_life < 0 || plan->half_life > PAVE_HEAT_MAX_HALF_LIFE)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: half_life outside 0 .. 2^18");
  if (plan->anchor < PAVE_ZONE_ANCHOR_FEET || plan->anchor > PAVE_ZONE_ANCHOR_CENTRE)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: anchor outside 0 .. 2");
  if (plan->n_anchor < 0 || plan->n_anchor > PAVE_ZONE_MAX_ANCHOR_KPTS)
    return pave_internal_fail(PAVE_E_ARG, "heat_update: n_anchor outside 0 .. 4");
  for (int i = 0; i < plan->n_anchor; ++i)
    if (plan->anchor_kpt[i] < 0 || plan->anchor_kpt[i] >= plan->K)
      return pave_internal_fail(PAVE_E_ARG, "heat_update: an anchor key point outside [0, K)");
  if (plan->max_age < 0) return pave_internal_fail(PAVE_E_ARG, "heat_update: max_age below 0");
  for (int i = 0; i < plan->entries; ++i) {
    const int n = plan->n[i];
    if (n < 0 || n > PAVE_TRACK_MAX_POSES) return pave_internal_fail(PAVE_E_ARG, "heat_update: N outside 0 .. 128");
    if (n > 0 && (!plan->kpts[i] || !plan->bboxes[i])) return pave_internal_fail(PAVE_E_ARG, "heat_update: null pose tensor");
    if (n > 0 && !plan->ids[i]) return pave_internal_fail(PAVE_E_ARG, "heat_update: null ids tensor");
    if (n > 0 && (!plan->out_cell[i] || !plan->out_dwell[i] || !plan->out_visits[i]))
      return pave_internal_fail(PAVE_E_ARG, "heat_update: null output tensor");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "heat_update: a camera index outside [0, cameras)");
    if (!(plan->scale[i][0] > 0.f && plan->scale[i][1] > 0.f && isfinite(plan->scale[i][0]) && isfinite(plan->scale[i][1])))
      return pave_internal_fail(PAVE_E_ARG, "heat_update: scale must be positive and finite");
  }
  return pave_launch<heat_update_kernel>(dim3((unsigned)plan->entries), dim3(NT), 0,
                                         reinterpret_cast<hipStream_t>(stream), *plan);
}

int pave_draw_heat_nv12(const pave_heat_draw_plan* plan, void* stream) { return heat_draw_launch<0>(plan, stream); }

int pave_draw_heat_bgr(const pave_heat_draw_plan* plan, void* stream) { return heat_draw_launch<1>(plan, stream); }

}  // extern "C"
