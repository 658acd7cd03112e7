// What the ZoneMonitor knows, in the picture: zones tinted by their state, counting lines with a stem that points the
// way a forward crossing goes, and the running counts as digits, composited into decoder-style surfaces on the device
// in one launch for up to 32 separately allocated surfaces (pave_draw_zones_nv12: pitched NV12; pave_draw_zones_bgr:
// [H, W, 3] BGR).  The geometry, the counters and the alert bits are read where pave_zone_events keeps them.
//
// The rule is DESIGN section 19 and is integer-exact.
//   fill: pixel (px, py) is the point (8 px, 8 py) in the monitor's 1/8 pixel and is inside zone z by section 17's own
//     test (even-odd, half-open, int64), so a pixel is tinted iff an anchor standing on it would count.  Zone z is
//     alerted iff a slot with id != 0 has bit z in inside and alerted (colour row 16, alpha_alert), else occupied iff
//     occupancy[z] > 0 (its colour, alpha_occupied), else its colour and alpha.  Per byte
//     out = (src (256 - a) + col a + 128) >> 8, zones one after another in ascending index; an NV12 chroma sample
//     once per zone with a_c = (a n + 2) >> 2, n of its four luma pixels inside.  An effective alpha of 0 writes nothing.
//   opaque primitives, over the fills, largest id wins (section 13's rule and capsule test, unchanged), on quarter-pixel
//     vertices Q = G >> 1 (the capsule test's squares need coordinates below 32768): zone edges (radius 2 outline,
//     id 16 z + e), lines (2 thickness, 128 + l), stems M -> T (136 + l; M = (Q(A) + Q(B)) >> 1, d = Q(B) - Q(A),
//     L = isqrt(d.d), T = clamp(M + trunc((-d.y, d.x) 4 arrow / L), 0, 32767)), and labels: a plate of g (6 n + 1) x 9 g
//     pixels whose corner is max(c - extent / 2, 0) per axis about the zone's mean vertex (floor(sum Q / nv) >> 2) or
//     the line's T >> 2 (M >> 2 without a stem), ids 144 + 2 z and 160 + 2 l, and on it the ink (+ 1): an optional
//     minus and the decimal digits of |v|, v an int32 of the counters.
//
// pave_draw.hip's tile scheme: 256 threads own a 32 x 32 pixel tile, a thread one 2 x 2 block of it (and, NV12, its
// chroma sample), so every output byte has one writer, the stores are ordinary vector stores and a byte nothing
// covers is never written.  Per block the camera's 306 geometry words and 56 counters go into LDS once, clamped as
// they are read; the alert flags are an LDS OR over the at most 128 slots; one lane per zone or line works out its
// state, its label's centre, its stem and whether its fill can touch the tile; then one lane per primitive (128 + 8
// + 8 + 32 = 176) builds it, culls it against the tile and appends it to a 256-entry LDS list (append order is
// irrelevant under the largest-id rule): one round.  A tile nothing touches ends there without a write.  Every loop
// bound is from the plan or the header's maxima, every barrier is block-uniform, there are no global atomics and no
// scratch area.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"
#include "pave_tracked.h"

namespace {

using pave_tracked::QMAX;

constexpr int TILE = 32;        // pixels per tile edge
constexpr int MAXZ = PAVE_ZONE_MAX_ZONES;
constexpr int MAXL = PAVE_ZONE_MAX_LINES;
constexpr int MAXV = PAVE_ZONE_MAX_VERTICES;
constexpr int PLATE = -1, INK = -2;
constexpr int FIRST_LINE = MAXZ * MAXV, FIRST_STEM = FIRST_LINE + MAXL, FIRST_ZONE_LABEL = FIRST_STEM + MAXL,
              FIRST_LINE_LABEL = FIRST_ZONE_LABEL + 2 * MAXZ, PRIMS = FIRST_LINE_LABEL + 2 * MAXL;
static_assert(PRIMS == 176 && PRIMS <= 256, "one lane per primitive, one round");
static_assert(PAVE_TRACK_MAX_TRACKS <= 256 && MAXZ + MAXL <= 64, "thread roles");

struct Prim {                   // one candidate of the tile's list
  short ax, ay, bx, by;         // a capsule's ends in quarter pixels; a label: its corner in pixels, n glyphs, g
  int id;
  short r;                      // quarter pixels, or PLATE | INK
  short col;                    // row of the colour table
  int v;                        // a label's value
};

// Section 13's coverage rule, all terms in int64 (|w x d| <= 2^31, its square < 2^63).
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

// |v| in unsigned arithmetic, so that -2^31 has one.
__device__ __forceinline__ unsigned magnitude(const int v) { return v < 0 ? 0u - (unsigned)v : (unsigned)v; }

// The glyphs of v: an optional minus and the decimal digits of |v|: 1 .. 11.
__device__ __forceinline__ int glyphs_of(const int v) {
  const unsigned m = magnitude(v);
  return (v < 0) + 1 + (m >= 10u) + (m >= 100u) + (m >= 1000u) + (m >= 10000u) + (m >= 100000u) + (m >= 1000000u) +
         (m >= 10000000u) + (m >= 100000000u) + (m >= 1000000000u);
}

// pave_draw.hip's label rule for pixel (qx, qy), with the minus face for the first glyph of a negative value.
__device__ __forceinline__ bool label_covers(const int kind, const int qx, const int qy, const int ax, const int ay,
                                             const int g, const int n, const int v, const unsigned char* font) {
  if (kind == PLATE) return (unsigned)(qx - ax) < (unsigned)(g * (6 * n + 1)) && (unsigned)(qy - ay) < (unsigned)(9 * g);
  const int u = qx - ax - g, w = qy - ay - g;
  if ((unsigned)u >= (unsigned)(6 * g * n) || (unsigned)w >= (unsigned)(7 * g)) return false;
  const int cell = u / (6 * g), uu = u - cell * 6 * g;
  if (uu >= 5 * g) return false;
  int face = PAVE_ZONE_DRAW_FACES - 1;
  if (!(v < 0 && cell == 0)) {
    unsigned q = magnitude(v);                                  // glyph `cell`, the most significant digit first
    for (int k = n - 1 - cell; k > 0; --k) q /= 10u;
    face = (int)(q % 10u);
  }
  return (font[face * 7 + w / g] >> (4 - uu / g)) & 1;
}

// floor(sqrt(x)), 0 <= x <= 2^31 + 2^16: the double root is within one of it.
__device__ __forceinline__ int isqrt(const long long x) {
  long long r = (long long)sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return (int)r;
}

__device__ __forceinline__ int blend(const int src, const int col, const int a) {
  return (src * (256 - a) + col * a + 128) >> 8;
}

// BGR = 0: NV12 (dst = H rows of Y, then H / 2 rows of interleaved U, V; pitch bytes per row).
// BGR = 1: [H, W, 3] bytes, pitch bytes per row.  The surface is blockIdx.z.
template <int BGR>
__global__ __launch_bounds__(256) void draw_zones_kernel(const pave_zone_draw_plan plan) {
  __shared__ int geom[PAVE_ZONE_GEOM_WORDS];
  __shared__ int cnt[PAVE_ZONE_COUNTER_WORDS];
  __shared__ Prim cand[256];
  __shared__ int n_cand, alert_bits, fill_bits;
  __shared__ short zone_col[MAXZ], zone_alpha[MAXZ];
  __shared__ short centre[MAXZ + MAXL][2];   // of a label, pixels: the zones, then the lines
  __shared__ short stem[MAXL][5];            // M.x, M.y, T.x, T.y, drawn
  __shared__ unsigned char color[PAVE_ZONE_DRAW_COLORS][4];
  __shared__ unsigned char font[PAVE_ZONE_DRAW_FACES * 7];

  const int s = blockIdx.z;
  const int W = plan.width[s], H = plan.height[s];
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  if (x0 >= W || y0 >= H) return;   // (block-uniform: before any barrier)
  const int tid = threadIdx.x;
  const int cam = plan.camera[s], S = plan.S;
  const int32_t* __restrict__ g_geom = plan.geometry + (long long)cam * PAVE_ZONE_GEOM_WORDS;
  const int32_t* __restrict__ g_count = plan.counters + (long long)cam * PAVE_ZONE_COUNTER_WORDS;
  const int32_t* __restrict__ g_id = plan.slot_id + (long long)cam * S;
  const int32_t* __restrict__ g_alerted = plan.slot_alerted + (long long)cam * S;
  const int32_t* __restrict__ g_inside = plan.slot_inside + (long long)cam * S;

  if (tid == 0) { n_cand = 0; alert_bits = 0; fill_bits = 0; }
  for (int i = tid; i < PAVE_ZONE_GEOM_WORDS; i += 256) {   // the geometry, clamped as it is read
    int v = g_geom[i];
    if (i == PAVE_ZONE_GEOM_NZONES) v = min(max(v, 0), MAXZ);
    else if (i == PAVE_ZONE_GEOM_NLINES) v = min(max(v, 0), MAXL);
    else if (i >= PAVE_ZONE_GEOM_NVERT && i < PAVE_ZONE_GEOM_NVERT + MAXZ) v = min(max(v, 0), MAXV);
    else if (i >= PAVE_ZONE_GEOM_ZONES) v = min(max(v, 0), 65535);
    geom[i] = v;
  }
  if (tid < PAVE_ZONE_COUNTER_WORDS) cnt[tid] = g_count[tid];
  if (tid >= 64 && tid < 64 + PAVE_ZONE_DRAW_COLORS) {
    const int i = tid - 64, tab = plan.table[s];
    color[i][0] = plan.color[tab][i][0];
    color[i][1] = plan.color[tab][i][1];
    color[i][2] = plan.color[tab][i][2];
  }
  if (tid >= 128 && tid < 128 + PAVE_ZONE_DRAW_FACES * 7) font[tid - 128] = plan.font[(tid - 128) / 7][(tid - 128) % 7];
  __syncthreads();
  if (tid < S && g_id[tid] != 0) {   // a free slot's fields are never trusted
    const int bits = g_inside[tid] & g_alerted[tid] & 0xff;
    if (bits != 0) atomicOr(&alert_bits, bits);
  }
  __syncthreads();

  const int nz = geom[PAVE_ZONE_GEOM_NZONES], nl = geom[PAVE_ZONE_GEOM_NLINES];
  const int g = plan.label_scale;
  const int xe = min(x0 + TILE, W), ye = min(y0 + TILE, H);
  // the tile's pixels as points, clipped to the surface, in quarter pixels
  const int tx0 = 4 * x0, ty0 = 4 * y0, tx1 = 4 * (xe - 1), ty1 = 4 * (ye - 1);

  // ---- one lane per zone or line: state, label centre, stem, fill cull ----
  if (tid < MAXZ) {
    const int z = tid, nv = geom[PAVE_ZONE_GEOM_NVERT + z];
    int col = z, a = plan.alpha;
    if (cnt[PAVE_ZONE_CNT_OCCUPANCY + z] > 0) a = plan.alpha_occupied;
    if ((alert_bits >> z) & 1) { col = PAVE_ZONE_DRAW_ALERT; a = plan.alpha_alert; }
    zone_col[z] = (short)col;
    zone_alpha[z] = (short)a;
    int cx = 0, cy = 0;
    if (z < nz && nv > 0) {
      const int* v = geom + PAVE_ZONE_GEOM_ZONES + z * MAXV * 2;
      int lox = 65535, loy = 65535, hix = 0, hiy = 0, sum_x = 0, sum_y = 0;
      for (int i = 0; i < nv; ++i) {
        lox = min(lox, v[2 * i]); hix = max(hix, v[2 * i]);
        loy = min(loy, v[2 * i + 1]); hiy = max(hiy, v[2 * i + 1]);
        sum_x += v[2 * i] >> 1;
        sum_y += v[2 * i + 1] >> 1;
      }
      cx = (sum_x / nv) >> 2;   // (sums >= 0: / is floor)
      cy = (sum_y / nv) >> 2;
      // a pixel's point can be inside only within the bounding box of the vertices
      if (a > 0 && lox <= 8 * (xe - 1) && hix >= 8 * x0 && loy <= 8 * (ye - 1) && hiy >= 8 * y0) atomicOr(&fill_bits, 1 << z);
    }
    centre[z][0] = (short)cx;
    centre[z][1] = (short)cy;
  } else if (tid < MAXZ + MAXL) {
    const int l = tid - MAXZ;
    const int* ln = geom + PAVE_ZONE_GEOM_LINES + l * 4;
    const int ax = ln[0] >> 1, ay = ln[1] >> 1, bx = ln[2] >> 1, by = ln[3] >> 1;
    const int mx = (ax + bx) >> 1, my = (ay + by) >> 1, dx = bx - ax, dy = by - ay;
    int tx = mx, ty = my, drawn = 0;
    if (plan.arrow > 0 && (dx != 0 || dy != 0)) {
      const int L = isqrt((long long)dx * dx + (long long)dy * dy);   // >= 1
      tx = min(max(mx + (-dy * 4 * plan.arrow) / L, 0), QMAX);        // (/ truncates)
      ty = min(max(my + (dx * 4 * plan.arrow) / L, 0), QMAX);
      drawn = 1;
    }
    stem[l][0] = (short)mx; stem[l][1] = (short)my; stem[l][2] = (short)tx; stem[l][3] = (short)ty;
    stem[l][4] = (short)drawn;
    centre[MAXZ + l][0] = (short)(tx >> 2);
    centre[MAXZ + l][1] = (short)(ty >> 2);
  }
  __syncthreads();

  // ---- one lane per primitive: build, cull, append ----
  if (tid < PRIMS) {
    Prim c;
    c.v = 0;
    bool on = false;
    if (tid < FIRST_ZONE_LABEL) {
      int ax = 0, ay = 0, bx = 0, by = 0, r = 0;
      if (tid < FIRST_LINE) {
        const int z = tid >> 4, e = tid & 15, nv = geom[PAVE_ZONE_GEOM_NVERT + z];
        if (z < nz && e < nv && plan.outline > 0) {
          const int* v = geom + PAVE_ZONE_GEOM_ZONES + z * MAXV * 2;
          const int f = e + 1 < nv ? e + 1 : 0;
          ax = v[2 * e] >> 1; ay = v[2 * e + 1] >> 1; bx = v[2 * f] >> 1; by = v[2 * f + 1] >> 1;
          r = 2 * plan.outline;
          c.col = zone_col[z];
          on = true;
        }
      } else if (tid < FIRST_STEM) {
        const int l = tid - FIRST_LINE;
        if (l < nl) {
          const int* ln = geom + PAVE_ZONE_GEOM_LINES + l * 4;
          ax = ln[0] >> 1; ay = ln[1] >> 1; bx = ln[2] >> 1; by = ln[3] >> 1;
          r = 2 * plan.thickness;
          c.col = (short)(MAXZ + l);
          on = true;
        }
      } else {
        const int l = tid - FIRST_STEM;
        if (l < nl && stem[l][4] != 0) {
          ax = stem[l][0]; ay = stem[l][1]; bx = stem[l][2]; by = stem[l][3];
          r = 2 * plan.thickness;
          c.col = (short)(MAXZ + l);
          on = true;
        }
      }
      on = on && min(ax, bx) - r <= tx1 && max(ax, bx) + r >= tx0 && min(ay, by) - r <= ty1 && max(ay, by) + r >= ty0;
      c.ax = (short)ax; c.ay = (short)ay; c.bx = (short)bx; c.by = (short)by;
      c.r = (short)r;
    } else {
      const bool line = tid >= FIRST_LINE_LABEL;
      const int j = (tid - (line ? FIRST_LINE_LABEL : FIRST_ZONE_LABEL)) >> 1, kind = (tid & 1) ? INK : PLATE;
      int v = 0;
      bool labelled = g >= 1;
      if (line) {
        const unsigned fwd = (unsigned)cnt[PAVE_ZONE_CNT_CROSSED + 2 * j], back = (unsigned)cnt[PAVE_ZONE_CNT_CROSSED + 2 * j + 1];
        v = plan.line_label == PAVE_LINE_LABEL_NET ? (int)(fwd - back) : plan.line_label == PAVE_LINE_LABEL_FORWARD ? (int)fwd : (int)back;
        labelled = labelled && j < nl && plan.line_label != PAVE_LINE_LABEL_NONE;
      } else {
        v = plan.zone_label == PAVE_ZONE_LABEL_ENTERED
                ? (int)((unsigned)cnt[PAVE_ZONE_CNT_ENTERED + j] + (unsigned)cnt[PAVE_ZONE_CNT_APPEARED + j])
                : cnt[PAVE_ZONE_CNT_OCCUPANCY + j];
        labelled = labelled && j < nz && geom[PAVE_ZONE_GEOM_NVERT + j] > 0 && plan.zone_label != PAVE_ZONE_LABEL_NONE;
      }
      if (labelled) {
        const int n = glyphs_of(v), k = line ? MAXZ + j : j;
        const int lx = max(centre[k][0] - ((g * (6 * n + 1)) >> 1), 0), ly = max(centre[k][1] - ((9 * g) >> 1), 0);
        // the rectangle that can be covered, in pixels: the plate, or the ink's field inside it
        const int rx0 = kind == PLATE ? lx : lx + g, rx1 = kind == PLATE ? lx + g * (6 * n + 1) : lx + g + 6 * g * n;
        const int ry0 = kind == PLATE ? ly : ly + g, ry1 = kind == PLATE ? ly + 9 * g : ly + 8 * g;
        on = rx0 < xe && rx1 > x0 && ry0 < ye && ry1 > y0;
        c.ax = (short)lx; c.ay = (short)ly; c.bx = (short)n; c.by = (short)g;
        c.r = (short)kind;
        c.col = kind == INK ? (short)PAVE_ZONE_DRAW_INK : line ? (short)(MAXZ + j) : zone_col[j];
        c.v = v;
      }
    }
    if (on) {
      c.id = tid;   // 16 z + e | 128 + l | 136 + l | 144 + 2 z (+ 1) | 160 + 2 l (+ 1)
      cand[atomicAdd(&n_cand, 1)] = c;
    }
  }
  __syncthreads();
  const int nc = n_cand, fills = fill_bits;
  if (nc == 0 && fills == 0) return;   // (block-uniform: nothing touches the tile)

  // ---- this lane's 2 x 2 pixels against the list ----
  const int px = x0 + 2 * (tid & 15), py = y0 + 2 * (tid >> 4);
  int best00 = -1, best01 = -1, best10 = -1, best11 = -1;   // [row][column]
  int col00 = 0, col01 = 0, col10 = 0, col11 = 0;
  for (int i = 0; i < nc; ++i) {
    const Prim c = cand[i];
    if (c.r < 0) {   // a label (the same entry in every lane: no divergence on this branch)
      if (c.id > best00 && label_covers(c.r, px, py, c.ax, c.ay, c.by, c.bx, c.v, font)) { best00 = c.id; col00 = c.col; }
      if (c.id > best01 && label_covers(c.r, px + 1, py, c.ax, c.ay, c.by, c.bx, c.v, font)) { best01 = c.id; col01 = c.col; }
      if (c.id > best10 && label_covers(c.r, px, py + 1, c.ax, c.ay, c.by, c.bx, c.v, font)) { best10 = c.id; col10 = c.col; }
      if (c.id > best11 && label_covers(c.r, px + 1, py + 1, c.ax, c.ay, c.by, c.bx, c.v, font)) { best11 = c.id; col11 = c.col; }
      continue;
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

  // ---- the fills: this lane's pixels inside every zone that can touch the tile ----
  // in[z]: bit 0 (px, py), 1 (px + 1, py), 2 (px, py + 1), 3 (px + 1, py + 1)
  unsigned char* __restrict__ dst = static_cast<unsigned char*>(plan.dst[s]);
  const long long pitch = plan.pitch[s];
  const bool ok00 = px < W && py < H, ok01 = px + 1 < W && py < H, ok10 = px < W && py + 1 < H,
             ok11 = px + 1 < W && py + 1 < H;
  int tint = 0;                 // bit p: a fill wrote pixel p; bit 4: the chroma sample
  int val[4][3];                // BGR: the pixels' bytes; NV12: [p][0] the lumas, [0][1], [0][2] the chroma sample
#pragma unroll
  for (int p = 0; p < 4; ++p) val[p][0] = val[p][1] = val[p][2] = 0;
  if (fills != 0) {
    if (BGR) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool ok = p == 0 ? ok00 : p == 1 ? ok01 : p == 2 ? ok10 : ok11;
        if (ok) {
          const unsigned char* o = dst + (py + (p >> 1)) * pitch + 3 * (px + (p & 1));
          val[p][0] = o[0]; val[p][1] = o[1]; val[p][2] = o[2];
        }
      }
    } else if (ok00) {   // W and H are even: the 2 x 2 block is inside or outside as a whole
      const unsigned char* y = dst + py * pitch + px;
      const unsigned char* uv = dst + ((long long)H + (py >> 1)) * pitch + px;
      val[0][0] = y[0]; val[1][0] = y[1]; val[2][0] = y[pitch]; val[3][0] = y[pitch + 1];
      val[0][1] = uv[0]; val[0][2] = uv[1];
    }
    const long long X0 = 8ll * px, Y0 = 8ll * py;
    for (int z = 0; z < nz; ++z) {
      if (!((fills >> z) & 1)) continue;   // (block-uniform)
      const int nv = geom[PAVE_ZONE_GEOM_NVERT + z];
      const int* v = geom + PAVE_ZONE_GEOM_ZONES + z * MAXV * 2;
      int in = 0;
      for (int i = 0; i < nv; ++i) {
        const int f = i + 1 < nv ? i + 1 : 0;
        const long long ex = v[2 * i], ey = v[2 * i + 1], fx = v[2 * f], fy = v[2 * f + 1];
        const long long dy = fy - ey, dx = fx - ex;
#pragma unroll
        for (int row = 0; row < 2; ++row) {
          const long long Y = Y0 + 8 * row;
          if ((ey > Y) != (fy > Y)) {
            const long long t0 = (X0 - ex) * dy - (Y - ey) * dx, t1 = t0 + 8 * dy;
            if (dy > 0 ? t0 < 0 : t0 > 0) in ^= 1 << (2 * row);
            if (dy > 0 ? t1 < 0 : t1 > 0) in ^= 2 << (2 * row);
          }
        }
      }
      const int a = zone_alpha[z], col = zone_col[z];
      if (BGR) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if ((in >> p) & 1) {
            tint |= 1 << p;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) val[p][ch] = blend(val[p][ch], color[col][ch], a);
          }
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if ((in >> p) & 1) {
            tint |= 1 << p;
            val[p][0] = blend(val[p][0], color[col][0], a);
          }
        const int ac = (a * __popc(in) + 2) >> 2;
        if (ac > 0) {
          tint |= 16;
          val[0][1] = blend(val[0][1], color[col][1], ac);
          val[0][2] = blend(val[0][2], color[col][2], ac);
        }
      }
    }
  }

  // ---- the stores: covered bytes only ----
  if (BGR) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool ok = p == 0 ? ok00 : p == 1 ? ok01 : p == 2 ? ok10 : ok11;
      const int best = p == 0 ? best00 : p == 1 ? best01 : p == 2 ? best10 : best11;
      const int col = p == 0 ? col00 : p == 1 ? col01 : p == 2 ? col10 : col11;
      if (!ok) continue;
      unsigned char* o = dst + (py + (p >> 1)) * pitch + 3 * (px + (p & 1));
      if (best >= 0) {
        o[0] = color[col][0]; o[1] = color[col][1]; o[2] = color[col][2];
      } else if ((tint >> p) & 1) {
        o[0] = (unsigned char)val[p][0]; o[1] = (unsigned char)val[p][1]; o[2] = (unsigned char)val[p][2];
      }
    }
  } else if (ok00) {
    unsigned char* y = dst + py * pitch + px;
    if (best00 >= 0) y[0] = color[col00][0]; else if (tint & 1) y[0] = (unsigned char)val[0][0];
    if (best01 >= 0) y[1] = color[col01][0]; else if (tint & 2) y[1] = (unsigned char)val[1][0];
    if (best10 >= 0) y[pitch] = color[col10][0]; else if (tint & 4) y[pitch] = (unsigned char)val[2][0];
    if (best11 >= 0) y[pitch + 1] = color[col11][0]; else if (tint & 8) y[pitch + 1] = (unsigned char)val[3][0];
    int m = best00, mc = col00;
    if (best01 > m) { m = best01; mc = col01; }
    if (best10 > m) { m = best10; mc = col10; }
    if (best11 > m) { m = best11; mc = col11; }
    unsigned char* uv = dst + ((long long)H + (py >> 1)) * pitch + px;
    if (m >= 0) {
      uv[0] = color[mc][1];
      uv[1] = color[mc][2];
    } else if (tint & 16) {
      uv[0] = (unsigned char)val[0][1];
      uv[1] = (unsigned char)val[0][2];
    }
  }
}

// Everything a plan could get wrong, before any device call.  bpp: bytes per pixel of a row (1 = NV12, 3 = BGR).
int zone_draw_check(const pave_zone_draw_plan* plan, const int bpp, int* max_w, int* max_h) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "draw_zones: null plan");
  if (plan->n < 1 || plan->n > PAVE_DRAW_MAX_SURFACES)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: 1 .. 32 surfaces per launch");
  if (!plan->geometry || !plan->counters || !plan->slot_id || !plan->slot_alerted || !plan->slot_inside)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: null monitor tensor");
  if (plan->cameras < 1 || plan->cameras > PAVE_TRACK_MAX_CAMERAS)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: cameras outside 1 .. 4096");
  if (plan->S < 1 || plan->S > PAVE_TRACK_MAX_TRACKS)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: max_tracks outside 1 .. 128");
  if (plan->alpha < 0 || plan->alpha > 256 || plan->alpha_occupied < 0 || plan->alpha_occupied > 256 ||
      plan->alpha_alert < 0 || plan->alpha_alert > 256)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: an alpha outside 0 .. 256");
  if (plan->outline < 0 || plan->outline > 32) return pave_internal_fail(PAVE_E_ARG, "draw_zones: outline outside 0 .. 32");
  if (plan->thickness < 1 || plan->thickness > 32)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: thickness outside 1 .. 32");
  if (plan->arrow < 0 || plan->arrow > 255) return pave_internal_fail(PAVE_E_ARG, "draw_zones: arrow outside 0 .. 255");
  if (plan->label_scale < 0 || plan->label_scale > 8)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: label_scale outside 0 .. 8");
  if (plan->zone_label < PAVE_ZONE_LABEL_NONE || plan->zone_label > PAVE_ZONE_LABEL_ENTERED)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: zone_label outside 0 .. 2");
  if (plan->line_label < PAVE_LINE_LABEL_NONE || plan->line_label > PAVE_LINE_LABEL_BACKWARD)
    return pave_internal_fail(PAVE_E_ARG, "draw_zones: line_label outside 0 .. 3");
  for (int d = 0; d < PAVE_ZONE_DRAW_FACES; ++d)
    for (int row = 0; row < 7; ++row)
      if (plan->font[d][row] & ~0x1f) return pave_internal_fail(PAVE_E_ARG, "draw_zones: a font row has bits above the low 5");
  *max_w = *max_h = 0;
  for (int i = 0; i < plan->n; ++i) {
    const int w = plan->width[i], h = plan->height[i];
    if (!plan->dst[i]) return pave_internal_fail(PAVE_E_ARG, "draw_zones: null surface");
    if (w < 1 || h < 1 || w > PAVE_DRAW_MAX_SIZE || h > PAVE_DRAW_MAX_SIZE)
      return pave_internal_fail(PAVE_E_ARG, "draw_zones: width and height in 1 .. 8192");
    if (bpp == 1 && ((w | h) & 1)) return pave_internal_fail(PAVE_E_ARG, "draw_zones: NV12 width and height must be even");
    if (plan->pitch[i] < bpp * w) return pave_internal_fail(PAVE_E_ARG, "draw_zones: pitch below the bytes of a row");
    if (plan->table[i] >= PAVE_DRAW_MAX_TABLES) return pave_internal_fail(PAVE_E_ARG, "draw_zones: colour table index >= 4");
    if (plan->camera[i] < 0 || plan->camera[i] >= plan->cameras)
      return pave_internal_fail(PAVE_E_ARG, "draw_zones: a camera index outside [0, cameras)");
    *max_w = w > *max_w ? w : *max_w;
    *max_h = h > *max_h ? h : *max_h;
  }
  return PAVE_OK;
}

template <int BGR>
int zone_draw_launch(const pave_zone_draw_plan* plan, void* stream) {
  int w = 0, h = 0;
  const int st = zone_draw_check(plan, BGR ? 3 : 1, &w, &h);
  if (st != PAVE_OK) return st;
  return pave_launch<draw_zones_kernel<BGR>>(dim3((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE),
                                                   (unsigned)plan->n),
                                              dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // namespace

extern "C" {

int pave_draw_zones_nv12(const pave_zone_draw_plan* plan, void* stream) { return zone_draw_launch<0>(plan, stream); }

int pave_draw_zones_bgr(const pave_zone_draw_plan* plan, void* stream) { return zone_draw_launch<1>(plan, stream); }

}  // extern "C"
