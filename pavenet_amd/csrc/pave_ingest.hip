// Ingest of decoder surfaces: NV12 (pitched 8-bit Y plane, interleaved half-resolution U, V plane) straight into
// the network's input canvas, in one launch for T surfaces of one allocation (pave_preprocess_frames_nv12) or for
// up to 32 separately allocated surfaces of several cameras (pave_preprocess_surfaces_nv12); and the ring write of
// the live path (pave_scatter_rows_f32): freshly encoded frames into their rows of up to 8 tensors in one launch.
//
// A source pixel is converted to the 8-bit BGR value a software conversion would have stored:
//   t = (Y - yoff) * cy;  B = t + (U - 128) * cbu;  G = (t + (U - 128) * cgu) + (V - 128) * cgv;
//   R = t + (V - 128) * crv;  each rounded to nearest even and clamped to [0, 255],
// chroma taken from block (y >> 1, x >> 1) (nearest: no chroma interpolation).  From that value on the arithmetic
// is preprocess_frames_kernel's (pave_kernels.hip), operation for operation: OpenCV's float INTER_LINEAR, optional
// BGR -> RGB, (x - mean) * std_inv, zero pad, HWC -> CHW.  Contraction is off, so every product and sum is rounded
// to fp32 on its own and the output equals pave_preprocess_frames(src_is_u8 = 1) on the converted image bit for
// bit.  One thread per output pixel; its four bilinear taps each fetch Y, U, V and convert.  The kernel reads
// 1.5 B per source pixel and writes 12 B per canvas pixel: bandwidth-bound, no LDS.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"

namespace {

struct Csc {
  float yoff, cy, crv, cgu, cgv, cbu;
};

// One source pixel of an NV12 surface -> its 8-bit B, G, R as floats.
__device__ __forceinline__ void nv12_bgr(const unsigned char* __restrict__ luma, const unsigned char* __restrict__ chroma,
                                         const int pitch, const int y, const int x, const Csc k, float* bgr) {
#pragma clang fp contract(off)
  const float Y = (float)luma[(long long)y * pitch + x];
  const unsigned char* uv = chroma + (long long)(y >> 1) * pitch + ((x >> 1) << 1);
  const float u = (float)uv[0] - 128.f, v = (float)uv[1] - 128.f;
  const float ys = Y - k.yoff;
  const float t = ys * k.cy;
  const float ub = u * k.cbu, ug = u * k.cgu, vg = v * k.cgv, vr = v * k.crv;
  const float b = t + ub;
  const float g0 = t + ug;
  const float g = g0 + vg;
  const float r = t + vr;
  bgr[0] = fminf(fmaxf(rintf(b), 0.f), 255.f);
  bgr[1] = fminf(fmaxf(rintf(g), 0.f), 255.f);
  bgr[2] = fminf(fmaxf(rintf(r), 0.f), 255.f);
}

// One canvas pixel (x, y) of one surface: from the source coordinates to the three stores.  Both ingest kernels
// call it, so a surface gives the same bits whichever launch it goes through.
__device__ __forceinline__ void nv12_canvas_pixel(
    const unsigned char* __restrict__ luma, const int pitch, float* __restrict__ out, const int x, const int y,
    const int H0, const int W0, const int Hn, const int Wn, const int Hp, const int Wp, const double scx,
    const double scy, const Csc k, const float m0, const float m1, const float m2, const float s0, const float s1,
    const float s2, const int to_rgb) {
#pragma clang fp contract(off)   // every product and sum below is rounded on its own (no FMA)
  float c[3] = {0.f, 0.f, 0.f};
  if (x < Wn && y < Hn) {
    float fx = (float)(((double)x + 0.5) * scx - 0.5), fy = (float)(((double)y + 0.5) * scy - 0.5);
    int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    fx = fx - (float)x0;
    fy = fy - (float)y0;
    if (x0 < 0) { x0 = 0; fx = 0.f; }
    if (x0 >= W0 - 1) { x0 = W0 - 1; fx = 0.f; }
    if (y0 < 0) { y0 = 0; fy = 0.f; }
    if (y0 >= H0 - 1) { y0 = H0 - 1; fy = 0.f; }
    const int x1 = min(x0 + 1, W0 - 1), y1 = min(y0 + 1, H0 - 1);
    const float gx = 1.f - fx, gy = 1.f - fy;
    const unsigned char* chroma = luma + (long long)H0 * pitch;
    float a[3], b[3], cc[3], d[3];
    nv12_bgr(luma, chroma, pitch, y0, x0, k, a);
    nv12_bgr(luma, chroma, pitch, y0, x1, k, b);
    nv12_bgr(luma, chroma, pitch, y1, x0, k, cc);
    nv12_bgr(luma, chroma, pitch, y1, x1, k, d);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float t0 = a[ch] * gx, t1 = b[ch] * fx, b0 = cc[ch] * gx, b1 = d[ch] * fx;
      const float top = t0 + t1, bot = b0 + b1;
      const float u0 = top * gy, u1 = bot * fy;
      c[ch] = u0 + u1;
    }
    if (to_rgb) {
      const float tmp = c[0];
      c[0] = c[2];
      c[2] = tmp;
    }
    c[0] = (c[0] - m0) * s0;   // mmcv.imnormalize: subtract, then multiply
    c[1] = (c[1] - m1) * s1;
    c[2] = (c[2] - m2) * s2;
  }
  const long long plane = (long long)Hp * Wp;
  float* o = out + (long long)y * Wp + x;
  o[0] = c[0];
  o[plane] = c[1];
  o[2 * plane] = c[2];
}

__global__ __launch_bounds__(256) void preprocess_frames_nv12_kernel(
    const unsigned char* __restrict__ src, const long long frame_stride, const int pitch, float* __restrict__ dst,
    const int T, const int H0, const int W0, const int Hn, const int Wn, const int Hp, const int Wp, const Csc k,
    const float m0, const float m1, const float m2, const float s0, const float s1, const float s2,
    const int to_rgb) {
  const long long n = (long long)T * Hp * Wp;
  // the source coordinates of preprocess_frames_kernel (OpenCV's published order, in double)
  const double scx = 1.0 / ((double)Wn / (double)W0), scy = 1.0 / ((double)Hn / (double)H0);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % Wp);
    const int y = (int)((i / Wp) % Hp);
    const int t = (int)(i / ((long long)Wp * Hp));
    nv12_canvas_pixel(src + (long long)t * frame_stride, pitch, dst + (long long)t * 3 * Hp * Wp, x, y, H0, W0, Hn,
                      Wn, Hp, Wp, scx, scy, k, m0, m1, m2, s0, s1, s2, to_rgb);
  }
}

// The same for separately allocated surfaces, each with its own pitch and coefficients.  The surface is
// blockIdx.y, so what a block reads from the by-value plan is wave-uniform (scalar loads from the kernel
// arguments); a per-lane index into the plan's arrays would copy the plan to scratch.
__global__ __launch_bounds__(256) void preprocess_surfaces_nv12_kernel(
    const pave_ingest_plan plan, float* __restrict__ dst, const int H0, const int W0, const int Hn, const int Wn,
    const int Hp, const int Wp, const float m0, const float m1, const float m2, const float s0, const float s1,
    const float s2, const int to_rgb) {
  const int t = blockIdx.y;
  const unsigned char* luma = static_cast<const unsigned char*>(plan.src[t]);
  const int pitch = plan.pitch[t];
  const Csc k = {plan.csc[t][0], plan.csc[t][1], plan.csc[t][2], plan.csc[t][3], plan.csc[t][4], plan.csc[t][5]};
  const int n = Hp * Wp;
  const double scx = 1.0 / ((double)Wn / (double)W0), scy = 1.0 / ((double)Hn / (double)H0);
  float* out = dst + (long long)t * 3 * Hp * Wp;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    nv12_canvas_pixel(luma, pitch, out, i % Wp, i / Wp, H0, W0, Hn, Wn, Hp, Wp, scx, scy, k, m0, m1, m2, s0, s1, s2,
                      to_rgb);
}

// Row scatter: dst[z][row[y]] = src[z][y] for k tensors of one row size, 16 bytes per lane and access.  The source
// row is blockIdx.y and the tensor blockIdx.z: pointers and the destination row come from the by-value plan through
// scalar loads.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const pave_scatter_plan plan) {
  const int i = blockIdx.y, z = blockIdx.z;
  const long long n4 = plan.row_elems >> 2;
  const float4* __restrict__ s = static_cast<const float4*>(plan.src[z]) + (long long)i * n4;
  float4* __restrict__ d = static_cast<float4*>(plan.dst[z]) + (long long)plan.row[i] * n4;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n4; j += (long long)gridDim.x * blockDim.x)
    d[j] = s[j];
}

}  // namespace

extern "C" {

int pave_preprocess_frames_nv12(const void* src, long long frame_stride, int pitch, float* dst, int T, int H0,
                                int W0, int Hn, int Wn, int Hp, int Wp, const float* csc, const float* mean,
                                const float* std, int to_rgb, void* stream) {
  if (!src || !dst || !csc || !mean || !std) return pave_internal_fail(PAVE_E_ARG, "preprocess_frames_nv12: null pointer");
  if (T <= 0 || H0 <= 0 || W0 <= 0 || Hn <= 0 || Wn <= 0 || Hp < Hn || Wp < Wn)
    return pave_internal_fail(PAVE_E_ARG, "preprocess_frames_nv12: bad sizes");
  if ((H0 & 1) || (W0 & 1)) return pave_internal_fail(PAVE_E_ARG, "preprocess_frames_nv12: H0 and W0 must be even");
  if (pitch < W0 || frame_stride < (long long)pitch * (H0 + H0 / 2))
    return pave_internal_fail(PAVE_E_ARG, "preprocess_frames_nv12: pitch >= W0 and frame_stride >= pitch * H0 * 3 / 2");
  const long long n = (long long)T * Hp * Wp;
  long long nb = (n + 255) / 256;
  if (nb > 256 * 32) nb = 256 * 32;
  const float s0 = (float)(1.0 / (double)std[0]), s1 = (float)(1.0 / (double)std[1]),
              s2 = (float)(1.0 / (double)std[2]);
  const Csc k = {csc[0], csc[1], csc[2], csc[3], csc[4], csc[5]};
  return pave_launch<preprocess_frames_nv12_kernel>(
      dim3((unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), static_cast<const unsigned char*>(src),
      frame_stride, pitch, dst, T, H0, W0, Hn, Wn, Hp, Wp, k, mean[0], mean[1], mean[2], s0, s1, s2, to_rgb);
}

int pave_preprocess_surfaces_nv12(const pave_ingest_plan* plan, float* dst, int H0, int W0, int Hn, int Wn, int Hp,
                                  int Wp, const float* mean, const float* std, int to_rgb, void* stream) {
  if (!plan || !dst || !mean || !std) return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: null pointer");
  if (plan->n < 1 || plan->n > PAVE_INGEST_MAX_SURFACES)
    return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: 1 .. 32 surfaces per launch");
  if (H0 <= 0 || W0 <= 0 || Hn <= 0 || Wn <= 0 || Hp < Hn || Wp < Wn)
    return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: bad sizes");
  if ((H0 & 1) || (W0 & 1)) return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: H0 and W0 must be even");
  if ((long long)Hp * Wp >= (1ll << 31)) return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: canvas too large");
  for (int i = 0; i < plan->n; ++i) {
    if (!plan->src[i]) return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: null surface");
    if (plan->pitch[i] < W0) return pave_internal_fail(PAVE_E_ARG, "preprocess_surfaces_nv12: pitch >= W0");
  }
  long long nb = ((long long)Hp * Wp + 255) / 256;
  if (nb > 256 * 32) nb = 256 * 32;
  const float s0 = (float)(1.0 / (double)std[0]), s1 = (float)(1.0 / (double)std[1]),
              s2 = (float)(1.0 / (double)std[2]);
  return pave_launch<preprocess_surfaces_nv12_kernel>(
      dim3((unsigned)nb, (unsigned)plan->n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *plan, dst, H0, W0,
      Hn, Wn, Hp, Wp, mean[0], mean[1], mean[2], s0, s1, s2, to_rgb);
}

int pave_scatter_rows_f32(const pave_scatter_plan* plan, void* stream) {
  if (!plan) return pave_internal_fail(PAVE_E_ARG, "scatter_rows: null plan");
  const int n = plan->n, k = plan->k;
  if (n < 1 || n > PAVE_SCATTER_MAX_ROWS || k < 1 || k > PAVE_SCATTER_MAX_TENSORS || plan->dst_rows < 1 ||
      plan->row_elems < 1)
    return pave_internal_fail(PAVE_E_ARG, "scatter_rows: 1 .. 64 rows, 1 .. 8 tensors, dst_rows and row_elems positive");
  if (plan->row_elems % 4 != 0) return pave_internal_fail(PAVE_E_ARG, "scatter_rows: row_elems must be a multiple of 4");
  for (int t = 0; t < k; ++t) {
    if (!plan->src[t] || !plan->dst[t]) return pave_internal_fail(PAVE_E_ARG, "scatter_rows: null tensor");
    if ((reinterpret_cast<uintptr_t>(plan->src[t]) | reinterpret_cast<uintptr_t>(plan->dst[t])) & 15)
      return pave_internal_fail(PAVE_E_ARG, "scatter_rows: tensors must be 16-byte aligned");
  }
  for (int i = 0; i < n; ++i) {
    if (plan->row[i] < 0 || plan->row[i] >= plan->dst_rows)
      return pave_internal_fail(PAVE_E_ARG, "scatter_rows: a row outside [0, dst_rows)");
    for (int j = 0; j < i; ++j)   // a duplicate makes the result depend on block order
      if (plan->row[j] == plan->row[i]) return pave_internal_fail(PAVE_E_ARG, "scatter_rows: duplicate destination row");
  }
  long long nb = (plan->row_elems / 4 + 255) / 256;
  if (nb > 1024) nb = 1024;
  return pave_launch<scatter_rows_kernel>(dim3((unsigned)nb, (unsigned)n, (unsigned)k), dim3(256), 0,
                                          reinterpret_cast<hipStream_t>(stream), *plan);
}

}  // extern "C"
