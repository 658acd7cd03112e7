// Test-time augmentation on the device: the merge of the per-augmentation results with box NMS
// (pave_aug_merge_nms_f32) and the horizontal flip of preprocessed canvases (pave_hflip_canvas_f32).
//
// Restates, for one launch over B images:
//   opera/models/detectors/petr.py:118-187 (merge_aug_results + aug_test's merge),
//   mmdet/core/bbox/transforms.py:22-72 (bbox_flip, bbox_mapping_back),
//   opera/core/keypoint/transforms.py:157-192 (kpt_flip, kpt_mapping_back),
//   mmdet/core/post_processing/bbox_nms.py:8-93 (multiclass_nms, one class, return_inds),
//   mmcv/ops/nms.py:264-370 (batched_nms: a single class has offset 0) and
//   mmcv/ops/csrc/pytorch/cpu/nms.cpp:5-160 (nms_cpu, softnms_cpu).
// The whole arithmetic runs with contraction off, in the reference's operation order, so that hard,
// naive and linear results are bit-equal to an fp32 host restatement (gaussian goes through expf).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pave_hip.h"
#include "pave_internal.h"

namespace {

constexpr int kMaxBoxes = 4096;   // A * N per image: the image's boxes live in LDS (36 B per box)
constexpr int kMaxPerThread = 4;  // contiguous scan items per thread (threads = n / 4, 64 .. 1024)

// std::max / std::min of the C++ loop (NaN handling included: the first operand wins unless the test holds)
__device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float smin(float a, float b) { return (b < a) ? b : a; }

// Exclusive prefix sum of `v` over the block (thread order), and the block total.  Every thread calls it.
__device__ int block_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int off = 0, tot = 0;
  for (int k = 0; k < nw; ++k) {
    const int s = wsum[k];
    off += (k < w) ? s : 0;
    tot += s;
  }
  __syncthreads();   // wsum is reused by the next call
  *total = tot;
  return off + x - v;
}

struct AugLds {
  float *x1, *y1, *x2, *y2, *sc;
  int *idx;   // index into the concatenated (kept) rows of all augmentations: the reference's `inds`
  int *src;   // aug * N + row: where the box's key points are read from
  int *aux0, *aux1;   // hard: score order (then the kept positions), dead flags; soft: aux1 = fillers by back rank
  int* wsum;          // [16] scan / reduction scratch
  float* rs;          // [16] argmax scratch (scores)
  int* rp;            // [16] argmax scratch (positions)
};

__device__ __forceinline__ float box_area(const AugLds& L, int p, float off) {
#pragma clang fp contract(off)
  return (L.x2[p] - L.x1[p] + off) * (L.y2[p] - L.y1[p] + off);   // nms.cpp: areas_t
}

__device__ __forceinline__ float box_iou(const AugLds& L, float ix1, float iy1, float ix2, float iy2, float iarea,
                                         int p, float off) {
#pragma clang fp contract(off)
  const float xx1 = smax(ix1, L.x1[p]), yy1 = smax(iy1, L.y1[p]);
  const float xx2 = smin(ix2, L.x2[p]), yy2 = smin(iy2, L.y2[p]);
  const float w = smax(0.f, xx2 - xx1 + off), h = smax(0.f, yy2 - yy1 + off);
  const float inter = w * h;
  return inter / (iarea + box_area(L, p, off) - inter);
}

__device__ __forceinline__ void move_box(const AugLds& L, int from, int to) {
  L.x1[to] = L.x1[from];
  L.y1[to] = L.y1[from];
  L.x2[to] = L.x2[from];
  L.y2[to] = L.y2[from];
  L.sc[to] = L.sc[from];
  L.idx[to] = L.idx[from];
  L.src[to] = L.src[from];
}

// One workgroup per image.  Phases: (1) stage every augmentation's rows into LDS, mapped back to the
// original image (flip, then divide by the scale factor) and filtered by score > score_thr; (2) NMS;
// (3) the first `count` survivors -> fixed-shape outputs (key points gathered and mapped back by `src`).
__global__ __launch_bounds__(1024) void aug_merge_nms_kernel(const pave_aug_plan plan, const float score_thr,
                                                             const int max_num, const int M, const int method,
                                                             const float iou_thr, const float sigma,
                                                             const float min_score, const int offset,
                                                             float* __restrict__ dets, int64_t* __restrict__ labels,
                                                             float* __restrict__ kpts_out,
                                                             int64_t* __restrict__ inds, int32_t* __restrict__ keep,
                                                             int32_t* __restrict__ count_out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int A = plan.n_aug, B = plan.B, N = plan.N, K = plan.K;
  const int total = A * N;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  AugLds L;
  L.x1 = reinterpret_cast<float*>(smem);
  L.y1 = L.x1 + total;
  L.x2 = L.y1 + total;
  L.y2 = L.x2 + total;
  L.sc = L.y2 + total;
  L.idx = reinterpret_cast<int*>(L.sc + total);
  L.src = L.idx + total;
  L.aux0 = L.src + total;
  L.aux1 = L.aux0 + total;
  L.wsum = L.aux1 + total;
  L.rs = reinterpret_cast<float*>(L.wsum + 16);
  L.rp = reinterpret_cast<int*>(L.rs + 16);
  const float off = (float)offset;

  // ---- (1) staging: thread t owns rows [t * cpt, (t + 1) * cpt) of the concatenation (aug-major)
  const int cpt = (total + nt - 1) / nt;
  int kept_c = 0, valid_c = 0;
  int kflag[kMaxPerThread], vflag[kMaxPerThread];
  float bx[kMaxPerThread][5];
#pragma unroll
  for (int c = 0; c < kMaxPerThread; ++c) {
    kflag[c] = vflag[c] = 0;
    const int r = tid * cpt + c;
    if (c >= cpt || r >= total) continue;
    const int a = r / N, j = r - a * N;
    const long long row = (long long)b * N + j;
    kflag[c] = plan.keep[a] ? (plan.keep[a][row] != 0) : 1;
    if (!kflag[c]) continue;
    const float* bb = plan.bboxes[a] + row * 5;
    const int slot = a * B + b;
    const float w = plan.img_w[slot];
    float x1 = bb[0], y1 = bb[1], x2 = bb[2], y2 = bb[3];
    if (plan.flip[a]) {   // bbox_flip: x1' = w - x2, x2' = w - x1
      const float f1 = w - x2, f2 = w - x1;
      x1 = f1;
      x2 = f2;
    }
    const float* sf = plan.scale_factor[slot];
    bx[c][0] = x1 / sf[0];
    bx[c][1] = y1 / sf[1];
    bx[c][2] = x2 / sf[2];
    bx[c][3] = y2 / sf[3];
    bx[c][4] = bb[4];
    vflag[c] = bb[4] > score_thr;   // multiclass_nms: valid_mask = scores > score_thr (strict)
    kept_c += 1;
    valid_c += vflag[c];
  }
  int n_kept, n;
  const int kept_off = block_scan(kept_c, L.wsum, &n_kept);
  const int valid_off = block_scan(valid_c, L.wsum, &n);
  {
    int ko = kept_off, vo = valid_off;
#pragma unroll
    for (int c = 0; c < kMaxPerThread; ++c) {
      if (!kflag[c]) continue;
      if (vflag[c]) {
        L.x1[vo] = bx[c][0];
        L.y1[vo] = bx[c][1];
        L.x2[vo] = bx[c][2];
        L.y2[vo] = bx[c][3];
        L.sc[vo] = bx[c][4];
        L.idx[vo] = ko;
        L.src[vo] = tid * cpt + c;
        ++vo;
      }
      ++ko;
    }
  }
  __syncthreads();

  // ---- (2) NMS over the n valid boxes (positions 0 .. n-1, in concatenation order)
  const int limit = max_num > 0 ? min(max_num, M) : M;   // rows the output keeps
  int count = 0;
  int* outpos = nullptr;   // hard NMS: position of output row r; soft: row r is position r
  if (n > 0 && method == 0) {
    // nms_cpu: descending score order (ties: lower merged index first), suppress ovr > thr
    int* order = L.aux0;
    int* dead = L.aux1;
    for (int p = tid; p < n; p += nt) {
      const float s = L.sc[p];
      int rank = 0;
      for (int q = 0; q < n; ++q) {
        const float t = L.sc[q];
        rank += (t > s) || (t == s && q < p);
      }
      order[rank] = p;
      dead[p] = 0;
    }
    __syncthreads();
    for (int ii = 0; ii < n; ++ii) {
      const int i = order[ii];
      if (dead[i]) continue;   // uniform: LDS read after the last barrier
      __syncthreads();         // every thread has read order[.. ii]: slot `count` (<= ii) is free
      if (tid == 0) order[count] = i;   // the kept positions, in order, overwrite the consumed prefix
      if (++count == limit) break;
      const float ix1 = L.x1[i], iy1 = L.y1[i], ix2 = L.x2[i], iy2 = L.y2[i];
      const float iarea = box_area(L, i, off);
      for (int jj = ii + 1 + tid; jj < n; jj += nt) {
        const int j = order[jj];
        if (dead[j]) continue;
        if (box_iou(L, ix1, iy1, ix2, iy2, iarea, j, off) > iou_thr) dead[j] = 1;
      }
      __syncthreads();
    }
    __syncthreads();
    outpos = order;
  } else if (n > 0) {
    // softnms_cpu: argmax of [i, n) in the current arrangement (first occurrence), swap to i, weight every later
    // box once, and drop the ones below min_score by swapping in the last box -- equivalently: holes in
    // [i+1, i+1+S) are filled, in ascending order, by the survivors beyond, taken from the back.
    int ncur = n;
    int i = 0;
    for (; i < ncur && i < limit; ++i) {
      // argmax
      float best = -INFINITY;
      int bp = 0x7fffffff;
      for (int p = i + tid; p < ncur; p += nt) {
        const float s = L.sc[p];
        if (s > best || (s == best && p < bp)) {
          best = s;
          bp = p;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float s2 = __shfl_xor(best, o, 64);
        const int p2 = __shfl_xor(bp, o, 64);
        if (s2 > best || (s2 == best && p2 < bp)) {
          best = s2;
          bp = p2;
        }
      }
      if ((tid & 63) == 0) {
        L.rs[tid >> 6] = best;
        L.rp[tid >> 6] = bp;
      }
      __syncthreads();
      if (tid == 0) {
        float bs = L.rs[0];
        int bpos = L.rp[0];
        for (int w = 1; w < (nt + 63) / 64; ++w) {
          const float s2 = L.rs[w];
          const int p2 = L.rp[w];
          if (s2 > bs || (s2 == bs && p2 < bpos)) {
            bs = s2;
            bpos = p2;
          }
        }
        const float si = L.sc[i];
        if (si != si || bpos == 0x7fffffff) bpos = i;   // a NaN at i is never beaten (max_score < sc[pos])
        if (bpos != i) {
          // swap boxes bpos <-> i
          const float t1 = L.x1[i], t2 = L.y1[i], t3 = L.x2[i], t4 = L.y2[i], t5 = L.sc[i];
          const int t6 = L.idx[i], t7 = L.src[i];
          move_box(L, bpos, i);
          L.x1[bpos] = t1;
          L.y1[bpos] = t2;
          L.x2[bpos] = t3;
          L.y2[bpos] = t4;
          L.sc[bpos] = t5;
          L.idx[bpos] = t6;
          L.src[bpos] = t7;
        }
      }
      __syncthreads();
      // weight every box of (i, ncur): thread t owns the contiguous run [i+1 + t*cpt2, ...)
      const float ix1 = L.x1[i], iy1 = L.y1[i], ix2 = L.x2[i], iy2 = L.y2[i];
      const float iarea = box_area(L, i, off);
      const int len = ncur - i - 1;
      const int cpt2 = (len + nt - 1) / nt;
      int alive[kMaxPerThread];
      int ac = 0;
#pragma unroll
      for (int c = 0; c < kMaxPerThread; ++c) {
        alive[c] = 0;
        const int p = i + 1 + tid * cpt2 + c;
        if (c >= cpt2 || p >= ncur) continue;
        const float ovr = box_iou(L, ix1, iy1, ix2, iy2, iarea, p, off);
        float weight = 1.f;
        if (method == 1) {
          if (ovr >= iou_thr) weight = 0.f;
        } else if (method == 2) {
          if (ovr >= iou_thr) weight = 1.f - ovr;
        } else {
          weight = expf(-(ovr * ovr) / sigma);
        }
        const float s = L.sc[p] * weight;
        L.sc[p] = s;
        alive[c] = !(s < min_score);
        ac += alive[c];
      }
      int S;
      const int aoff = block_scan(ac, L.wsum, &S);   // (the scan's barriers order the score writes too)
      const int head_end = i + 1 + S;
      // survivors beyond the head, by back rank (alive boxes in (p, ncur))
      {
        int a_before = aoff;   // alive boxes in [i+1, p)
#pragma unroll
        for (int c = 0; c < kMaxPerThread; ++c) {
          const int p = i + 1 + tid * cpt2 + c;
          if (c >= cpt2 || p >= ncur) continue;
          if (p >= head_end && alive[c]) L.aux1[S - 1 - a_before] = p;
          a_before += alive[c];
        }
      }
      __syncthreads();
      // the hole of rank h (dead boxes in [i+1, p)) receives the survivor of back rank h
      {
        int a_before = aoff;
#pragma unroll
        for (int c = 0; c < kMaxPerThread; ++c) {
          const int p = i + 1 + tid * cpt2 + c;
          if (c >= cpt2 || p >= ncur) continue;
          if (p < head_end && !alive[c]) move_box(L, L.aux1[(p - i - 1) - a_before], p);
          a_before += alive[c];
        }
      }
      __syncthreads();
      ncur = head_end;
    }
    count = i;   // rows 0 .. i-1 are final (output order = selection order)
  }

  // ---- (3) outputs: rows [0, count) from LDS, the rest zeroed (keep = 0, inds = -1)
  for (int r = tid; r < M; r += nt) {
    const long long o = (long long)b * M + r;
    if (r < count) {
      const int p = outpos ? outpos[r] : r;
      dets[o * 5 + 0] = L.x1[p];
      dets[o * 5 + 1] = L.y1[p];
      dets[o * 5 + 2] = L.x2[p];
      dets[o * 5 + 3] = L.y2[p];
      dets[o * 5 + 4] = L.sc[p];
      inds[o] = L.idx[p];
      keep[o] = 1;
    } else {
      for (int k = 0; k < 5; ++k) dets[o * 5 + k] = 0.f;
      inds[o] = -1;
      keep[o] = 0;
    }
    labels[o] = 0;   // one class: multiclass_nms labels are 0
  }
  // key points of the output rows: kpt_flip (x' = w - x, then the left/right swap) and / scale_factor[:2]
  for (int t = tid; t < M * K; t += nt) {
    const int r = t / K, k = t - r * K;
    const long long o = ((long long)b * M + r) * K + k;
    if (r < count) {
      const int p = outpos ? outpos[r] : r;
      const int s = L.src[p];
      const int a = s / N, j = s - a * N;
      const int slot = a * B + b;
      const int ks = plan.flip[a] ? plan.flip_perm[k] : k;
      const float* kp = plan.kpts[a] + (((long long)b * N + j) * K + ks) * 3;
      float x = kp[0];
      const float y = kp[1];
      if (plan.flip[a]) x = plan.img_w[slot] - x;
      kpts_out[o * 3 + 0] = x / plan.scale_factor[slot][0];
      kpts_out[o * 3 + 1] = y / plan.scale_factor[slot][1];
      kpts_out[o * 3 + 2] = 1.f;   // aug_test: a score channel of ones
    } else {
      kpts_out[o * 3 + 0] = 0.f;
      kpts_out[o * 3 + 1] = 0.f;
      kpts_out[o * 3 + 2] = 0.f;
    }
  }
  if (tid == 0) count_out[b] = count;
}

// [n, C, Hp, Wp]: columns [0, w_n) mirrored within themselves, the padding columns copied as they are.
__global__ __launch_bounds__(256) void hflip_canvas_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const int32_t* __restrict__ valid_w, const int valid_w_all,
                                                           const int C, const int Hp, const int Wp,
                                                           const long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(i % Wp);
    const long long rowbase = i - col;
    const int img = (int)(i / ((long long)C * Hp * Wp));
    int w = valid_w ? valid_w[img] : valid_w_all;
    w = w < 0 ? 0 : (w > Wp ? Wp : w);
    const int sc = col < w ? w - 1 - col : col;
    y[i] = x[rowbase + sc];
  }
}

}  // namespace

extern "C" {

int pave_aug_merge_nms_f32(const pave_aug_plan* plan, float score_thr, int max_num, int method, float iou_thr,
                           float sigma, float min_score, int offset, float* dets, int64_t* labels, float* kpts,
                           int64_t* inds, int32_t* keep, int32_t* count, void* stream) {
  if (!plan || !dets || !labels || !kpts || !inds || !keep || !count)
    return pave_internal_fail(PAVE_E_ARG, "aug_merge_nms: null pointer");
  const int A = plan->n_aug, B = plan->B, N = plan->N, K = plan->K;
  if (A <= 0 || B <= 0 || N <= 0 || K <= 0) return pave_internal_fail(PAVE_E_ARG, "aug_merge_nms: sizes must be positive");
  if (A > PAVE_AUG_MAX_AUGS || A * B > PAVE_AUG_MAX_SLOTS || K > PAVE_AUG_MAX_K)
    return pave_internal_fail(PAVE_E_UNSUPPORTED, "aug_merge_nms: at most 16 augmentations, 128 (augmentation, "
                                                  "image) pairs and 64 key points");
  if (A * N > kMaxBoxes)
    return pave_internal_fail(PAVE_E_UNSUPPORTED, "aug_merge_nms: at most 4096 boxes (augmentations x rows) per "
                                                  "image: they are kept in LDS");
  if (method < 0 || method > 3) return pave_internal_fail(PAVE_E_ARG, "aug_merge_nms: method 0..3");
  if (offset != 0 && offset != 1) return pave_internal_fail(PAVE_E_ARG, "aug_merge_nms: offset 0 or 1");
  for (int a = 0; a < A; ++a)
    if (!plan->bboxes[a] || !plan->kpts[a]) return pave_internal_fail(PAVE_E_ARG, "aug_merge_nms: null input");
  for (int k = 0; k < K; ++k)
    if (plan->flip_perm[k] < 0 || plan->flip_perm[k] >= K)
      return pave_internal_fail(PAVE_E_ARG, "aug_merge_nms: flip_perm entries must lie in [0, K)");
  const int total = A * N;
  const int M = (max_num > 0 && max_num < total) ? max_num : total;
  int threads = ((total + kMaxPerThread - 1) / kMaxPerThread + 63) / 64 * 64;
  threads = threads < 64 ? 64 : (threads > 1024 ? 1024 : threads);
  const size_t smem = (size_t)total * 9 * 4 + 16 * 4 * 3;
  return pave_launch_lds<aug_merge_nms_kernel>(
      "aug_merge_nms: cannot raise the dynamic LDS limit", dim3((unsigned)B), dim3(threads), smem,
      reinterpret_cast<hipStream_t>(stream), *plan, score_thr, max_num, M, method, iou_thr, sigma, min_score, offset,
      dets, labels, kpts, inds, keep, count);
}

int pave_hflip_canvas_f32(const float* x, float* y, const int32_t* valid_w, int valid_w_all, int n, int C, int Hp,
                          int Wp, void* stream) {
  if (!x || !y) return pave_internal_fail(PAVE_E_ARG, "hflip_canvas: null pointer");
  if (x == y) return pave_internal_fail(PAVE_E_ARG, "hflip_canvas: out of place only");
  if (n <= 0 || C <= 0 || Hp <= 0 || Wp <= 0) return pave_internal_fail(PAVE_E_ARG, "hflip_canvas: bad sizes");
  const long long total = (long long)n * C * Hp * Wp;
  long long nb = (total + 255) / 256;
  if (nb > 256 * 32) nb = 256 * 32;
  return pave_launch<hflip_canvas_kernel>(
      dim3((unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, valid_w, valid_w_all, C, Hp, Wp,
      total);
}

}  // extern "C"
