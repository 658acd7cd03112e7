/* Shared between the translation units of libpave_hip.so (not part of the C ABI).  Include after
   <hip/hip_runtime.h> and pave_hip.h. */
#ifndef PAVE_INTERNAL_H_
#define PAVE_INTERNAL_H_
#include <type_traits>

int pave_internal_fail(int code, const char* msg); /* records pave_last_error(), returns code */

// ---- the one launch path of the host code ----
// pave_launch: launch KERN, read the runtime's last error, return PAVE_OK or PAVE_E_LAUNCH with its message.
// pave_launch_lds: the same for a kernel whose dynamic LDS needs the function attribute raised -- done when
// `smem` exceeds what THIS instantiation (= this kernel) was raised to before; `refusal` is the message if the
// runtime declines.  The marks are per process and unsynchronised, as the once-flags they replace: two threads
// making a kernel's first launch at once both set the attribute to the same value.
template <auto KERN, class... A>
inline int pave_launch(dim3 grid, dim3 block, int smem, hipStream_t st, A... args) {
  hipLaunchKernelGGL(KERN, grid, block, smem, st, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pave_internal_fail(PAVE_E_LAUNCH, hipGetErrorString(e));
  return PAVE_OK;
}
template <auto KERN, class... A>
inline int pave_launch_lds(const char* refusal, dim3 grid, dim3 block, int smem, hipStream_t st, A... args) {
  static int raised = 0;
  if (smem > raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                            smem) != hipSuccess)
      return pave_internal_fail(PAVE_E_LAUNCH, refusal);
    raised = smem;
  }
  return pave_launch<KERN>(grid, block, smem, st, args...);
}

/* Kernel-form overrides for A/B runs and the form-equality tests (native.diag_build(v) passes the integer).
   Only the -DPAVE_DIAG build (lib/libpave_hip_diag.so, loaded by tests/ and tools/ through native.diag_build())
   has the process-global and its setter pave_diag_gemm_variant(); in the shipped library the form selection is
   a compile-time constant. */
enum PaveDiag : int {
  PAVE_DV_NONE = 0,
  PAVE_DV_TILE256 = 2,          // first generation: the 256-row tile forms
  PAVE_DV_W8_ALWAYS = 3,        // first generation: 128 x 256 / 8-wave tiles wherever N % 256 == 0 ...
  PAVE_DV_W8_NEVER = 4,         // ... never (what the shipped selection does)
  PAVE_DV_CONV3_ADDR64 = 5,     // 3x3 form with 64-bit lane addresses (not buffer-addressed)
  PAVE_DV_NO_SPLITK = 6,        // no split-K plan
  PAVE_DV_WIDE_ALWAYS = 7,      // wide tile form wherever it applies (default: from 512 tiles up)
  PAVE_DV_WIDE_NEVER = 8,       // LDS-DMA generation without its wide tile form
  PAVE_DV_FIRST_GEN = 9,        // first-generation kernels for every 3-plane form (A/B against the LDS-DMA
                                // generation of pave_gemm_dma.hip, the default)
  PAVE_DV_LN_8WAVE = 13,        // LayerNorm-epilogue GEMM: always the 8-wave form ...
  PAVE_DV_LN_WIDE = 14,         // ... always the wide form
  PAVE_DV_RM2_NEVER = 15,       // two row tiles per wave (256-row blocks) for the 64- / 96-column tile forms and
  PAVE_DV_RM2_ALWAYS = 16,      // the ResNet layer1 chain: never / wherever the form exists
  PAVE_DV_NO_HALF_TAIL = 17,    // no half-tail form (33 .. 48 output columns of a 3x3 as zero-padded 32x32x16
                                // products instead of 16x16x32 products over slab pairs)
  PAVE_DV_SWIN_PER_LANE = 18,   // Swin window attention on the per-lane (LDS broadcast) form instead of the
                                // fp32-MFMA form (pave_decoder.hip)
  PAVE_DV_SMALL_ROWS_R5 = 19,   // the small-row selection of rounds 4 - 5 (no K-split small-row form: the forms
                                // the bit-equality tests compare)
  PAVE_DV_WIDE_ONE_PER_CU = 20, // the wide GEMM capped at one block per CU (40 KiB of unused dynamic LDS;
                                // tools/coresidency_probe.py)
  PAVE_DV_SK_ANY_ROWS = 21,     // form policy 2 keeps gemm_sk_kernel above 2 048 rows (no multi-tile K-split
                                // form: the bit-equality test)
};
#ifdef PAVE_DIAG
int pave_internal_diag_variant();
#else
static inline int pave_internal_diag_variant() { return PAVE_DV_NONE; }
#endif

// nplanes of the C ABI -> the LDS-DMA generation's operand planes (3 | 1 = fp16), 0 = not one of its modes
static inline int q_planes(int nplanes) { return nplanes == 3 ? 3 : (nplanes == PAVE_PLANES_FP16 ? 1 : 0); }
// The run-time planes (3 = the exact bf16 split, 1 = one plane of fp16 operands) as a template argument:
// f(std::integral_constant<int, PL>), or the refusal.
template <class F>
inline int pave_with_planes(int planes, const char* refusal, F f) {
  if (planes == 1) return f(std::integral_constant<int, 1>{});
  if (planes != 3) return pave_internal_fail(PAVE_E_ARG, refusal);
  return f(std::integral_constant<int, 3>{});
}

// pave_gemm_dma.hip: the LDS-DMA generation of the 3-plane split GEMM.  Where the A rows come from:
enum GemmQRows : int {   // (the values are the kernels' KIND; 2, the 3x3 with 64-bit addresses, is the dispatcher's)
  GEMMQ_ROWS = 0,        // a [M, lda] (lda 0: K), optionally in column groups of group_n
  GEMMQ_CONV3X3 = 1,     // 3x3 / pad 1 windows of the NHWC map a [.., H, W, Cin], K = 9 Cin padded to 32
  GEMMQ_CONV1X1S = 3,    // the strided pixels of that map, K = Cin
  GEMMQ_ROWS2 = 4,       // columns [0, k1) from a [M, k1], the rest from a2 [M, K - k1]
};
struct GemmQ {
  GemmQRows rows = GEMMQ_ROWS;
  const float* a = nullptr;
  const float* a2 = nullptr;        // GEMMQ_ROWS2
  const float* a_bias = nullptr;    // [K] added to every A row (GEMMQ_ROWS)
  const void* w_planes = nullptr;
  const float* bias = nullptr;
  const float* residual = nullptr;
  long long residual_rows = 0;      // < M: the residual is row-periodic
  float* out = nullptr;
  float* out2 = nullptr;            // columns from n_split on go here
  int n_split = 0;
  long long M = 0;
  int K = 0, N = 0;                 // as padded in the weight planes
  int n_real = 0;                   // columns of out / bias / residual (0: N)
  int relu = 0;                     // 0 none, 1 ReLU, 2 GELU, 3 sigmoid
  int lda = 0, group_n = 0;         // GEMMQ_ROWS
  bool narrow_groups = false;       // ... with 64-column group tiles
  int H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, stride = 0;   // the two convolution forms
  int k1 = 0;                       // GEMMQ_ROWS2
  int ksplit = 1, ks_slabs = 0;     // split-K: parts (raw partial sums into out) and slabs per part
  int planes = 3;                   // 3 = the exact bf16 split, 1 = one plane of fp16 operands
  void* stream = nullptr;
};
int pave_internal_gemm_q(const GemmQ& q);
// split-K (few output rows, long K): plan, and the ordered sum of the parts + bias / residual / ReLU
void pave_internal_splitk_plan(long long M, int Kp, int Np, int* ksplit, int* ks_slabs);
// the calling thread's form policy (pave_set_form_policy); pave_internal_splitk_plan honours it
int pave_internal_form_policy();
int pave_internal_splitk_reduce(const float* ws, int parts, long long M, int n, const float* bias,
                                const float* residual, int relu, float* out, void* stream);
int pave_internal_gemm_q_ln(const float* a, const void* w_planes, const float* bias, const float* residual,
                            const float* gamma, const float* beta, float eps, float* out, long long M,
                            int K, int N, void* stream, int planes = 3);
int pave_internal_gemm_encproj(const float* a, const void* w_planes, const float* table, long long table_rows,
                               const float* value_bias, const float* ref, const int* levels_hw, float* value,
                               float* samp, long long M, int K, void* stream, int planes = 3);
int pave_internal_gemm_f16act(const void* a, int a_f16, const void* w_plane, const float* bias, const float* residual,
                              const float* gamma, const float* beta, float eps, void* out, int out_f16, long long M,
                              int K, int N, int relu, void* stream);
int pave_internal_stem7x7_q(const float* x, const void* w_stem, const float* bias, float* y, int N,
                            int H, int W, int pitch, int relu, void* stream, int planes = 3);
#endif /* PAVE_INTERNAL_H_ */
