// C ABI over the probe kernels; loaded in-process by dcos_commons_amd.ops (ctypes) with torch
// tensors' device pointers and the current HIP stream. Every entry point validates the shapes
// the kernel's grid assumes before launching and returns a hipError_t (0 = success) or a
// negative code for a rejected shape.
#include "probe_kernels.hip"
#include "f8_kernels.hip"
#include "f4_kernels.hip"
#include "i8_kernels.hip"
#include "f64_kernels.hip"
#include "sp_kernels.hip"
#include "f32_kernels.hip"

#include <climits>
#include <cmath>
#include <initializer_list>
#include <mutex>
#include <type_traits>

#define AMDPROBE_EXPORT extern "C" __attribute__((visibility("default")))

using namespace amdprobe;

enum { ERR_SHAPE = -1, ERR_ALIGN = -2 };

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The preamble of the GEMM-shaped entry points: M, N multiples of `mn`, K a multiple of `kg` and at
// most `kmax`, block scales both or neither, every pointer of `ptrs` 16-byte aligned (null passes).
static int check_args(int M, int N, int K, int mn, int kg, int kmax, const void* sa, const void* sb,
                      std::initializer_list<const void*> ptrs) {
  if (M <= 0 || N <= 0 || K <= 0 || M % mn || N % mn || K % kg || K > kmax) return ERR_SHAPE;
  if ((sa == nullptr) != (sb == nullptr)) return ERR_SHAPE;
  for (const void* p : ptrs)
    if (!aligned16(p)) return ERR_ALIGN;
  return 0;
}

AMDPROBE_EXPORT int amdprobe_version() { return 1; }

// variant: 0 = pick (256x256 glds pipeline when the shape allows, else 128x128),
//          1 = 128x128 register-staged, 2 = 256x256 glds pipeline (M, N % 256 == 0, K % 128 == 0)
AMDPROBE_EXPORT int amdprobe_gemm_bf16_nt_variant(const void* A, const void* Bt, float* C, int M, int N, int K,
                                                  int variant, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return ERR_SHAPE;
  if (!aligned16(A) || !aligned16(Bt) || !aligned16(C)) return ERR_ALIGN;
  const bool big_ok = M % big::BM == 0 && N % big::BN == 0 && K % (2 * big::BK) == 0;
  if (variant == 0) variant = big_ok ? 2 : 1;
  if (variant == 2) {
    if (!big_ok) return ERR_SHAPE;
    const int nwg = (M / big::BM) * (N / big::BN);
    hipLaunchKernelGGL(gemm_bf16_nt_256_kernel, dim3(nwg), dim3(big::THREADS), 0, (hipStream_t)stream,
                       (const __bf16*)A, (const __bf16*)Bt, C, M, N, K);
    return (int)hipGetLastError();
  }
  if (variant != 1 || M % BM || N % BN || K % BK) return ERR_SHAPE;
  const int nwg = (M / BM) * (N / BN);
  hipLaunchKernelGGL(gemm_bf16_nt_kernel, dim3(nwg), dim3(GEMM_THREADS), 0, (hipStream_t)stream,
                     (const __bf16*)A, (const __bf16*)Bt, C, M, N, K);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_gemm_bf16_nt(const void* A, const void* Bt, float* C, int M, int N, int K,
                                          void* stream) {
  return amdprobe_gemm_bf16_nt_variant(A, Bt, C, M, N, K, 0, stream);
}

AMDPROBE_EXPORT int amdprobe_mfma_peak(float* out, int blocks, int iters, float seed, void* stream) {
  if (blocks <= 0 || iters <= 0) return ERR_SHAPE;
  hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, iters, seed);
  return (int)hipGetLastError();
}

// FLOPs issued by one amdprobe_mfma_peak launch (for the caller's TFLOP/s).
AMDPROBE_EXPORT double amdprobe_mfma_peak_flops(int blocks, int iters) {
  const double waves = (double)blocks * 4.0;
  return waves * (double)iters * 4.0 * (32.0 * 32.0 * 16.0 * 2.0);
}

AMDPROBE_EXPORT int amdprobe_hbm_copy(const void* src, void* dst, size_t bytes, int blocks, void* stream) {
  if (bytes == 0 || bytes % 16 || blocks <= 0) return ERR_SHAPE;
  if (!aligned16(src) || !aligned16(dst)) return ERR_ALIGN;
  hipLaunchKernelGGL(hbm_copy_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)src,
                     (uint4*)dst, bytes / 16);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_pattern_write(void* p, size_t bytes, unsigned seed, int blocks, void* stream) {
  if (bytes == 0 || bytes % 16 || blocks <= 0) return ERR_SHAPE;
  if (!aligned16(p)) return ERR_ALIGN;
  hipLaunchKernelGGL(pattern_write_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)p, bytes / 16,
                     (uint32_t)seed);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_pattern_check(const void* p, size_t bytes, unsigned seed, unsigned long long* errors,
                                           int blocks, void* stream) {
  if (bytes == 0 || bytes % 16 || blocks <= 0) return ERR_SHAPE;
  if (!aligned16(p)) return ERR_ALIGN;
  hipLaunchKernelGGL(pattern_check_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)p,
                     bytes / 16, (uint32_t)seed, errors);
  return (int)hipGetLastError();
}

// The four dense checks below add sum((C - ref)^2) to out2[0] and sum(ref^2) to out2[1] (device
// pointer, 2 floats that the caller zeroes), ref being an fp32 (INT8: int32) VALU reference of A Bt^T.
AMDPROBE_EXPORT int amdprobe_gemm_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                        int inject, float* out2, void* stream) {
  if (const int rc = check_args(M, N, K, CHECK_TILE, 8, CHECK_MAX_K, nullptr, nullptr, {A, Bt})) return rc;
  hipLaunchKernelGGL(gemm_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const __bf16*)A, (const __bf16*)Bt, C, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// The hashed operand fill (tests compare it with a host model of the hash). `blocks` 0 sizes the
// grid to the buffer, at most 1024 workgroups. `res`, when not null, is a 32-byte ReadinessResult
// slot and is zeroed.
static int launch_fill_pair(void* p, size_t bytes, unsigned seed, uint32_t and4, uint32_t add4, int blocks, void* res,
                            void* stream) {
  if (bytes == 0 || bytes % 16) return ERR_SHAPE;
  if (!aligned16(p) || !aligned16(res)) return ERR_ALIGN;
  const size_t n16 = bytes / 16;
  if (blocks == 0) blocks = (int)((n16 + 255) / 256 < 1024 ? (n16 + 255) / 256 : 1024);
  hipLaunchKernelGGL(hashed_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)p, n16,
                     (uint32_t)seed, and4, add4, (ReadinessResult*)res);
  return (int)hipGetLastError();
}

static int launch_fill(void* p, size_t bytes, unsigned seed, int kind, int blocks, void* res, void* stream) {
  if (kind < 0 || kind >= FILL_KINDS) return ERR_SHAPE;
  return launch_fill_pair(p, bytes, seed, FILL_AND4[kind], FILL_ADD4[kind], blocks, res, stream);
}

// The fp32 fill: hashed_fill_kernel with the dword pair of f32_kernels.hip, with launch_fill's contract.
static int launch_fill_f32(void* p, size_t bytes, unsigned seed, void* res, void* stream) {
  return launch_fill_pair(p, bytes, seed, FILL_F32_AND, FILL_F32_ADD, 0, res, stream);
}

// The bf16 readiness fill: `ab` gets `ab_bytes` of hashed bf16 and `res` (32 bytes) is zeroed.
AMDPROBE_EXPORT int amdprobe_readiness_fill(void* ab, size_t ab_bytes, unsigned seed, void* res, void* stream) {
  return launch_fill(ab, ab_bytes, seed, FILL_BF16, 64, res, stream);
}

// The fp64 fill (hashed_fill_f64_kernel), with launch_fill's contract.
static int launch_fill_f64(void* p, size_t bytes, unsigned seed, void* res, void* stream) {
  if (bytes == 0 || bytes % 16) return ERR_SHAPE;
  if (!aligned16(p) || !aligned16(res)) return ERR_ALIGN;
  const size_t n16 = bytes / 16;
  const int blocks = (int)((n16 + 255) / 256 < 1024 ? (n16 + 255) / 256 : 1024);
  hipLaunchKernelGGL(hashed_fill_f64_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)p, n16,
                     (uint32_t)seed, (ReadinessResult*)res);
  return (int)hipGetLastError();
}

// The 2:4 metadata fill (hashed_fill_meta24_kernel), with launch_fill's contract.
static int launch_fill_meta24(void* p, size_t bytes, unsigned seed, void* res, void* stream) {
  if (bytes == 0 || bytes % 16) return ERR_SHAPE;
  if (!aligned16(p) || !aligned16(res)) return ERR_ALIGN;
  const size_t n16 = bytes / 16;
  const int blocks = (int)((n16 + 255) / 256 < 1024 ? (n16 + 255) / 256 : 1024);
  hipLaunchKernelGGL(hashed_fill_meta24_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)p, n16,
                     (uint32_t)seed, (ReadinessResult*)res);
  return (int)hipGetLastError();
}

// The FP8 / FP4 readiness fill: kind 0 = E4M3 bytes, 1 = E5M2 bytes, 2 = E8M0 block scales, 3 = packed
// E2M1 nibbles (see hashed_fill_kernel), 5 = fp64 (hashed_fill_f64_kernel), 6 = legal 2:4 metadata nibbles
// (hashed_fill_meta24_kernel), 7 = fp32 (hashed_fill_kernel, sign and 23 mantissa bits hashed, exponent 126). `res`
// may be null; otherwise see launch_fill.
AMDPROBE_EXPORT int amdprobe_f8_fill(void* p, size_t bytes, unsigned seed, int kind, float* res, void* stream) {
  if (kind == FILL_F64) return launch_fill_f64(p, bytes, seed, res, stream);
  if (kind == FILL_META24) return launch_fill_meta24(p, bytes, seed, res, stream);
  if (kind == FILL_F32) return launch_fill_f32(p, bytes, seed, res, stream);
  return kind > FILL_E2M1 ? (int)ERR_SHAPE : launch_fill(p, bytes, seed, kind, 0, res, stream);
}

// ---------------------------------------------------------------------------------------
// FP8 / MXFP8 (f8_kernels.hip). fmt_a / fmt_b: 0 = E4M3, 1 = E5M2 (OCP); the pairs built are
// E4M3 x E4M3, E5M2 x E5M2 and E4M3 x E5M2. sa / sb: E8M0 block scales [M][K/32], [N][K/32], both
// null for an unscaled product.
// ---------------------------------------------------------------------------------------
namespace {
// Calls launch(FA, FB) with the format pair as compile-time constants; ERR_SHAPE for a pair that is not built.
template <typename Launch>
int dispatch_f8(int fmt_a, int fmt_b, Launch&& launch) {
  using E4 = std::integral_constant<int, F8_E4M3>;
  using E5 = std::integral_constant<int, F8_E5M2>;
  if (fmt_a == F8_E4M3 && fmt_b == F8_E4M3) launch(E4{}, E4{});
  else if (fmt_a == F8_E5M2 && fmt_b == F8_E5M2) launch(E5{}, E5{});
  else if (fmt_a == F8_E4M3 && fmt_b == F8_E5M2) launch(E4{}, E5{});
  else return ERR_SHAPE;
  return (int)hipGetLastError();
}
}  // namespace

AMDPROBE_EXPORT int amdprobe_gemm_f8_nt(const void* A, const void* Bt, float* C, int M, int N, int K, int fmt_a,
                                        int fmt_b, const void* sa, const void* sb, void* stream) {
  if (const int rc = check_args(M, N, K, f8::BM, f8::BK, INT_MAX, sa, sb, {A, Bt, C, sa, sb})) return rc;
  const dim3 grid((M / f8::BM) * (N / f8::BN)), block(f8::THREADS);
  const uint8_t *a = (const uint8_t*)A, *b = (const uint8_t*)Bt, *pa = (const uint8_t*)sa, *pb = (const uint8_t*)sb;
  return dispatch_f8(fmt_a, fmt_b, [&](auto fa, auto fb) {
    constexpr int FA = decltype(fa)::value, FB = decltype(fb)::value;
    if (sa != nullptr)
      hipLaunchKernelGGL((gemm_f8_nt_kernel<FA, FB, true>), grid, block, 0, (hipStream_t)stream, a, b, C, pa, pb, M, N, K);
    else
      hipLaunchKernelGGL((gemm_f8_nt_kernel<FA, FB, false>), grid, block, 0, (hipStream_t)stream, a, b, C, pa, pb, M, N, K);
  });
}

AMDPROBE_EXPORT int amdprobe_gemm_f8_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                           int fmt_a, int fmt_b, const void* sa, const void* sb, int inject,
                                           float* out2, void* stream) {
  if (const int rc = check_args(M, N, K, CHECK_TILE, 32, CHECK_MAX_K, sa, sb, {A, Bt})) return rc;
  const dim3 grid((M / CHECK_TILE) * (N / CHECK_TILE)), block(CHECK_THREADS);
  return dispatch_f8(fmt_a, fmt_b, [&](auto fa, auto fb) {
    hipLaunchKernelGGL((gemm_f8_check_kernel<decltype(fa)::value, decltype(fb)::value>), grid, block, 0,
                       (hipStream_t)stream, (const uint8_t*)A, (const uint8_t*)Bt, C, (const uint8_t*)sa,
                       (const uint8_t*)sb, M, N, K, inject, out2);
  });
}

// ---------------------------------------------------------------------------------------
// FP4 / MXFP4 (f4_kernels.hip). A, Bt: packed E2M1, K/2 bytes per row. sa / sb: E8M0 block scales
// [M][K/32], [N][K/32], both null for an unscaled product.
// ---------------------------------------------------------------------------------------
AMDPROBE_EXPORT int amdprobe_gemm_f4_nt(const void* A, const void* Bt, float* C, int M, int N, int K, const void* sa,
                                        const void* sb, void* stream) {
  if (const int rc = check_args(M, N, K, f4::BM, f4::BK, INT_MAX, sa, sb, {A, Bt, C, sa, sb})) return rc;
  const dim3 grid((M / f4::BM) * (N / f4::BN)), block(f4::THREADS);
  const uint8_t *a = (const uint8_t*)A, *b = (const uint8_t*)Bt, *pa = (const uint8_t*)sa, *pb = (const uint8_t*)sb;
  if (sa != nullptr)
    hipLaunchKernelGGL(gemm_f4_nt_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, C, pa, pb, M, N, K);
  else
    hipLaunchKernelGGL(gemm_f4_nt_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, C, pa, pb, M, N, K);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_gemm_f4_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                           const void* sa, const void* sb, int inject, float* out2, void* stream) {
  if (const int rc = check_args(M, N, K, CHECK_TILE, 32, CHECK_MAX_K, sa, sb, {A, Bt})) return rc;
  hipLaunchKernelGGL(gemm_f4_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)A, (const uint8_t*)Bt, C, (const uint8_t*)sa,
                     (const uint8_t*)sb, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// INT8 (i8_kernels.hip). A, Bt: int8, K bytes per row; C: int32. K <= 65536 keeps every sum below 2^31.
// ---------------------------------------------------------------------------------------
AMDPROBE_EXPORT int amdprobe_gemm_i8_nt(const void* A, const void* Bt, int* C, int M, int N, int K, void* stream) {
  if (const int rc = check_args(M, N, K, i8::BM, i8::BK, i8::MAX_K, nullptr, nullptr, {A, Bt, C})) return rc;
  hipLaunchKernelGGL(gemm_i8_nt_kernel, dim3((M / i8::BM) * (N / i8::BN)), dim3(i8::THREADS), 0, (hipStream_t)stream,
                     (const int8_t*)A, (const int8_t*)Bt, C, M, N, K);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_gemm_i8_check(const void* A, const void* Bt, const int* C, int M, int N, int K,
                                           int inject, float* out2, void* stream) {
  if (const int rc = check_args(M, N, K, CHECK_TILE, 16, CHECK_MAX_K, nullptr, nullptr, {A, Bt})) return rc;
  hipLaunchKernelGGL(gemm_i8_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const int8_t*)A, (const int8_t*)Bt, C, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// FP64 (f64_kernels.hip). A, Bt: doubles, 8 * K bytes per row; C: fp64. M % 256, N % 128, K % 16.
// ---------------------------------------------------------------------------------------
AMDPROBE_EXPORT int amdprobe_gemm_f64_nt(const void* A, const void* Bt, double* C, int M, int N, int K, void* stream) {
  if (const int rc = check_args(M, N, K, f64::BN, f64::BK, INT_MAX, nullptr, nullptr, {A, Bt, C})) return rc;
  if (M % f64::BM) return ERR_SHAPE;
  hipLaunchKernelGGL(gemm_f64_nt_kernel, dim3((M / f64::BM) * (N / f64::BN)), dim3(f64::THREADS), 0,
                     (hipStream_t)stream, (const double*)A, (const double*)Bt, C, M, N, K);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_gemm_f64_check(const void* A, const void* Bt, const double* C, int M, int N, int K,
                                            int inject, float* out2, void* stream) {
  if (const int rc = check_args(M, N, K, CHECK_TILE, 4, f64::CHECK_MAX_K, nullptr, nullptr, {A, Bt})) return rc;
  hipLaunchKernelGGL(gemm_f64_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const double*)A, (const double*)Bt, C, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// 2:4 sparse bf16 (sp_kernels.hip). vals: bf16 [M][K/2], meta: uint8 [M][K/8], Bt: bf16 [N][K]; C: fp32.
// M % 256, N % 128, K % 128. The metadata nibbles are not validated (see sp24_expand_kernel).
// ---------------------------------------------------------------------------------------
AMDPROBE_EXPORT int amdprobe_gemm_sp_bf16_nt(const void* vals, const void* meta, const void* Bt, float* C, int M,
                                             int N, int K, void* stream) {
  if (const int rc = check_args(M, N, K, sp::BN, sp::BK, INT_MAX, nullptr, nullptr, {vals, meta, Bt, C})) return rc;
  if (M % sp::BM) return ERR_SHAPE;
  hipLaunchKernelGGL(gemm_sp_bf16_nt_kernel, dim3((M / sp::BM) * (N / sp::BN)), dim3(sp::THREADS), 0,
                     (hipStream_t)stream, (const __bf16*)vals, (const uint8_t*)meta, (const __bf16*)Bt, C, M, N, K);
  return (int)hipGetLastError();
}

// The dense bf16 A[M][K] of a compressed (vals, meta) pair. K % 8 == 0.
AMDPROBE_EXPORT int amdprobe_sp24_expand(const void* vals, const void* meta, void* A, int M, int K, void* stream) {
  if (M <= 0 || K <= 0 || K % 8) return ERR_SHAPE;
  if (!aligned16(vals) || !aligned16(A)) return ERR_ALIGN;
  const size_t n = (size_t)M * (K / 8);
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(sp24_expand_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint2*)vals,
                     (const uint8_t*)meta, (uint4*)A, n);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// FP32 (f32_kernels.hip). A, Bt: floats, 4 * K bytes per row; C: fp32. M, N % 256, K % 32.
// ---------------------------------------------------------------------------------------
AMDPROBE_EXPORT int amdprobe_gemm_f32_nt(const void* A, const void* Bt, float* C, int M, int N, int K, void* stream) {
  static_assert(f32::BM == f32::BN, "one M, N granule");
  if (const int rc = check_args(M, N, K, f32::BM, f32::BK, INT_MAX, nullptr, nullptr, {A, Bt, C})) return rc;
  hipLaunchKernelGGL(gemm_f32_nt_kernel, dim3((M / f32::BM) * (N / f32::BN)), dim3(f32::THREADS), 0,
                     (hipStream_t)stream, (const float*)A, (const float*)Bt, C, M, N, K);
  return (int)hipGetLastError();
}

AMDPROBE_EXPORT int amdprobe_gemm_f32_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                            int inject, float* out2, void* stream) {
  if (const int rc = check_args(M, N, K, CHECK_TILE, 8, f32::CHECK_MAX_K, nullptr, nullptr, {A, Bt})) return rc;
  hipLaunchKernelGGL(gemm_f32_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const float*)A, (const float*)Bt, C, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The readiness checks: the whole check of one device in one call (see probe_kernels.hip). Buffers, a
// non-blocking stream and a pinned result slot are created on first use per device and reused; calls
// for one device serialize on its context, and the bf16 and f8 / f4 paths have contexts of their own
// and so have fp64 and sparse24
// (they neither wait for each other nor allocate each other's buffers). The calling thread's current
// device is restored. Returns 0 or a HIP error / negative shape code.
//
// The buffers outlive the call, so a kernel that dropped its writes would leave the previous call's
// correct data behind. Two things stop that from passing: C is poisoned with 0xFF bytes (NaN; -1 as
// int32) before the GEMM, and every call mixes a per-device call counter into the seed, so the operands and the pattern
// differ from the last call's and stale data cannot match.
// ---------------------------------------------------------------------------------------
namespace {
constexpr int RM = 256, RN = 256, RK = 512;
constexpr size_t PATTERN_BYTES = size_t(64) << 20;
constexpr int MAX_DEVICES = 64;
constexpr size_t C_BYTES = size_t(RM) * RN * sizeof(float);

enum { BUF_AB = 0, BUF_C = 1, BUF_AUX = 2, PROBE_BUFS = 3 };   // aux: the HBM pattern (bf16) or the block scales
struct ProbeCtx {
  std::mutex mu;
  bool ready = false;
  hipStream_t stream = nullptr;
  void* buf[PROBE_BUFS] = {};       // A (RM rows) then Bt (RN rows); C (RM x RN fp32); aux
  ReadinessResult* res = nullptr;
  ReadinessResult* host = nullptr;  // pinned
  uint32_t calls = 0;               // mixed into the seed: no two calls share operands or pattern
};
ProbeCtx g_readiness[MAX_DEVICES], g_readiness_f8[MAX_DEVICES], g_readiness_f64[MAX_DEVICES],
    g_readiness_sp[MAX_DEVICES];
constexpr size_t BF16_BYTES[PROBE_BUFS] = {size_t(RM + RN) * RK * sizeof(__bf16), C_BYTES, PATTERN_BYTES};
constexpr size_t F8_BYTES[PROBE_BUFS] = {size_t(RM + RN) * RK, C_BYTES, size_t(RM + RN) * (RK / 32)};
// fp64: K = 128 is 8 K-tiles of 16, so the three-stage ring of gemm_f64_nt_kernel reaches its steady state
// (it needs ring depth + 2 = 5), and the 256 x 256 product is two of its 256 x 128 workgroups. No aux buffer is
// used; the slot gets 16 bytes.
constexpr int RK64 = 128;
constexpr size_t F64_BYTES[PROBE_BUFS] = {size_t(RM + RN) * RK64 * sizeof(double), size_t(RM) * RN * sizeof(double), 16};
// sparse24: K = 512 is SP_RING + 2 = 4 K-tiles of 128 = 8 half-stages of gemm_sp_bf16_nt_kernel's ring of four:
// every ring slot gets a second occupant, the counted vmcnt(9) waits of the steady state run (they need a K-tile
// T + 2) and so do the shorter ones of the last two K-tiles. It is the smallest K that does all three, and below
// the dense check's CHECK_MAX_K. BUF_AB holds the expanded A, then Bt, then vals (Bt and vals are filled as
// one run of hashed bf16); the aux buffer is the metadata. The 256 x 256 product is two 256 x 128 workgroups.
constexpr int RKSP = 512;
// fp32: K = (f32::RING + 2) * f32::BK = 128 is 4 K-tiles on gemm_f32_nt_kernel's ring of two: every ring slot gets
// a second occupant, and the prologue's counted wait, the loop's barrier with and without a stage after it and the
// barrier-free last tile all run. The product is one 256 x 256 workgroup. Operands and product are exactly the
// sizes of the f8 context's buffers, so the mode runs there, as int8 does.
constexpr int RK32 = (f32::RING + 2) * f32::BK;
constexpr size_t SP_A_BYTES = size_t(RM) * RKSP * sizeof(__bf16), SP_BT_BYTES = size_t(RN) * RKSP * sizeof(__bf16);
constexpr size_t SP_BYTES[PROBE_BUFS] = {SP_A_BYTES + SP_BT_BYTES + SP_A_BYTES / 2, C_BYTES, size_t(RM) * (RKSP / 8)};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Returns a failed step's code: a hipError_t, or the int of an entry point of this file (0 = success for both).
#define PROBE_TRY(expr)                                  \
  do {                                                   \
    const int e_ = (int)(expr);                          \
    if (e_ != 0) return e_;                              \
  } while (0)

void probe_release(ProbeCtx& ctx) {
  if (ctx.stream != nullptr) (void)hipStreamDestroy(ctx.stream);
  for (void*& p : ctx.buf) {
    if (p != nullptr) (void)hipFree(p);
    p = nullptr;
  }
  if (ctx.res != nullptr) (void)hipFree(ctx.res);
  if (ctx.host != nullptr) (void)hipHostFree(ctx.host);
  ctx.stream = nullptr;
  ctx.res = ctx.host = nullptr;
}

int probe_alloc(ProbeCtx& ctx, const size_t (&bytes)[PROBE_BUFS]) {
  PROBE_TRY(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
  for (int i = 0; i < PROBE_BUFS; ++i) PROBE_TRY(hipMalloc(&ctx.buf[i], bytes[i]));
  PROBE_TRY(hipMalloc((void**)&ctx.res, sizeof(ReadinessResult)));
  PROBE_TRY(hipHostMalloc((void**)&ctx.host, sizeof(ReadinessResult), hipHostMallocDefault));
  return 0;
}

// One readiness call on `device`'s context of `table`. Enter: validate the device, take the context's
// lock for the whole call, make the device current, allocate on first use (the context then lives for
// the process; a failed allocation releases whatever it got, so the next call starts clean instead of
// leaking). Then `launches(ctx, call_seed)` enqueues the work on ctx.stream. Finish: one read-back of
// the result slot; rel_err = sqrt(diff2 / ref2), or HUGE_VAL when that is not a number a pass could
// have produced (NaN C, never written, fails).
template <typename Launches>
int run_probe(ProbeCtx* table, const size_t (&bytes)[PROBE_BUFS], int device, unsigned seed, double* rel_err,
              unsigned long long* bad_words, Launches&& launches) {
  if (rel_err == nullptr || device < 0 || device >= MAX_DEVICES) return ERR_SHAPE;
  int ndev = 0;
  PROBE_TRY(hipGetDeviceCount(&ndev));
  if (device >= ndev) return ERR_SHAPE;
  ProbeCtx& ctx = table[device];
  std::lock_guard<std::mutex> lock(ctx.mu);
  DeviceGuard guard(device);
  if (!ctx.ready) {
    if (const int rc = probe_alloc(ctx, bytes)) {
      probe_release(ctx);
      return rc;
    }
    ctx.ready = true;
  }
  if (const int rc = launches(ctx, (uint32_t)seed ^ (0x9E3779B9u * ++ctx.calls))) return rc;
  PROBE_TRY(hipMemcpyAsync(ctx.host, ctx.res, sizeof(ReadinessResult), hipMemcpyDeviceToHost, ctx.stream));
  PROBE_TRY(hipStreamSynchronize(ctx.stream));
  const double d2 = ctx.host->diff2, w2 = ctx.host->ref2;
  *rel_err = (w2 > 0.0 && std::isfinite(d2)) ? std::sqrt(d2 / w2) : HUGE_VAL;
  if (bad_words != nullptr) *bad_words = ctx.host->bad_words;
  return 0;
}
}  // namespace

// bf16 MFMA GEMM with its dense check, then the HBM pattern test: five launches and one 32-byte
// read-back. inject: 0 = none, 1 = lose one 16x16 tile of the product (the check must fail), 2 = corrupt
// one pattern word (the memory check must count it), 3 = skip the GEMM launch, 4 = skip the pattern
// write (both model a kernel that silently drops its writes; the check must still fail).
AMDPROBE_EXPORT int amdprobe_readiness(int device, unsigned seed, int inject, double* rel_err,
                                       unsigned long long* bad_words) {
  if (bad_words == nullptr) return ERR_SHAPE;
  return run_probe(g_readiness, BF16_BYTES, device, seed, rel_err, bad_words, [&](ProbeCtx& ctx, uint32_t call_seed) {
    hipStream_t s = ctx.stream;
    const __bf16* A = (const __bf16*)ctx.buf[BUF_AB];
    const __bf16* Bt = A + size_t(RM) * RK;
    float* C = (float*)ctx.buf[BUF_C];
    void* pattern = ctx.buf[BUF_AUX];
    PROBE_TRY(amdprobe_readiness_fill(ctx.buf[BUF_AB], BF16_BYTES[BUF_AB], call_seed, ctx.res, s));
    PROBE_TRY(hipMemsetAsync(C, 0xFF, C_BYTES, s));  // NaN until the GEMM writes
    // 128x128 tiles: four workgroups for the 256x256 product (one 256x256-tile workgroup takes ~15 us)
    if (inject != 3) PROBE_TRY(amdprobe_gemm_bf16_nt_variant(A, Bt, C, RM, RN, RK, 1, s));
    PROBE_TRY(amdprobe_gemm_check(A, Bt, C, RM, RN, RK, inject == 1 ? 1 : 0, &ctx.res->diff2, s));
    if (inject != 4) PROBE_TRY(amdprobe_pattern_write(pattern, PATTERN_BYTES, call_seed, 2048, s));
    if (inject == 2) PROBE_TRY(hipMemsetAsync(pattern, 0, 4, s));
    PROBE_TRY(amdprobe_pattern_check(pattern, PATTERN_BYTES, call_seed, &ctx.res->bad_words, 2048, s));
    return 0;
  });
}

// The FP8 / FP4 matrix path: mode 0 = fp8 (E4M3), 1 = bf8 (E5M2), 2 = mxfp8 (E4M3 with E8M0 block
// scales through the MFMA scale inputs), 3 = mxfp4 (packed E2M1 with block scales: the f4 GEMM and
// check on the same buffers, half filled), 4 = int8 (the i8 GEMM and its exact check on the same
// buffers: any byte is an int8, C is int32 and a healthy product gives rel_err == 0). Hashed operands (and scales), the GEMM, the dense VALU
// check, one read-back. inject: 0 = none, 1 = lose one 16x16 tile of the product, 3 = skip the GEMM
// launch (both must fail). There is no HBM pattern here: amdprobe_readiness does that.
// Mode 5 = fp64 runs on a context and buffers of its own (8-byte operands and product do not fit F8_BYTES):
// hashed doubles, C poisoned with 0xFF bytes (a double NaN), the f64 GEMM, its fp64 check, one read-back.
// Mode 6 = sparse24, also on a context of its own: hashed bf16 vals and Bt, hashed legal metadata, the VALU
// expansion to a dense A, C poisoned, the sparse GEMM, and the dense bf16 check of C against expanded A x Bt^T.
// Mode 7 = fp32, on the f8 context (its operands and product have the sizes of that context's buffers): hashed
// floats, C poisoned, the f32 GEMM at 256 x 256 x 128, its fp32 VALU check, one read-back.
AMDPROBE_EXPORT int amdprobe_readiness_f8(int device, unsigned seed, int mode, int inject, double* rel_err) {
  if (mode < 0 || mode > 7) return ERR_SHAPE;
  if (mode == 7) {
    static_assert(size_t(RM + RN) * RK32 * sizeof(float) == F8_BYTES[BUF_AB] && RM % f32::BM == 0 &&
                      RN % f32::BN == 0 && RK32 <= f32::CHECK_MAX_K,
                  "the fp32 mode runs on the f8 context's buffers");
    return run_probe(g_readiness_f8, F8_BYTES, device, seed, rel_err, nullptr, [&](ProbeCtx& ctx, uint32_t call_seed) {
      hipStream_t s = ctx.stream;
      const float* A = (const float*)ctx.buf[BUF_AB];
      const float* Bt = A + size_t(RM) * RK32;
      float* C = (float*)ctx.buf[BUF_C];
      PROBE_TRY(launch_fill_f32(ctx.buf[BUF_AB], F8_BYTES[BUF_AB], call_seed, ctx.res, s));
      PROBE_TRY(hipMemsetAsync(C, 0xFF, C_BYTES, s));  // NaN until the GEMM writes
      if (inject != 3) PROBE_TRY(amdprobe_gemm_f32_nt(A, Bt, C, RM, RN, RK32, s));
      PROBE_TRY(amdprobe_gemm_f32_check(A, Bt, C, RM, RN, RK32, inject == 1 ? 1 : 0, &ctx.res->diff2, s));
      return 0;
    });
  }
  if (mode == 6)
    return run_probe(g_readiness_sp, SP_BYTES, device, seed, rel_err, nullptr, [&](ProbeCtx& ctx, uint32_t call_seed) {
      hipStream_t s = ctx.stream;
      char* A = (char*)ctx.buf[BUF_AB];
      char* Bt = A + SP_A_BYTES;
      char* vals = Bt + SP_BT_BYTES;
      void* meta = ctx.buf[BUF_AUX];
      float* C = (float*)ctx.buf[BUF_C];
      PROBE_TRY(launch_fill(Bt, SP_BT_BYTES + SP_A_BYTES / 2, call_seed, FILL_BF16, 0, ctx.res, s));
      PROBE_TRY(launch_fill_meta24(meta, SP_BYTES[BUF_AUX], call_seed ^ 0x5CA1E5u, nullptr, s));
      PROBE_TRY(amdprobe_sp24_expand(vals, meta, A, RM, RKSP, s));
      PROBE_TRY(hipMemsetAsync(C, 0xFF, C_BYTES, s));  // NaN until the GEMM writes
      if (inject != 3) PROBE_TRY(amdprobe_gemm_sp_bf16_nt(vals, meta, Bt, C, RM, RN, RKSP, s));
      PROBE_TRY(amdprobe_gemm_check(A, Bt, C, RM, RN, RKSP, inject == 1 ? 1 : 0, &ctx.res->diff2, s));
      return 0;
    });
  if (mode == 5)
    return run_probe(g_readiness_f64, F64_BYTES, device, seed, rel_err, nullptr, [&](ProbeCtx& ctx, uint32_t call_seed) {
      hipStream_t s = ctx.stream;
      const double* A = (const double*)ctx.buf[BUF_AB];
      const double* Bt = A + size_t(RM) * RK64;
      double* C = (double*)ctx.buf[BUF_C];
      PROBE_TRY(launch_fill_f64(ctx.buf[BUF_AB], F64_BYTES[BUF_AB], call_seed, ctx.res, s));
      PROBE_TRY(hipMemsetAsync(C, 0xFF, F64_BYTES[BUF_C], s));  // NaN until the GEMM writes
      if (inject != 3) PROBE_TRY(amdprobe_gemm_f64_nt(A, Bt, C, RM, RN, RK64, s));
      PROBE_TRY(amdprobe_gemm_f64_check(A, Bt, C, RM, RN, RK64, inject == 1 ? 1 : 0, &ctx.res->diff2, s));
      return 0;
    });
  return run_probe(g_readiness_f8, F8_BYTES, device, seed, rel_err, nullptr, [&](ProbeCtx& ctx, uint32_t call_seed) {
    hipStream_t s = ctx.stream;
    const bool f4 = mode == 3, i8 = mode == 4, mx = mode == 2 || f4;
    const int fmt = mode == 1 ? F8_E5M2 : F8_E4M3;
    const size_t row_bytes = f4 ? RK / 2 : RK;
    uint8_t* scales = (uint8_t*)ctx.buf[BUF_AUX];
    const uint8_t* A = (const uint8_t*)ctx.buf[BUF_AB];
    const uint8_t* Bt = A + size_t(RM) * row_bytes;
    const uint8_t* sa = mx ? scales : nullptr;
    const uint8_t* sb = mx ? scales + size_t(RM) * (RK / 32) : nullptr;
    float* C = (float*)ctx.buf[BUF_C];
    float* out2 = &ctx.res->diff2;
    const int lose = inject == 1 ? 1 : 0;
    PROBE_TRY(launch_fill(ctx.buf[BUF_AB], size_t(RM + RN) * row_bytes, call_seed,
                          f4 || i8 ? FILL_E2M1 : mode == 1 ? FILL_E5M2 : FILL_E4M3, 0, ctx.res, s));
    if (mx) PROBE_TRY(launch_fill(scales, F8_BYTES[BUF_AUX], call_seed ^ 0x5CA1E5u, FILL_SCALE, 0, nullptr, s));
    PROBE_TRY(hipMemsetAsync(C, 0xFF, C_BYTES, s));  // NaN (int8: -1) until the GEMM writes
    if (i8) {
      if (inject != 3) PROBE_TRY(amdprobe_gemm_i8_nt(A, Bt, (int*)C, RM, RN, RK, s));
      PROBE_TRY(amdprobe_gemm_i8_check(A, Bt, (const int*)C, RM, RN, RK, lose, out2, s));
      return 0;
    }
    if (inject != 3)
      PROBE_TRY(f4 ? amdprobe_gemm_f4_nt(A, Bt, C, RM, RN, RK, sa, sb, s)
                  : amdprobe_gemm_f8_nt(A, Bt, C, RM, RN, RK, fmt, fmt, sa, sb, s));
    PROBE_TRY(f4 ? amdprobe_gemm_f4_check(A, Bt, C, RM, RN, RK, sa, sb, lose, out2, s)
                : amdprobe_gemm_f8_check(A, Bt, C, RM, RN, RK, fmt, fmt, sa, sb, lose, out2, s));
    return 0;
  });
}
