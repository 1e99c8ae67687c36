// C ABI over the probe kernels; loaded in-process by dcos_commons_amd.ops (ctypes) with torch
// tensors' device pointers and the current HIP stream. Every entry point validates the shapes
// the kernel's grid assumes before launching and returns a hipError_t (0 = success) or a
// negative code for a rejected shape.
#include "probe_kernels.hip"
#include "f8_kernels.hip"
#include "f4_kernels.hip"

#include <cmath>
#include <mutex>

#define AMDPROBE_EXPORT extern "C" __attribute__((visibility("default")))

using namespace amdprobe;

enum { ERR_SHAPE = -1, ERR_ALIGN = -2 };

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

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

// Dense fp32 check of C = A Bt^T: adds sum((C - A Bt^T)^2) to out2[0] and sum((A Bt^T)^2) to
// out2[1] (device pointer, 2 floats that the caller zeroes).
AMDPROBE_EXPORT int amdprobe_gemm_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                        int inject, float* out2, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || M % CHECK_TILE || N % CHECK_TILE || K % 8 || K > CHECK_MAX_K) return ERR_SHAPE;
  if (!aligned16(A) || !aligned16(Bt)) return ERR_ALIGN;
  hipLaunchKernelGGL(gemm_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const __bf16*)A, (const __bf16*)Bt, C, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// The readiness operand fill on its own (tests compare it with a host model of the hash):
// `ab` gets `ab_bytes` of hashed bf16 and `res` (32 bytes) is zeroed.
AMDPROBE_EXPORT int amdprobe_readiness_fill(void* ab, size_t ab_bytes, unsigned seed, void* res, void* stream) {
  if (ab_bytes == 0 || ab_bytes % 16) return ERR_SHAPE;
  if (!aligned16(ab) || !aligned16(res)) return ERR_ALIGN;
  hipLaunchKernelGGL(readiness_prep_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, (uint4*)ab, ab_bytes / 16,
                     (uint32_t)seed, (ReadinessResult*)res);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// amdprobe_readiness: the whole readiness check of one device in one call (see the kernel file).
// Buffers, a non-blocking stream and a pinned result slot are created on first use per device
// and reused; calls for one device serialize on its context. The calling thread's current device
// is restored. inject: 0 = none, 1 = lose one 16x16 tile of the product (the check must fail), 2 = corrupt one
// pattern word (the memory check must count it), 3 = skip the GEMM launch, 4 = skip the pattern write (both
// model a kernel that silently drops its writes; the check must still fail). Returns 0 or a HIP error /
// negative shape code.
//
// The buffers outlive the call, so a kernel that dropped its writes would leave the previous call's correct
// data behind. Two things stop that from passing: C is poisoned with NaN bytes before the GEMM, and every
// call mixes a per-device call counter into the seed, so the operands and the pattern differ from the last
// call's and stale data cannot match.
// ---------------------------------------------------------------------------------------
namespace {
constexpr int RM = 256, RN = 256, RK = 512;
constexpr size_t PATTERN_BYTES = size_t(64) << 20;
constexpr int MAX_DEVICES = 64;

struct ReadinessCtx {
  std::mutex mu;
  bool ready = false;
  hipStream_t stream = nullptr;
  __bf16* ab = nullptr;          // A (RM x RK) then Bt (RN x RK)
  float* c = nullptr;            // RM x RN
  uint4* pattern = nullptr;
  ReadinessResult* res = nullptr;
  ReadinessResult* host = nullptr;  // pinned
  uint32_t calls = 0;               // mixed into the seed: no two calls share operands or pattern
};
ReadinessCtx g_readiness[MAX_DEVICES];

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

#define PROBE_TRY(expr)                                  \
  do {                                                   \
    const hipError_t e_ = (expr);                        \
    if (e_ != hipSuccess) return (int)e_;                \
  } while (0)

void readiness_release(ReadinessCtx& ctx) {
  if (ctx.stream != nullptr) (void)hipStreamDestroy(ctx.stream);
  if (ctx.ab != nullptr) (void)hipFree(ctx.ab);
  if (ctx.c != nullptr) (void)hipFree(ctx.c);
  if (ctx.pattern != nullptr) (void)hipFree(ctx.pattern);
  if (ctx.res != nullptr) (void)hipFree(ctx.res);
  if (ctx.host != nullptr) (void)hipHostFree(ctx.host);
  ctx.stream = nullptr;
  ctx.ab = nullptr;
  ctx.c = nullptr;
  ctx.pattern = nullptr;
  ctx.res = nullptr;
  ctx.host = nullptr;
}

int readiness_alloc(ReadinessCtx& ctx) {
  PROBE_TRY(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
  PROBE_TRY(hipMalloc((void**)&ctx.ab, size_t(RM + RN) * RK * sizeof(__bf16)));
  PROBE_TRY(hipMalloc((void**)&ctx.c, size_t(RM) * RN * sizeof(float)));
  PROBE_TRY(hipMalloc((void**)&ctx.pattern, PATTERN_BYTES));
  PROBE_TRY(hipMalloc((void**)&ctx.res, sizeof(ReadinessResult)));
  PROBE_TRY(hipHostMalloc((void**)&ctx.host, sizeof(ReadinessResult), hipHostMallocDefault));
  return 0;
}

// The context lives for the process (one probe per pod launch reuses it); a failed allocation
// releases whatever it got, so the next call starts clean instead of leaking.
int readiness_init(ReadinessCtx& ctx) {
  const int rc = readiness_alloc(ctx);
  if (rc) {
    readiness_release(ctx);
    return rc;
  }
  ctx.ready = true;
  return 0;
}
}  // namespace

AMDPROBE_EXPORT int amdprobe_readiness(int device, unsigned seed, int inject, double* rel_err,
                                       unsigned long long* bad_words) {
  if (rel_err == nullptr || bad_words == nullptr || device < 0 || device >= MAX_DEVICES) return ERR_SHAPE;
  int ndev = 0;
  PROBE_TRY(hipGetDeviceCount(&ndev));
  if (device >= ndev) return ERR_SHAPE;
  ReadinessCtx& ctx = g_readiness[device];
  std::lock_guard<std::mutex> lock(ctx.mu);
  DeviceGuard guard(device);
  if (!ctx.ready) {
    const int rc = readiness_init(ctx);
    if (rc) return rc;
  }
  hipStream_t s = ctx.stream;
  const __bf16* A = ctx.ab;
  const __bf16* Bt = ctx.ab + size_t(RM) * RK;
  const uint32_t call_seed = (uint32_t)seed ^ (0x9E3779B9u * ++ctx.calls);
  hipLaunchKernelGGL(readiness_prep_kernel, dim3(64), dim3(256), 0, s, (uint4*)ctx.ab,
                     size_t(RM + RN) * RK * sizeof(__bf16) / 16, call_seed, ctx.res);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemsetAsync(ctx.c, 0xFF, size_t(RM) * RN * sizeof(float), s));  // NaN until the GEMM writes
  if (inject != 3) {
    // 128x128 tiles: four workgroups for the 256x256 product (one 256x256-tile workgroup takes ~15 us)
    const int rc = amdprobe_gemm_bf16_nt_variant(A, Bt, ctx.c, RM, RN, RK, 1, s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(gemm_check_kernel, dim3((RM / CHECK_TILE) * (RN / CHECK_TILE)), dim3(CHECK_THREADS), 0, s, A,
                     Bt, (const float*)ctx.c, RM, RN, RK, inject == 1 ? 1 : 0, &ctx.res->diff2);
  PROBE_TRY(hipGetLastError());
  if (inject != 4) {
    hipLaunchKernelGGL(pattern_write_kernel, dim3(2048), dim3(256), 0, s, ctx.pattern, PATTERN_BYTES / 16,
                       call_seed);
    PROBE_TRY(hipGetLastError());
  }
  if (inject == 2) PROBE_TRY(hipMemsetAsync(ctx.pattern, 0, 4, s));
  hipLaunchKernelGGL(pattern_check_kernel, dim3(2048), dim3(256), 0, s, (const uint4*)ctx.pattern,
                     PATTERN_BYTES / 16, call_seed, &ctx.res->bad_words);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpyAsync(ctx.host, ctx.res, sizeof(ReadinessResult), hipMemcpyDeviceToHost, s));
  PROBE_TRY(hipStreamSynchronize(s));
  const double d2 = ctx.host->diff2, w2 = ctx.host->ref2;
  *rel_err = (w2 > 0.0 && std::isfinite(d2)) ? std::sqrt(d2 / w2) : HUGE_VAL;  // NaN C (never written) fails
  *bad_words = ctx.host->bad_words;
  return 0;
}

// ---------------------------------------------------------------------------------------
// FP8 / MXFP8 (f8_kernels.hip). fmt_a / fmt_b: 0 = E4M3, 1 = E5M2 (OCP); the pairs built are
// E4M3 x E4M3, E5M2 x E5M2 and E4M3 x E5M2. sa / sb: E8M0 block scales [M][K/32], [N][K/32], both
// null for an unscaled product.
// ---------------------------------------------------------------------------------------
namespace {
template <bool MX>
int launch_gemm_f8(const uint8_t* A, const uint8_t* Bt, float* C, const uint8_t* sa, const uint8_t* sb, int M, int N,
                   int K, int fmt_a, int fmt_b, hipStream_t s) {
  const dim3 grid((M / f8::BM) * (N / f8::BN)), block(f8::THREADS);
  if (fmt_a == F8_E4M3 && fmt_b == F8_E4M3)
    hipLaunchKernelGGL((gemm_f8_nt_kernel<F8_E4M3, F8_E4M3, MX>), grid, block, 0, s, A, Bt, C, sa, sb, M, N, K);
  else if (fmt_a == F8_E5M2 && fmt_b == F8_E5M2)
    hipLaunchKernelGGL((gemm_f8_nt_kernel<F8_E5M2, F8_E5M2, MX>), grid, block, 0, s, A, Bt, C, sa, sb, M, N, K);
  else if (fmt_a == F8_E4M3 && fmt_b == F8_E5M2)
    hipLaunchKernelGGL((gemm_f8_nt_kernel<F8_E4M3, F8_E5M2, MX>), grid, block, 0, s, A, Bt, C, sa, sb, M, N, K);
  else
    return ERR_SHAPE;
  return (int)hipGetLastError();
}
}  // namespace

AMDPROBE_EXPORT int amdprobe_gemm_f8_nt(const void* A, const void* Bt, float* C, int M, int N, int K, int fmt_a,
                                        int fmt_b, const void* sa, const void* sb, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || M % f8::BM || N % f8::BN || K % f8::BK) return ERR_SHAPE;
  if ((sa == nullptr) != (sb == nullptr)) return ERR_SHAPE;
  if (!aligned16(A) || !aligned16(Bt) || !aligned16(C) || !aligned16(sa) || !aligned16(sb)) return ERR_ALIGN;
  const uint8_t *a = (const uint8_t*)A, *b = (const uint8_t*)Bt, *pa = (const uint8_t*)sa, *pb = (const uint8_t*)sb;
  return sa != nullptr ? launch_gemm_f8<true>(a, b, C, pa, pb, M, N, K, fmt_a, fmt_b, (hipStream_t)stream)
                       : launch_gemm_f8<false>(a, b, C, pa, pb, M, N, K, fmt_a, fmt_b, (hipStream_t)stream);
}

// Dense VALU check of an FP8 product: adds sum((C - ref)^2) to out2[0] and sum(ref^2) to out2[1]
// (device pointer, 2 floats that the caller zeroes).
AMDPROBE_EXPORT int amdprobe_gemm_f8_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                           int fmt_a, int fmt_b, const void* sa, const void* sb, int inject,
                                           float* out2, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || M % CHECK_TILE || N % CHECK_TILE || K % 32 || K > F8_CHECK_MAX_K)
    return ERR_SHAPE;
  if ((sa == nullptr) != (sb == nullptr)) return ERR_SHAPE;
  if (!aligned16(A) || !aligned16(Bt)) return ERR_ALIGN;
  const dim3 grid((M / CHECK_TILE) * (N / CHECK_TILE)), block(CHECK_THREADS);
  const uint8_t *a = (const uint8_t*)A, *b = (const uint8_t*)Bt, *pa = (const uint8_t*)sa, *pb = (const uint8_t*)sb;
  hipStream_t s = (hipStream_t)stream;
  if (fmt_a == F8_E4M3 && fmt_b == F8_E4M3)
    hipLaunchKernelGGL((gemm_f8_check_kernel<F8_E4M3, F8_E4M3>), grid, block, 0, s, a, b, C, pa, pb, M, N, K, inject,
                       out2);
  else if (fmt_a == F8_E5M2 && fmt_b == F8_E5M2)
    hipLaunchKernelGGL((gemm_f8_check_kernel<F8_E5M2, F8_E5M2>), grid, block, 0, s, a, b, C, pa, pb, M, N, K, inject,
                       out2);
  else if (fmt_a == F8_E4M3 && fmt_b == F8_E5M2)
    hipLaunchKernelGGL((gemm_f8_check_kernel<F8_E4M3, F8_E5M2>), grid, block, 0, s, a, b, C, pa, pb, M, N, K, inject,
                       out2);
  else
    return ERR_SHAPE;
  return (int)hipGetLastError();
}

// The readiness operand fill on its own: kind 0 = E4M3 bytes, 1 = E5M2 bytes, 2 = E8M0 block
// scales (see f8_fill_kernel), 3 = packed E2M1 nibbles (any byte). `zero2` (2 floats) may be null.
AMDPROBE_EXPORT int amdprobe_f8_fill(void* p, size_t bytes, unsigned seed, int kind, float* zero2, void* stream) {
  if (bytes == 0 || bytes % 16 || kind < F8_FILL_E4M3 || kind > F4_FILL_E2M1) return ERR_SHAPE;
  if (!aligned16(p)) return ERR_ALIGN;
  static const uint32_t and4[4] = {0x87878787u, 0x83838383u, 0x07070707u, 0xFFFFFFFFu};
  static const uint32_t add4[4] = {0x30303030u, 0x38383838u, 0x7C7C7C7Cu, 0u};
  const int blocks = (int)((bytes / 16 + 255) / 256 < 1024 ? (bytes / 16 + 255) / 256 : 1024);
  hipLaunchKernelGGL(f8_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)p, bytes / 16,
                     (uint32_t)seed, and4[kind], add4[kind], zero2);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// FP4 / MXFP4 (f4_kernels.hip). A, Bt: packed E2M1, K/2 bytes per row. sa / sb: E8M0 block scales
// [M][K/32], [N][K/32], both null for an unscaled product.
// ---------------------------------------------------------------------------------------
AMDPROBE_EXPORT int amdprobe_gemm_f4_nt(const void* A, const void* Bt, float* C, int M, int N, int K, const void* sa,
                                        const void* sb, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || M % f4::BM || N % f4::BN || K % f4::BK) return ERR_SHAPE;
  if ((sa == nullptr) != (sb == nullptr)) return ERR_SHAPE;
  if (!aligned16(A) || !aligned16(Bt) || !aligned16(C) || !aligned16(sa) || !aligned16(sb)) return ERR_ALIGN;
  const dim3 grid((M / f4::BM) * (N / f4::BN)), block(f4::THREADS);
  const uint8_t *a = (const uint8_t*)A, *b = (const uint8_t*)Bt, *pa = (const uint8_t*)sa, *pb = (const uint8_t*)sb;
  if (sa != nullptr)
    hipLaunchKernelGGL(gemm_f4_nt_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, C, pa, pb, M, N, K);
  else
    hipLaunchKernelGGL(gemm_f4_nt_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, C, pa, pb, M, N, K);
  return (int)hipGetLastError();
}

// Dense VALU check of an FP4 product: adds sum((C - ref)^2) to out2[0] and sum(ref^2) to out2[1]
// (device pointer, 2 floats that the caller zeroes).
AMDPROBE_EXPORT int amdprobe_gemm_f4_check(const void* A, const void* Bt, const float* C, int M, int N, int K,
                                           const void* sa, const void* sb, int inject, float* out2, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || M % CHECK_TILE || N % CHECK_TILE || K % 32 || K > F4_CHECK_MAX_K)
    return ERR_SHAPE;
  if ((sa == nullptr) != (sb == nullptr)) return ERR_SHAPE;
  if (!aligned16(A) || !aligned16(Bt)) return ERR_ALIGN;
  hipLaunchKernelGGL(gemm_f4_check_kernel, dim3((M / CHECK_TILE) * (N / CHECK_TILE)), dim3(CHECK_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)A, (const uint8_t*)Bt, C, (const uint8_t*)sa,
                     (const uint8_t*)sb, M, N, K, inject, out2);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// amdprobe_readiness_f8: the FP8 matrix path of one device in one call. mode 0 = fp8 (E4M3),
// 1 = bf8 (E5M2), 2 = mxfp8 (E4M3 with E8M0 block scales through the MFMA scale inputs), 3 = mxfp4
// (packed E2M1 with block scales: the f4 GEMM and check on the same buffers, half filled). Same
// pattern as amdprobe_readiness, on a context of its own (created on first use per device): hashed
// operands, C poisoned with NaN bytes, the f8 GEMM, the dense VALU check, one 8-byte read-back on
// a private stream; the call counter is mixed into the seed. inject: 0 = none, 1 = lose one 16x16
// tile of the product, 3 = skip the GEMM launch (both must fail). There is no HBM pattern here:
// amdprobe_readiness does that.
// ---------------------------------------------------------------------------------------
namespace {
struct ReadinessF8Ctx {
  std::mutex mu;
  bool ready = false;
  hipStream_t stream = nullptr;
  uint8_t* ab = nullptr;      // A (RM x RK) then Bt (RN x RK)
  uint8_t* scales = nullptr;  // sa (RM x RK/32) then sb (RN x RK/32)
  float* c = nullptr;         // RM x RN
  float* res = nullptr;       // diff2, ref2
  float* host = nullptr;      // pinned
  uint32_t calls = 0;
};
ReadinessF8Ctx g_readiness_f8[MAX_DEVICES];

void readiness_f8_release(ReadinessF8Ctx& ctx) {
  if (ctx.stream != nullptr) (void)hipStreamDestroy(ctx.stream);
  if (ctx.ab != nullptr) (void)hipFree(ctx.ab);
  if (ctx.scales != nullptr) (void)hipFree(ctx.scales);
  if (ctx.c != nullptr) (void)hipFree(ctx.c);
  if (ctx.res != nullptr) (void)hipFree(ctx.res);
  if (ctx.host != nullptr) (void)hipHostFree(ctx.host);
  ctx.stream = nullptr;
  ctx.ab = ctx.scales = nullptr;
  ctx.c = ctx.res = ctx.host = nullptr;
}

int readiness_f8_alloc(ReadinessF8Ctx& ctx) {
  PROBE_TRY(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
  PROBE_TRY(hipMalloc((void**)&ctx.ab, size_t(RM + RN) * RK));
  PROBE_TRY(hipMalloc((void**)&ctx.scales, size_t(RM + RN) * (RK / 32)));
  PROBE_TRY(hipMalloc((void**)&ctx.c, size_t(RM) * RN * sizeof(float)));
  PROBE_TRY(hipMalloc((void**)&ctx.res, 2 * sizeof(float)));
  PROBE_TRY(hipHostMalloc((void**)&ctx.host, 2 * sizeof(float), hipHostMallocDefault));
  return 0;
}
}  // namespace

AMDPROBE_EXPORT int amdprobe_readiness_f8(int device, unsigned seed, int mode, int inject, double* rel_err) {
  if (rel_err == nullptr || device < 0 || device >= MAX_DEVICES || mode < 0 || mode > 3) return ERR_SHAPE;
  int ndev = 0;
  PROBE_TRY(hipGetDeviceCount(&ndev));
  if (device >= ndev) return ERR_SHAPE;
  ReadinessF8Ctx& ctx = g_readiness_f8[device];
  std::lock_guard<std::mutex> lock(ctx.mu);
  DeviceGuard guard(device);
  if (!ctx.ready) {
    const int rc = readiness_f8_alloc(ctx);
    if (rc) {
      readiness_f8_release(ctx);
      return rc;
    }
    ctx.ready = true;
  }
  hipStream_t s = ctx.stream;
  const bool f4 = mode == 3, mx = mode >= 2;
  const int fmt = mode == 1 ? F8_E5M2 : F8_E4M3;
  const size_t row_bytes = f4 ? RK / 2 : RK;
  const uint8_t* A = ctx.ab;
  const uint8_t* Bt = ctx.ab + size_t(RM) * row_bytes;
  const uint8_t* sa = mx ? ctx.scales : nullptr;
  const uint8_t* sb = mx ? ctx.scales + size_t(RM) * (RK / 32) : nullptr;
  const uint32_t call_seed = (uint32_t)seed ^ (0x9E3779B9u * ++ctx.calls);
  int rc = amdprobe_f8_fill(ctx.ab, size_t(RM + RN) * row_bytes, call_seed,
                            f4 ? F4_FILL_E2M1 : fmt == F8_E5M2 ? F8_FILL_E5M2 : F8_FILL_E4M3, ctx.res, s);
  if (rc) return rc;
  if (mx) {
    rc = amdprobe_f8_fill(ctx.scales, size_t(RM + RN) * (RK / 32), call_seed ^ 0x5CA1E5u, F8_FILL_SCALE, nullptr, s);
    if (rc) return rc;
  }
  PROBE_TRY(hipMemsetAsync(ctx.c, 0xFF, size_t(RM) * RN * sizeof(float), s));  // NaN until the GEMM writes
  if (inject != 3) {
    rc = f4 ? amdprobe_gemm_f4_nt(A, Bt, ctx.c, RM, RN, RK, sa, sb, s)
            : amdprobe_gemm_f8_nt(A, Bt, ctx.c, RM, RN, RK, fmt, fmt, sa, sb, s);
    if (rc) return rc;
  }
  rc = f4 ? amdprobe_gemm_f4_check(A, Bt, ctx.c, RM, RN, RK, sa, sb, inject == 1 ? 1 : 0, ctx.res, s)
          : amdprobe_gemm_f8_check(A, Bt, ctx.c, RM, RN, RK, fmt, fmt, sa, sb, inject == 1 ? 1 : 0, ctx.res, s);
  if (rc) return rc;
  PROBE_TRY(hipMemcpyAsync(ctx.host, ctx.res, 2 * sizeof(float), hipMemcpyDeviceToHost, s));
  PROBE_TRY(hipStreamSynchronize(s));
  const double d2 = ctx.host[0], w2 = ctx.host[1];
  *rel_err = (w2 > 0.0 && std::isfinite(d2)) ? std::sqrt(d2 / w2) : HUGE_VAL;  // NaN C (never written) fails
  return 0;
}
