// FP8 / MXFP8 MFMA kernels of the readiness probe (gfx950). #included after probe_kernels.hip
// (uses its floatx4, xcd_remap, grouped_tile, glds16 and the shared parts of the dense check).
//
// The bf16 kernels exercise v_mfma_f32_16x16x32_bf16 only. FP8 and block-scaled (MX) payloads run
// on a different part of the matrix pipe: the f8f6f4 instructions with a 32-byte-per-lane operand
// path, and the E8M0 block-scale inputs of v_mfma_scale_*. These kernels put both under the probe.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amdprobe {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

enum { F8_E4M3 = 0, F8_E5M2 = 1 };   // OCP encodings; the values are the instruction's cbsz / blgp

// ---------------------------------------------------------------------------------------
// FP8 GEMM:  C[M][N] (fp32) = A[M][K] * Bt[N][K]^T, A and Bt K-contiguous bytes (E4M3 or E5M2 per
// operand: template FA / FB). MX = true adds E8M0 block scales sa[M][K/32], sb[N][K/32] (one byte
// per 32 consecutive K elements, value 2^(s - 127)) which go to the instruction's scale inputs:
// v_mfma_scale_f32_16x16x128_f8f6f4. Nothing is pre-multiplied in software. MX = false passes
// constant-zero scales, which the compiler lowers to the unscaled v_mfma_f32_16x16x128_f8f6f4.
//
// Work split. Block tile 128x128, BK = 128 elements = 128-B rows. 256 threads = 2x2 waves, each
// wave 64x64 = 4x4 MFMA 16x16x128: 16 MFMAs per wave per K-tile, operands fully register
// resident (8 fragments x 8 VGPRs) before the first MFMA of the tile issues.
//
// Fragments. The 16x16x128 f8 MFMA consumes K as two halves of 64: lane (i = lane & 15,
// q = lane >> 4) supplies row i of a 16-row group, K bytes [16q, 16q + 16) in VGPRs 0-3 and
// [64 + 16q, 64 + 16q + 16) in VGPRs 4-7, i.e. logical 16-B chunks q and 4 + q of the 128-B row,
// read with two ds_read_b128 into one v8i32. (Feeding a lane 32 contiguous bytes instead is the
// same product unscaled, a K permutation common to A and B, but puts each lane's bytes in two
// different 32-element scale blocks: the MX exact test pins the order used here.)
//
// LDS image. Rows are 128 B unpadded; 16-B chunk c of tile row r is stored at chunk
// c ^ ((r >> 1) & 7). Argument that both reads of a fragment are conflict-free: a ds_read_b128
// is served 16 lanes at a time (16 x 16 B = all 64 banks once), and a lane group has one q, so
// within ONE read instruction all 16 lanes ask for the same logical chunk c (q in the first
// read, 4 + q in the second) of rows i = 0..15. The 256-B bank window holds two rows: even rows
// fall in its first half, odd rows in its second. Among the 8 rows of one parity (i >> 1) & 7 takes
// each value once, and x -> c ^ x is a bijection for any fixed c, so those 8 lanes hit 8 distinct
// 16-B slots of their half: 16 lanes, 16 distinct slots, every bank once. The argument never
// uses which c, so two chunks per lane need no change to the bf16 256-kernel's permutation; it
// only needs the two chunks of a lane to come from separate instructions (they do: physical
// chunks p and p ^ 4). (r >> 1) & 7 == (i >> 1) & 7 since fragment groups start at
// multiples of 16 rows.
//
// Staging. global_load_lds_dwordx4 (glds16) writes LDS lane-linearly (wave base + 16 * lane), so
// the permutation is applied to each lane's global SOURCE address: LDS slot p = j * 256 + tid
// (row p >> 3, physical chunk p & 7) is fed from logical chunk (p & 7) ^ ((row >> 1) & 7). 8 glds16
// per thread per K-tile (4 A + 4 B); MX adds one global_load_lds_dword per thread for the tile's
// 512 + 512 scale bytes (threads 0-127: A row tid's 4 K-block scales, threads 128-255: B's).
//
// Ring depth: D = 2 LDS buffers of 32 KiB (+1 KiB scales). LDS is 160 KiB per CU and the kernel
// runs 2 workgroups per CU (two waves per SIMD, so one wave's LDS reads and barriers hide under
// the other's MFMAs): 2 x 2 x 33 = 132 KiB fits, a third buffer (198 KiB) does not. Because the
// fragments of tile t are all in registers before its MFMAs start, buffer t & 1 is free again
// right after those reads, and tile t + 2 is staged into it BEFORE the 16 MFMAs of tile t. The
// pipeline is therefore three tiles deep on two buffers: t in registers / matrix pipe, t + 1
// landing, t + 2 just issued. Per K-tile:
//     s_waitcnt vmcnt(P)      own pieces of tile t landed; tile t + 1 (P ops) stays in flight
//     s_barrier               everyone's pieces of tile t landed
//     16 ds_read_b128 (+ 8 ds_read_u8 scales), s_waitcnt lgkmcnt(0)
//     s_barrier               everyone finished reading buffer t & 1
//     stage(t + 2) -> buffer t & 1
//     16 MFMA
// P = 8 (9 with MX): the wait is counted, never 0 until the last tile.
//
// Scales. The scale of row i, 32-element K-block j is taken from lane i + 16j (so lane (i, q)
// supplies block q, which is NOT the block its own data bytes are in: those are halves of blocks
// q >> 1 and 2 + (q >> 1)). From the
// staged [row][4] bytes a lane reads byte q of its row in each of the wave's 4 m-tiles (n-tiles)
// and packs them into one dword, byte m = m-tile m; the MFMA of tile (m, n) selects them with
// opsel_a = m, opsel_b = n.
//
// Tile order: xcd_remap + grouped_tile (8-row bands), as the bf16 kernels. Epilogue: 16x16
// accumulator layout, row (lane >> 4) * 4 + j, col lane & 15.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage, gfx950): unscaled 158 VGPRs,
// 64 KiB LDS; MX 170 VGPRs, 66 KiB LDS; no AGPRs, no scratch, no spills; occupancy 2 waves per
// SIMD = 2 workgroups per CU (the plan above). gemm_f8_check_kernel: 47 VGPRs, 33.5 KiB LDS, no
// scratch.
// ---------------------------------------------------------------------------------------
namespace f8 {
constexpr int BM = 128, BN = 128, BK = 128, THREADS = 256;
constexpr int OPER_BYTES = BM * BK;              // 16 KiB, one operand tile
constexpr int SCALE_BYTES = (BM + BN) * 4;       // 1 KiB, MX only
constexpr int RING = 2;
}  // namespace f8

__device__ __forceinline__ void glds4(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)gsrc, (lds_void*)lds_wave_base, 4, 0, 0);
}

template <int FA, int FB, bool MX, int OA, int OB>
__device__ __forceinline__ floatx4 mfma_f8(intx8 a, intx8 b, floatx4 c, int sa, int sb) {
  if constexpr (MX)
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, OA, sa, OB, sb);
  else
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, 0, 0, 0, 0);
}

template <int FA, int FB, bool MX>
__global__ __launch_bounds__(f8::THREADS, 2)
void gemm_f8_nt_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt, float* __restrict__ C,
                       const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb, int M, int N, int K) {
  constexpr int BM = f8::BM, BN = f8::BN, BK = f8::BK, OPER_BYTES = f8::OPER_BYTES;
  constexpr int BUF_BYTES = 2 * OPER_BYTES + (MX ? f8::SCALE_BYTES : 0);
  __shared__ __attribute__((aligned(1024))) char smem[f8::RING * BUF_BYTES];
  const int tiles_n = N / BN;
  const int nwg = (M / BM) * tiles_n;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, nwg), M / BM, tiles_n, 8, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  const uint8_t* Ablk = A + (size_t)tm * BM * K;
  const uint8_t* Bblk = Bt + (size_t)tn * BN * K;
  // staging: this lane's four 16-B pieces of an operand tile (loop invariant byte offsets)
  size_t soff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = j * 256 + tid;                   // 16-B slot in the operand tile image
    const int row = p >> 3, chunk = (p & 7) ^ ((row >> 1) & 7);
    soff[j] = (size_t)row * K + chunk * 16;
  }
  // MX: thread tid < 128 stages A row tid's scale dword, thread tid >= 128 B row tid - 128's
  const int kb_row = K / 32;
  const uint8_t* ssrc = nullptr;
  if constexpr (MX)
    ssrc = tid < BM ? sa + ((size_t)tm * BM + tid) * kb_row : sb + ((size_t)tn * BN + (tid - BM)) * kb_row;
  char* const wave_dst = smem + wave * 1024;
  auto stage = [&](int t) {
    char* dst = wave_dst + (t & 1) * BUF_BYTES;
    const uint8_t* a = Ablk + (size_t)t * BK;
    const uint8_t* b = Bblk + (size_t)t * BK;
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(a + soff[j], dst + j * 4096);
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(b + soff[j], dst + OPER_BYTES + j * 4096);
    if constexpr (MX) glds4(ssrc + t * 4, smem + (t & 1) * BUF_BYTES + 2 * OPER_BYTES + wave * 256);
  };
  // fragment reads: row i of a 16-row group, logical chunks q and 4 + q
  const int fi = lane & 15, fq = lane >> 4;
  const int pc0 = (fq ^ ((fi >> 1) & 7)) << 4, pc1 = pc0 ^ 64;
  const int rA = (wr * 64 + fi) * BK;              // within the A tile
  const int rB = OPER_BYTES + (wc * 64 + fi) * BK; // within the buffer
  const int sA = 2 * OPER_BYTES + (wr * 64 + fi) * 4 + fq;
  const int sB = 2 * OPER_BYTES + BM * 4 + (wc * 64 + fi) * 4 + fq;

  floatx4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nt = K / BK;
  stage(0);
  if (nt > 1) stage(1);
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      if constexpr (MX) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* buf = smem + (t & 1) * BUF_BYTES;
    intx8 af[4], bfr[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const intx4 lo = *reinterpret_cast<const intx4*>(buf + rA + m * 16 * BK + pc0);
      const intx4 hi = *reinterpret_cast<const intx4*>(buf + rA + m * 16 * BK + pc1);
      af[m] = intx8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const intx4 lo = *reinterpret_cast<const intx4*>(buf + rB + n * 16 * BK + pc0);
      const intx4 hi = *reinterpret_cast<const intx4*>(buf + rB + n * 16 * BK + pc1);
      bfr[n] = intx8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    int sca = 0, scb = 0;
    if constexpr (MX) {
      const uint8_t* s8 = reinterpret_cast<const uint8_t*>(buf);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        sca |= (int)s8[sA + m * 64] << (8 * m);    // byte m = m-tile m (16 rows x 4 B apart)
        scb |= (int)s8[sB + m * 64] << (8 * m);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < nt) stage(t + 2);
    __builtin_amdgcn_s_setprio(1);
#define F8_ROW(m)                                                            \
  acc[m][0] = mfma_f8<FA, FB, MX, m, 0>(af[m], bfr[0], acc[m][0], sca, scb); \
  acc[m][1] = mfma_f8<FA, FB, MX, m, 1>(af[m], bfr[1], acc[m][1], sca, scb); \
  acc[m][2] = mfma_f8<FA, FB, MX, m, 2>(af[m], bfr[2], acc[m][2], sca, scb); \
  acc[m][3] = mfma_f8<FA, FB, MX, m, 3>(af[m], bfr[3], acc[m][3], sca, scb);
    F8_ROW(0) F8_ROW(1) F8_ROW(2) F8_ROW(3)
#undef F8_ROW
    __builtin_amdgcn_s_setprio(0);
  }
  // epilogue: col = lane & 15, row = (lane >> 4) * 4 + j
  float* Cblk = C + (size_t)tm * BM * N + (size_t)tn * BN;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wr * 64 + m * 16 + (lane >> 4) * 4 + j;
        const int col = wc * 64 + n * 16 + (lane & 15);
        Cblk[(size_t)row * N + col] = acc[m][n][j];
      }
}

// ---------------------------------------------------------------------------------------
// Dense check of the FP8 product, the counterpart of gemm_check_kernel on its staging and finish
// (probe_kernels.hip). Every element's reference never touches the matrix pipe: bytes are decoded
// on the VALU (v_cvt_pk_f32_fp8 / _bf8) and summed with fp32 FMAs, 32 elements at a time; with
// scales each 32-element partial sum is multiplied by 2^(sa - 127) * 2^(sb - 127) with ldexpf.
// Needs M, N % 16 == 0, K % 32 == 0, K <= CHECK_MAX_K (host-checked).
// ---------------------------------------------------------------------------------------

template <int F>
__device__ __forceinline__ void f8_decode4(uint32_t w, float* o) {
  floatx2 lo, hi;
  if constexpr (F == F8_E4M3) {
    lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  } else {
    lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
  }
  o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}

template <int FA, int FB>
__global__ __launch_bounds__(CHECK_THREADS)
void gemm_f8_check_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt, const float* __restrict__ C,
                          const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb, int M, int N, int K,
                          int inject, float* __restrict__ out2) {
  __shared__ __attribute__((aligned(16))) uint8_t la[CHECK_TILE * (CHECK_MAX_K + 16)];
  __shared__ __attribute__((aligned(16))) uint8_t lb[CHECK_TILE * (CHECK_MAX_K + 16)];
  __shared__ uint8_t lsa[CHECK_TILE * (CHECK_MAX_K / 32)], lsb[CHECK_TILE * (CHECK_MAX_K / 32)];
  const CheckPos t(N);
  const int r = t.r, c = t.c, kblocks = K / 32;
  const bool scaled = sa != nullptr;
  check_stage_rows(A, Bt, t, K, la, lb);
  if (scaled) check_stage_scales(sa, sb, t, kblocks, lsa, lsb);
  __syncthreads();
  const uint8_t* pa = la + r * (K + 16);
  const uint8_t* pb = lb + c * (K + 16);
  float ref = 0.f;
  for (int kb = 0; kb < kblocks; ++kb) {
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint4 a4 = *reinterpret_cast<const uint4*>(pa + kb * 32 + h * 16);
      const uint4 b4 = *reinterpret_cast<const uint4*>(pb + kb * 32 + h * 16);
      const uint32_t aw[4] = {a4.x, a4.y, a4.z, a4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float fa[4], fb[4];
        f8_decode4<FA>(aw[w], fa);
        f8_decode4<FB>(bw[w], fb);
        p0 = fmaf(fa[0], fb[0], p0);
        p1 = fmaf(fa[1], fb[1], p1);
        p0 = fmaf(fa[2], fb[2], p0);
        p1 = fmaf(fa[3], fb[3], p1);
      }
    }
    float p = p0 + p1;
    if (scaled) p = ldexpf(p, (int)lsa[r * kblocks + kb] + (int)lsb[c * kblocks + kb] - 254);
    ref += p;
  }
  check_finish(C, N, t, ref, inject, out2);
}

}  // namespace amdprobe
