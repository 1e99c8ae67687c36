// FP64 MFMA kernels of the readiness probe (gfx950). #included after i8_kernels.hip (uses
// probe_kernels.hip's xcd_remap, grouped_tile, glds16, mix32, ReadinessResult and the shared parts of
// the dense check).
//
// v_mfma_f64_16x16x4_f64, with 8-byte operands and fp64 accumulators, is the data path of the matrix
// pipe that HPC payloads run on, and none of the other kernels reaches it: they all accumulate in fp32
// or int32. Its check subtracts in fp64, so a product that was silently formed at single precision
// (off by 2^-24) fails where the 1e-3 bound of the other modes would pass it.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amdprobe {

typedef double doublex2 __attribute__((ext_vector_type(2)));
typedef double doublex4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// FP64 GEMM:  C[M][N] (fp64) = A[M][K] * Bt[N][K]^T, A and Bt K-contiguous doubles. Every product and
// every sum is formed by v_mfma_f64_16x16x4_f64; nothing is added in software.
//
// The instruction (CDNA3 / CDNA4 ISA, matrix layout tables; pinned by the exact `index` test): lane
// (i = lane & 15, q = lane >> 4) supplies ONE double per operand, A[i][q] and B[q][i] of the 16x4 and
// 4x16 operands. The 16x16 result is 4 doubles per lane, and unlike the fp32 16x16 layouts the four
// registers of a lane are four rows apart: register j of a lane is row 4 * j + (lane >> 4), column
// lane & 15. One instruction is 2048 flops; at the 78.6 TFLOP/s fp64 matrix peak of the part (256 CUs,
// 4 SIMDs, 2.4 GHz: 32 flops per cycle per SIMD) that is 64 cycles of the pipe per instruction, for
// 8 operand bytes per lane and operand where an f8 fragment is 32.
//
// Work split. Block tile 256 (M) x 128 (N), K-tile 16 doubles = 128-B rows. 512 threads = 8 waves as
// 4 (M) x 2 (N); wave (wr, wc) owns rows wr * 64 + [0, 64), cols wc * 64 + [0, 64) = 4 x 4 MFMA tiles:
// 16 accumulators x 8 VGPRs = 128 accumulator VGPRs (a 128x64 wave tile would be 256, the whole
// budget). 4 K-steps x 16 = 64 MFMAs = 4096 pipe cycles per wave per K-tile, two waves per SIMD.
// __launch_bounds__(512): one workgroup per CU; the registers, not LDS, set the occupancy.
//
// Fragments. A lane fetches two 16-B chunks of its row with ds_read_b128, logical chunks q and 4 + q
// of the 128-B row, i.e. the doubles k = 2q, 2q + 1 and 8 + 2q, 9 + 2q of the K-tile, and feeds four
// consecutive MFMAs from the four doubles it holds. A sum over K does not depend on which K elements
// one MFMA takes as long as the A and B lanes of a K-group q take the same ones (they do: the same
// chunk and the same double of their rows); only the summation order differs from k = 0, 1, 2, ...
// MFMA (h, s), h the chunk (0: q, 1: 4 + q) and s the double in it, consumes the K elements
// {8h + s + 2q : q = 0..3} of the tile:
//     MFMA 0 (h0, s0): k = 0, 2, 4, 6        MFMA 1 (h0, s1): k = 1, 3, 5, 7
//     MFMA 2 (h1, s0): k = 8, 10, 12, 14     MFMA 3 (h1, s1): k = 9, 11, 13, 15
// That is 2 LDS reads per fragment row group per 4 MFMA K-steps, not one ds_read_b64 per MFMA.
//
// LDS image: 128-B rows unpadded, 16-B chunk c of tile row r stored at chunk c ^ ((r >> 1) & 7).
// Conflict freedom, derived for this read (two doubles per chunk, 16-row groups, 4 K-groups): a
// ds_read_b128 is served 16 lanes at a time (16 x 16 B = all 64 banks once). 16 consecutive lanes
// have one q (q = lane >> 4), and one read instruction has one h, so all 16 ask for the SAME logical
// chunk c = 4h + q, of the 16 rows i = 0..15 of a fragment group that starts at a multiple of 16
// rows, hence (r >> 1) & 7 == (i >> 1) & 7. The 256-B bank window holds two rows: even rows fall in
// its first half, odd rows in its second. Among the 8 rows of one parity (i >> 1) & 7 takes each value
// once and x -> c ^ x is a bijection for any fixed c, so the 8 lanes of a parity hit the 8 distinct
// 16-B slots of their half: 16 lanes, 16 distinct slots, every bank once. The two chunks of a lane
// come from two instructions (physical chunks p and p ^ 4). The address pattern is that of the f8
// fragment; what is new is that the 16 bytes are two K elements and that the K-group is the chunk.
//
// Staging. global_load_lds_dwordx4 (glds16) writes LDS lane-linearly, so the permutation is applied
// to the lane's global SOURCE address: slot p = j * 512 + tid of an operand image (row p >> 3 =
// j * 64 + (tid >> 3), physical chunk p & 7 = tid & 7) is fed from logical chunk (tid & 7) ^
// ((row >> 1) & 7); j * 64 rows does not change (row >> 1) & 7, so a lane has one offset per operand
// stride. 6 glds16 per thread per K-tile: 4 for the 32 KiB of A, 2 for the 16 KiB of Bt.
//
// Schedule. A K-tile is 4096 matrix-pipe cycles per wave and 8192 per SIMD, against 16 ds_read_b128
// per wave: LDS traffic is nothing against matrix time, and what is left to hide is barriers and the
// latency of the DMA. So (1) the fragments are double buffered by chunk, not by K-step: F0 = chunk q
// (MFMAs 0, 1), F1 = chunk 4 + q (MFMAs 2, 3), 32 VGPRs each, and each set is read under the 32 MFMAs
// of the other; (2) at the middle of tile t the whole of tile t is in registers, so its buffer is free
// there and ONE barrier per K-tile does both jobs (everyone read tile t, everyone's pieces of tile
// t + 1 landed); (3) the ring is three stages of 48 KiB = 144 KiB of the 160 KiB: LDS is free because
// the registers already hold the kernel to one workgroup per CU, and with three stages tile t + 3 is
// issued at the middle of tile t and first read at the middle of tile t + 2, so a DMA has two K-tiles
// (16384 cycles per SIMD) to land while a two-stage ring would give it one. Per K-tile t (buffer
// t % 3; F0 of tile t was read at the middle of tile t - 1):
//     8 ds_read_b128       F1 <- tile t, chunk 4 + q
//     32 MFMA on F0        MFMAs 0, 1
//     s_waitcnt lgkmcnt(0) F1 landed: this wave has finished reading buffer t % 3
//     s_waitcnt vmcnt(6)   own pieces of tile t + 1 landed; tile t + 2 (6 glds16) stays in flight
//     s_barrier            everyone's pieces of tile t + 1 landed, everyone finished buffer t % 3
//     stage(t + 3) -> buffer t % 3
//     8 ds_read_b128       F0 <- tile t + 1, chunk q
//     32 MFMA on F1        MFMAs 2, 3
//     s_waitcnt lgkmcnt(0)
// The vmcnt wait is counted: it is 0 only when tile t + 1 is the last one. The barrier is skipped on
// the last tile. Every lgkmcnt wait follows 32 MFMAs issued after the reads it waits for.
//
// As in i8_kernels.hip the schedule is held by empty asm statements (pin_acc) and fenced s_waitcnt
// builtins; re-inspect the .s (--save-temps) after any change: the loop has exactly the waits of the
// table, vmcnt(6) / vmcnt(0) before the barrier and none added by the compiler, 32 MFMAs between
// s_setprio 1 / 0, ScratchSize 0.
//
// Tile order: xcd_remap + grouped_tile (8-row bands). Epilogue: register j of acc[m][n] is row
// 16m + 4j + (lane >> 4), col 16n + (lane & 15) of the wave tile; global_store_dwordx2, 16 lanes
// = one 128-B line per row.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage, gfx950): 201 VGPRs, 144 KiB LDS, no
// AGPRs, no scratch, no spills; occupancy 2 waves per SIMD = one workgroup per CU.
// gemm_f64_check_kernel: 76 VGPRs, 66080 B LDS, no scratch. hashed_fill_f64_kernel: 24 VGPRs.
// ---------------------------------------------------------------------------------------
namespace f64 {
constexpr int BM = 256, BN = 128, BK = 16, THREADS = 512;
constexpr int ROW = BK * 8;                      // 128 B
constexpr int A_BYTES = BM * ROW;                // 32 KiB
constexpr int B_BYTES = BN * ROW;                // 16 KiB
constexpr int STAGE_BYTES = A_BYTES + B_BYTES;   // 48 KiB
constexpr int RING = 3;
constexpr int CHECK_MAX_K = 256;                 // the dense check: 2 KiB rows, as the bf16 check's
}  // namespace f64

__global__ __launch_bounds__(f64::THREADS)
void gemm_f64_nt_kernel(const double* __restrict__ A, const double* __restrict__ Bt, double* __restrict__ C, int M,
                        int N, int K) {
  constexpr int BM = f64::BM, BN = f64::BN, ROW = f64::ROW, A_BYTES = f64::A_BYTES;
  constexpr int STAGE_BYTES = f64::STAGE_BYTES, RING_BYTES = f64::RING * STAGE_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[RING_BYTES];
  const int tiles_n = N / BN;
  const int nwg = (M / BM) * tiles_n;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, nwg), M / BM, tiles_n, 8, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  // staging: this lane's byte offset into an operand panel, and the uniform 64-row step between its
  // pieces. Uniform running pointers of the next tile to stage and of its ring slot.
  const int srow = tid >> 3, schunk = (tid & 7) ^ ((srow >> 1) & 7);
  const size_t kbytes = (size_t)K * 8;
  const size_t soff = (size_t)srow * kbytes + schunk * 16;
  const size_t sstep = 64 * kbytes;
  const char* ga = reinterpret_cast<const char*>(A) + (size_t)tm * BM * kbytes;
  const char* gb = reinterpret_cast<const char*>(Bt) + (size_t)tn * BN * kbytes;
  char* const wave_dst = smem + wave * 1024;
  int stage_off = 0;
  auto stage = [&]() {
    char* dst = wave_dst + stage_off;
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(ga + j * sstep + soff, dst + j * 8192);
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(gb + j * sstep + soff, dst + A_BYTES + j * 8192);
    ga += ROW;
    gb += ROW;
    stage_off = stage_off + STAGE_BYTES == RING_BYTES ? 0 : stage_off + STAGE_BYTES;
  };
  // fragment reads: row i of a 16-row group, logical chunk 4h + q
  const int fi = lane & 15, fq = lane >> 4;
  const int pc0 = (fq ^ ((fi >> 1) & 7)) << 4;     // chunk h: pc0 ^ (h * 64)
  const int rA = (wr * 64 + fi) * ROW;                     // within the A image
  const int rB = A_BYTES + (wc * 64 + fi) * ROW;           // within the stage
  auto read_frags = [&](int off, int h, doublex2 (&af)[4], doublex2 (&bfr)[4]) {
    const char* buf = smem + off;
    const int pc = pc0 ^ (h * 64);
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = *reinterpret_cast<const doublex2*>(buf + rA + m * 16 * ROW + pc);
#pragma unroll
    for (int n = 0; n < 4; ++n) bfr[n] = *reinterpret_cast<const doublex2*>(buf + rB + n * 16 * ROW + pc);
  };

  doublex4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = doublex4{0.0, 0.0, 0.0, 0.0};
  doublex2 a0[4], b0[4], a1[4], b1[4];

  // An empty asm that "rewrites" the accumulators, so that the MFMAs of one half are not sunk below
  // the wait or barrier that follows them to join the MFMAs there (which would keep three fragment
  // sets live).
  auto pin_acc = [&]() {
#pragma unroll
    for (int m = 0; m < 4; ++m)
      asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]), "+v"(acc[m][2]), "+v"(acc[m][3]));
  };
#define F64_MFMA32(AF, BF)                                                                         \
  __builtin_amdgcn_s_setprio(1);                                                                   \
  _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                    \
  _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                    \
  _Pragma("unroll") for (int n = 0; n < 4; ++n)                                                    \
    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(AF[m][s], BF[n][s], acc[m][n], 0, 0, 0);      \
  __builtin_amdgcn_s_setprio(0);                                                                   \
  pin_acc();
  // s_waitcnt builtin (simm16: vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8]; all ones = no
  // wait) between compiler fences, as in i8_kernels.hip.
#define F64_FENCED_WAIT(IMM)             \
  asm volatile("" ::: "memory");         \
  __builtin_amdgcn_s_waitcnt(IMM);       \
  asm volatile("" ::: "memory")
#define F64_WAIT_LDS() F64_FENCED_WAIT(0xC07F)
#define F64_WAIT_VM(N) F64_FENCED_WAIT(0x0F70 | (N))

  const int nt = K / f64::BK;
  stage();
  if (nt > 1) stage();
  if (nt > 2) stage();
  if (nt > 2) {
    F64_WAIT_VM(12);
  } else if (nt > 1) {
    F64_WAIT_VM(6);
  } else {
    F64_WAIT_VM(0);
  }
  __builtin_amdgcn_s_barrier();
  read_frags(0, 0, a0, b0);
  F64_WAIT_LDS();
  int cur = 0;                                     // ring slot of tile t
  for (int t = 0; t < nt; ++t) {
    const int nxt = cur + STAGE_BYTES == RING_BYTES ? 0 : cur + STAGE_BYTES;
    read_frags(cur, 1, a1, b1);
    F64_MFMA32(a0, b0)
    F64_WAIT_LDS();                                // tile t is in registers
    if (t + 1 < nt) {
      if (t + 2 < nt) {
        F64_WAIT_VM(6);                            // tile t + 1 landed; tile t + 2 in flight
      } else {
        F64_WAIT_VM(0);
      }
      __builtin_amdgcn_s_barrier();                // tile t + 1 is in LDS; slot `cur` is free
      if (t + 3 < nt) stage();                     // tile t + 3 -> slot `cur` (stage_off == cur)
      read_frags(nxt, 0, a0, b0);
    }
    F64_MFMA32(a1, b1)
    F64_WAIT_LDS();
    cur = nxt;
  }
#undef F64_WAIT_VM
#undef F64_WAIT_LDS
#undef F64_FENCED_WAIT
#undef F64_MFMA32
  // epilogue: col = lane & 15, row = 4 * j + (lane >> 4)
  double* Cblk = C + (size_t)tm * BM * N + (size_t)tn * BN;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wr * 64 + m * 16 + 4 * j + fq;
        const int col = wc * 64 + n * 16 + fi;
        Cblk[(size_t)row * N + col] = acc[m][n][j];
      }
}

// ---------------------------------------------------------------------------------------
// Dense check of the FP64 product, the counterpart of the other four on the same staging and reduce
// (probe_kernels.hip). The fp64 reference of an element never touches the matrix pipe: v_fma_f64 on
// the VALU into two accumulators (even and odd k), 16 bytes at a time. check_finish<double> takes the
// difference in fp64 and only then narrows, so an element that is off by 2^-40 of its value is seen,
// and a product of integer-valued doubles gives d2 == 0.0f exactly. K is capped, not walked in
// chunks: a tile's rows are 8 * K bytes, and f64::CHECK_MAX_K = 256 makes them the 2 KiB rows of
// the bf16 check (66080 B of LDS); the readiness K is 128. Needs M, N % 16 == 0, K % 4 == 0 (rows
// of a multiple of 32 bytes: the pad argument of check_stage_rows), K <= 256 (host-checked).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CHECK_THREADS)
void gemm_f64_check_kernel(const double* __restrict__ A, const double* __restrict__ Bt, const double* __restrict__ C,
                           int M, int N, int K, int inject, float* __restrict__ out2) {
  __shared__ __attribute__((aligned(16))) uint8_t la[CHECK_TILE * (8 * f64::CHECK_MAX_K + 16)];
  __shared__ __attribute__((aligned(16))) uint8_t lb[CHECK_TILE * (8 * f64::CHECK_MAX_K + 16)];
  const CheckPos t(N);
  check_stage_rows(A, Bt, t, 8 * K, la, lb);
  __syncthreads();
  const uint8_t* pa = la + t.r * (8 * K + 16);
  const uint8_t* pb = lb + t.c * (8 * K + 16);
  double ref0 = 0.0, ref1 = 0.0;
  for (int kc = 0; kc < K / 2; ++kc) {
    const doublex2 a2 = *reinterpret_cast<const doublex2*>(pa + kc * 16);
    const doublex2 b2 = *reinterpret_cast<const doublex2*>(pb + kc * 16);
    ref0 = fma(a2[0], b2[0], ref0);
    ref1 = fma(a2[1], b2[1], ref1);
  }
  check_finish(C, N, t, ref0 + ref1, inject, out2);
}

// ---------------------------------------------------------------------------------------
// Hashed fp64 operand fill: finite doubles with a hashed sign, |x| in [0.5, 1) (exponent 0x3FE) and
// all 52 mantissa bits hashed. hashed_fill_kernel applies one mask pair to every dword; a double needs
// one for its high dword (sign, exponent, 20 mantissa bits) and none for its low one, hence a kernel
// of its own on the same hash and indexing. `res`, when given, is zeroed as there.
// ---------------------------------------------------------------------------------------
constexpr int FILL_F64 = FILL_KINDS;             // the `kind` of amdprobe_f8_fill, after the dword-mask kinds

__global__ __launch_bounds__(256)
void hashed_fill_f64_kernel(uint4* __restrict__ p, size_t n16, uint32_t seed, ReadinessResult* __restrict__ res) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n16; i += stride) {
    const uint64_t base = (i << 2) ^ ((uint64_t)seed << 40);
    p[i] = make_uint4(mix32(base), (mix32(base + 1) & 0x800FFFFFu) + 0x3FE00000u,
                      mix32(base + 2), (mix32(base + 3) & 0x800FFFFFu) + 0x3FE00000u);
  }
  if (tid == 0 && res != nullptr) *res = ReadinessResult{0.f, 0.f, 0ull, 0ull};
}

}  // namespace amdprobe
