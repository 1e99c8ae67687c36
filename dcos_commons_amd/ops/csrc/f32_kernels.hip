// FP32 MFMA kernels of the readiness probe (gfx950). #included after sp_kernels.hip (uses
// probe_kernels.hip's xcd_remap, grouped_tile, glds16, ReadinessResult, hashed_fill_kernel and the
// shared parts of the dense check).
//
// v_mfma_f32_32x32x2_f32, with 4-byte operands, is the single-precision multiplier array of the
// matrix pipe: every SGEMM of an fp32 training or HPC payload lands on it, and none of the other
// kernels reaches it (they feed bf16, f8, f4, int8 or fp64 operands). Its readiness mode has a bound
// of its own (gpu_health.MAX_GEMM_F32_REL_ERR): a product whose operands were squeezed through an
// 11-bit (tf32-like) path is off by 2.6e-4, which the shared 1e-3 would pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amdprobe {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// FP32 GEMM:  C[M][N] (fp32) = A[M][K] * Bt[N][K]^T, A and Bt K-contiguous floats. Every product and
// every sum is formed by v_mfma_f32_32x32x2_f32; nothing is added in software.
//
// The instruction (CDNA3 / CDNA4 ISA, matrix layout tables; pinned on the MI355X by the exact `index`
// test of tests/test_gpu_f32_ops.py, which a wrong lane, register or K pairing cannot pass, and which
// passed with the mapping written here): lane (i = lane & 31, h = lane >> 5) supplies ONE float per
// operand, A[i][h] and B[h][i] of the 32x2 and 2x32 operands. The 32x32 result is 16 floats per lane:
// register j is row 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3), column lane & 31. One instruction is
// 4096 flops; at the 157 TFLOP/s fp32 matrix peak of the part (256 CUs, 4 SIMDs, 2.4 GHz: 64 flops
// per cycle per SIMD) that is 64 cycles of the pipe per instruction for 4 operand bytes per lane and
// operand. It is used and not v_mfma_f32_16x16x4_f32 because per operand float fetched it does twice
// the flops (32 against 16 outputs per input), and its 32-row, 2-K-group operand layout is the one
// fp32-input layout that no other kernel here exercises.
//
// Work split. Block tile 256 (M) x 256 (N), K-tile 32 floats = 128-B rows. 512 threads = 8 waves as
// 2 (M) x 4 (N); wave (wr, wc) owns rows wr * 128 + [0, 128), cols wc * 64 + [0, 64) = 4 x 2 MFMA
// tiles of 32x32: 8 accumulators x 16 = 128 accumulator VGPRs. The 128 x 64 wave tile (and not
// 64 x 128) puts the four reads on the operand whose image the two wave rows split, and the two on
// the one that four wave columns split. 16 K-steps x 8 = 128 MFMAs = 8192 pipe cycles per wave per
// K-tile, two waves per SIMD. __launch_bounds__(512): one workgroup per CU.
//
// Fragments. A lane fetches 16-B chunks of its row with ds_read_b128: in pass p = 0..3 the logical
// chunk 2p + h of the 128-B row, i.e. the floats k = 8p + 4h + s, s = 0..3, of the K-tile, and feeds
// four consecutive MFMAs from the four floats it holds. A sum over K does not depend on which K
// elements one MFMA takes as long as the A and B lanes of a K-group h take the same ones (they do:
// the same chunk and the same float of their rows); only the summation order differs from
// k = 0, 1, 2, ... MFMA (p, s) consumes the K elements {8p + s, 8p + 4 + s} of the tile:
//     pass 0: {0,4} {1,5} {2,6} {3,7}        pass 1: {8,12} {9,13} {10,14} {11,15}
//     pass 2: {16,20} ... {19,23}            pass 3: {24,28} ... {27,31}
// Per wave a K-tile is 4 x (4 + 2) = 24 ds_read_b128 for 128 MFMAs, not one ds_read_b32 per operand
// and MFMA.
//
// LDS image: 128-B rows unpadded, 16-B chunk c of tile row r stored at chunk c ^ ((r >> 1) & 7).
// Conflict freedom, derived for this read (four floats per chunk, 32-row groups, 2 K-groups): a
// ds_read_b128 is served 16 lanes at a time (16 x 16 B = all 64 banks once). h = lane >> 5 is
// constant over each 32 lanes and one read instruction has one p, so the 16 lanes of a service group
// ask for the SAME logical chunk c = 2p + h, of the 16 rows i = 16g .. 16g + 15 (g = 0, 1) of a
// fragment group that starts at a multiple of 32 rows, hence (r >> 1) & 7 == (i >> 1) & 7. The 256-B
// bank window holds two rows: even rows fall in its first half, odd rows in its second. Among the 8
// rows of one parity in a run of 16, (i >> 1) & 7 takes each value once and x -> c ^ x is a bijection
// for any fixed c, so the 8 lanes of a parity hit the 8 distinct 16-B slots of their half: 16 lanes,
// 16 distinct slots, every bank once. That holds for each of the four service groups of the wave.
//
// Staging. global_load_lds_dwordx4 (glds16) writes LDS lane-linearly, so the permutation is applied
// to the lane's global SOURCE address: slot p = j * 512 + tid of an operand image (row p >> 3 =
// j * 64 + (tid >> 3), physical chunk p & 7 = tid & 7) is fed from logical chunk (tid & 7) ^
// ((row >> 1) & 7); j * 64 rows does not change (row >> 1) & 7, so a lane has one offset per operand
// stride. 8 glds16 per thread per K-tile: 4 for the 32 KiB of A, 4 for the 32 KiB of Bt.
//
// Schedule. A K-tile is 8192 matrix-pipe cycles per wave and 16384 per SIMD, against 24
// ds_read_b128 per wave: LDS traffic is nothing against matrix time, and what is left to hide is the
// barrier and the latency of the DMA. (1) The fragment sets are double buffered by pass: F0 holds
// passes 0 and 2, F1 passes 1 and 3, 24 VGPRs each, and each set is read under the 32 MFMAs of the
// pass before it. (2) A stage is 64 KiB, so the ring is two stages = 128 KiB of the 160 KiB; three
// do not fit. After the reads of pass 3 the whole of tile t is in registers and its buffer is free,
// so ONE barrier per K-tile does both jobs (everyone read tile t, everyone's pieces of tile t + 1
// landed), and tile t + 2 is issued into buffer t % 2 right after it. A DMA is issued at the barrier
// of tile t and first needed at the barrier of tile t + 1: a whole K-tile of matrix time (16384
// cycles per SIMD) to land. Per K-tile t (buffer t % 2; F0 of pass 0 was read under pass 3 of tile
// t - 1):
//     6 ds_read_b128       F1 <- tile t, pass 1
//     32 MFMA on F0        pass 0
//     s_waitcnt lgkmcnt(0)
//     6 ds_read_b128       F0 <- tile t, pass 2
//     32 MFMA on F1        pass 1
//     s_waitcnt lgkmcnt(0)
//     6 ds_read_b128       F1 <- tile t, pass 3
//     32 MFMA on F0        pass 2
//     s_waitcnt lgkmcnt(0) F1 landed: this wave has finished reading buffer t % 2
//     s_waitcnt vmcnt(0)   own pieces of tile t + 1 landed (nothing newer is in flight)
//     s_barrier            everyone's pieces of tile t + 1 landed, everyone finished buffer t % 2
//     stage(t + 2) -> buffer t % 2
//     6 ds_read_b128       F0 <- tile t + 1, pass 0
//     32 MFMA on F1        pass 3
//     s_waitcnt lgkmcnt(0)
// The loop's one vmcnt wait is vmcnt(0): with whole stages in a ring of two, the tile waited for is
// the only one in flight at the barrier, so there is nothing to count past. The prologue has the one
// counted wait, vmcnt(8) (tile 0 landed, the 8 glds16 of tile 1 in flight). A ring of half-stages as
// in sp_kernels.hip, which would let the loop's wait be counted, was not built and not measured. The
// barrier is skipped on the last tile. Every lgkmcnt wait follows 32 MFMAs issued after the reads it
// waits for.
//
// As in f64_kernels.hip the schedule is held by empty asm statements (pin_acc) and fenced s_waitcnt
// builtins; re-inspect the .s (--save-temps) after any change: the loop has exactly the waits of the
// table, vmcnt(0) before the barrier and none added by the compiler, 32 MFMAs between
// s_setprio 1 / 0, ScratchSize 0.
//
// Tile order: xcd_remap + grouped_tile (8-row bands). Epilogue: register j of acc[m][n] is row
// 32m + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3), col 32n + (lane & 31) of the wave tile;
// global_store_dword, 32 lanes = one 128-B line per row.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage, gfx950): 189 VGPRs, 128 KiB LDS, no
// AGPRs, no scratch, no spills; occupancy 2 waves per SIMD = one workgroup per CU. The 128 x 64 wave
// tile fits; the 64 x 64 fallback geometry was not needed. gemm_f32_check_kernel: 74 VGPRs, 66080 B
// LDS, no scratch.
// ---------------------------------------------------------------------------------------
namespace f32 {
constexpr int BM = 256, BN = 256, BK = 32, THREADS = 512;
constexpr int ROW = BK * 4;                      // 128 B
constexpr int A_BYTES = BM * ROW;                // 32 KiB
constexpr int B_BYTES = BN * ROW;                // 32 KiB
constexpr int STAGE_BYTES = A_BYTES + B_BYTES;   // 64 KiB
constexpr int RING = 2;
constexpr int CHECK_MAX_K = 512;                 // the dense check: 2 KiB rows, as the bf16 check's
}  // namespace f32

__global__ __launch_bounds__(f32::THREADS)
void gemm_f32_nt_kernel(const float* __restrict__ A, const float* __restrict__ Bt, float* __restrict__ C, int M,
                        int N, int K) {
  constexpr int BM = f32::BM, BN = f32::BN, ROW = f32::ROW, A_BYTES = f32::A_BYTES;
  constexpr int STAGE_BYTES = f32::STAGE_BYTES, RING_BYTES = f32::RING * STAGE_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[RING_BYTES];
  const int tiles_n = N / BN;
  const int nwg = (M / BM) * tiles_n;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, nwg), M / BM, tiles_n, 8, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  // staging: this lane's byte offset into an operand panel, and the uniform 64-row step between its
  // pieces. Uniform running pointers of the next tile to stage and of its ring slot.
  const int srow = tid >> 3, schunk = (tid & 7) ^ ((srow >> 1) & 7);
  const size_t kbytes = (size_t)K * 4;
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
    for (int j = 0; j < 4; ++j) glds16(gb + j * sstep + soff, dst + A_BYTES + j * 8192);
    ga += ROW;
    gb += ROW;
    stage_off ^= STAGE_BYTES;
  };
  // fragment reads: row i of a 32-row group, logical chunk 2p + h
  const int fi = lane & 31, fh = lane >> 5;
  const int pc0 = (fh ^ ((fi >> 1) & 7)) << 4;     // pass p: pc0 ^ (p * 32)
  const int rA = (wr * 128 + fi) * ROW;                    // within the A image
  const int rB = A_BYTES + (wc * 64 + fi) * ROW;           // within the stage
  auto read_frags = [&](int off, int p, f32x4 (&af)[4], f32x4 (&bfr)[2]) {
    const char* buf = smem + off;
    const int pc = pc0 ^ (p * 32);
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = *reinterpret_cast<const f32x4*>(buf + rA + m * 32 * ROW + pc);
#pragma unroll
    for (int n = 0; n < 2; ++n) bfr[n] = *reinterpret_cast<const f32x4*>(buf + rB + n * 32 * ROW + pc);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[m][n][j] = 0.f;
  f32x4 a0[4], b0[2], a1[4], b1[2];

  // An empty asm that "rewrites" the accumulators, so that the MFMAs of one pass are not sunk below
  // the wait or barrier that follows them to join the MFMAs there (which would keep three fragment
  // sets live).
  auto pin_acc = [&]() {
#pragma unroll
    for (int m = 0; m < 4; ++m) asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]));
  };
#define F32_MFMA32(AF, BF)                                                                         \
  __builtin_amdgcn_s_setprio(1);                                                                   \
  _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                    \
  _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                    \
  _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                    \
    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(AF[m][s], BF[n][s], acc[m][n], 0, 0, 0);      \
  __builtin_amdgcn_s_setprio(0);                                                                   \
  pin_acc();
  // s_waitcnt builtin (simm16: vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8]; all ones = no
  // wait) between compiler fences, as in f64_kernels.hip.
#define F32_FENCED_WAIT(IMM)             \
  asm volatile("" ::: "memory");         \
  __builtin_amdgcn_s_waitcnt(IMM);       \
  asm volatile("" ::: "memory")
#define F32_WAIT_LDS() F32_FENCED_WAIT(0xC07F)
#define F32_WAIT_VM(N) F32_FENCED_WAIT(0x0F70 | (N))

  const int nt = K / f32::BK;
  stage();
  if (nt > 1) {
    stage();
    F32_WAIT_VM(8);                                // tile 0 landed; tile 1 in flight
  } else {
    F32_WAIT_VM(0);
  }
  __builtin_amdgcn_s_barrier();
  read_frags(0, 0, a0, b0);
  F32_WAIT_LDS();
  int cur = 0;                                     // ring slot of tile t
  for (int t = 0; t < nt; ++t) {
    read_frags(cur, 1, a1, b1);
    F32_MFMA32(a0, b0)
    F32_WAIT_LDS();
    read_frags(cur, 2, a0, b0);
    F32_MFMA32(a1, b1)
    F32_WAIT_LDS();
    read_frags(cur, 3, a1, b1);
    F32_MFMA32(a0, b0)
    F32_WAIT_LDS();                                // tile t is in registers
    if (t + 1 < nt) {
      F32_WAIT_VM(0);                              // own pieces of tile t + 1 landed
      __builtin_amdgcn_s_barrier();                // tile t + 1 is in LDS; slot `cur` is free
      if (t + 2 < nt) stage();                     // tile t + 2 -> slot `cur` (stage_off == cur)
      read_frags(cur ^ STAGE_BYTES, 0, a0, b0);
    }
    F32_MFMA32(a1, b1)
    F32_WAIT_LDS();
    cur ^= STAGE_BYTES;
  }
#undef F32_WAIT_VM
#undef F32_WAIT_LDS
#undef F32_FENCED_WAIT
#undef F32_MFMA32
  // epilogue: col = lane & 31, row = 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)
  float* Cblk = C + (size_t)tm * BM * N + (size_t)tn * BN;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = wr * 128 + m * 32 + 8 * (j >> 2) + 4 * fh + (j & 3);
        const int col = wc * 64 + n * 32 + fi;
        Cblk[(size_t)row * N + col] = acc[m][n][j];
      }
}

// ---------------------------------------------------------------------------------------
// Dense check of the FP32 product, the counterpart of the other five on the same staging and reduce
// (probe_kernels.hip). The fp32 reference of an element never touches the matrix pipe: v_fma_f32 on
// the VALU into two accumulators (even and odd k), 16 bytes at a time. A product of integer-valued
// floats whose partial sums stay below 2^24 gives d2 == 0.0f exactly. K is capped, not walked in
// chunks: a tile's rows are 4 * K bytes, and f32::CHECK_MAX_K = 512 makes them the 2 KiB rows of the
// bf16 check (66080 B of LDS); the readiness K is 128. Needs M, N % 16 == 0, K % 8 == 0 (rows of a
// multiple of 32 bytes: the pad argument of check_stage_rows), K <= 512 (host-checked).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CHECK_THREADS)
void gemm_f32_check_kernel(const float* __restrict__ A, const float* __restrict__ Bt, const float* __restrict__ C,
                           int M, int N, int K, int inject, float* __restrict__ out2) {
  __shared__ __attribute__((aligned(16))) uint8_t la[CHECK_TILE * (4 * f32::CHECK_MAX_K + 16)];
  __shared__ __attribute__((aligned(16))) uint8_t lb[CHECK_TILE * (4 * f32::CHECK_MAX_K + 16)];
  const CheckPos t(N);
  check_stage_rows(A, Bt, t, 4 * K, la, lb);
  __syncthreads();
  const uint8_t* pa = la + t.r * (4 * K + 16);
  const uint8_t* pb = lb + t.c * (4 * K + 16);
  float ref0 = 0.f, ref1 = 0.f;
  for (int kc = 0; kc < K / 4; ++kc) {
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(pa + kc * 16);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(pb + kc * 16);
    ref0 = __builtin_fmaf(a4[0], b4[0], ref0);
    ref1 = __builtin_fmaf(a4[1], b4[1], ref1);
    ref0 = __builtin_fmaf(a4[2], b4[2], ref0);
    ref1 = __builtin_fmaf(a4[3], b4[3], ref1);
  }
  check_finish(C, N, t, ref0 + ref1, inject, out2);
}

// Hashed fp32 operand fill: hashed_fill_kernel with the dword pair below, i.e. finite floats with a
// hashed sign, exponent 126 (|x| in [0.5, 1)) and all 23 mantissa bits hashed. The launcher in
// probe_api.hip passes the pair; there is no fill kernel of its own.
constexpr int FILL_F32 = FILL_META24 + 1;        // the `kind` of amdprobe_f8_fill, after meta24
constexpr uint32_t FILL_F32_AND = 0x807FFFFFu, FILL_F32_ADD = 0x3F000000u;

}  // namespace amdprobe
