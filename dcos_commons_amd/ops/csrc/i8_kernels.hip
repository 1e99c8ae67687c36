// INT8 MFMA kernels of the readiness probe (gfx950). #included after f4_kernels.hip (uses
// f8_kernels.hip's intx4 and probe_kernels.hip's xcd_remap, grouped_tile, glds16 and the shared parts
// of the dense check).
//
// The integer MFMAs (v_mfma_i32_32x32x32_i8, v_mfma_i32_16x16x64_i8) and their int32 accumulators are a
// data path of the matrix pipe that none of the float kernels reaches; W8A8 inference runs on it. It is
// also the one matrix path whose result is exact for any operands, so its check passes on == 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amdprobe {

typedef int intx16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// INT8 GEMM:  C[M][N] (int32) = A[M][K] * Bt[N][K]^T, A and Bt K-contiguous int8. The accumulate is
// the instruction's wrapping int32 one and nothing is added in software; the host rejects K > 65536,
// and |a * b| <= 2^14, so no sum reaches 2^31.
//
// MFMA shape: 32x32x32, not 16x16x64. Both take one 16-B fragment per lane and operand, i.e. 2 x 1 KiB
// of LDS reads per MFMA, but the 32x32x32 does 32 * 32 * 32 = 32768 MACs with them and the 16x16x64
// does 16 * 16 * 64 = 16384: per MAC the 32x32 shape needs half the LDS fragment bytes. (No other GEMM
// here uses a 32x32 MFMA; only the register-only mfma_peak loop does.)
//
// Work split. Block tile 256x256, K-tile 128 bytes = four K-steps of 32. 512 threads = 8 waves as
// 2 (M) x 4 (N); wave (wr, wc) owns rows wr*128 + [0,128), cols wc*64 + [0,64) = 4 x 2 MFMA tiles of
// 32x32: 8 accumulators x 16 VGPRs = 128 accumulator VGPRs, 4 K-steps x 8 = 32 MFMAs per wave per
// K-tile. __launch_bounds__(512): two waves per SIMD, one workgroup per CU.
//
// Fragments. Lane (i = lane & 31, h = lane >> 5) supplies row (column) i of a 32-row group and the 16
// K bytes [32s + 16h, 32s + 16h + 16) of K-step s: logical 16-B chunk 2s + h of the 128-B row, ONE
// ds_read_b128 = 4 VGPRs per fragment. An integer dot product does not change under a permutation
// of K, so which 16 bytes a lane takes is free as long as the A and B lanes of one K-group h take the
// same bytes (they do: the same chunk of their rows). What the exact test pins is the row / column of
// each lane and the accumulator layout. A K-step needs 4 A + 2 B fragments (24 VGPRs); they are double
// buffered in registers (F0 = even steps, F1 = odd), so the LDS reads of step s + 1 run under the 8
// MFMAs of step s. Per CU and K-step: 8 waves x 6 KiB = 48 KiB of LDS reads against 2 waves x 8 MFMAs
// of 16 passes per SIMD.
//
// LDS image: as the f8 / f4 kernels, 128-B rows unpadded, 16-B chunk c of tile row r stored at chunk
// c ^ ((r >> 1) & 7). Conflict freedom, re-derived for this fragment: a ds_read_b128 is served 16
// lanes at a time (16 x 16 B = all 64 banks once). A group of 16 consecutive lanes has one h (h
// changes at lane 32) and in one read instruction one s, so all 16 lanes ask for the SAME logical
// chunk c = 2s + h, of 16 consecutive rows: i = 0..15 or 16..31 of a fragment group that starts at a
// multiple of 32 rows, hence (r >> 1) & 7 == (i >> 1) & 7. The 256-B bank window holds two rows: even
// rows fall in its first half, odd rows in its second. Among the 8 rows of one parity (i >> 1) & 7
// takes each value once (for i in 16..31 too: bit 4 of i is dropped by the & 7), and x -> c ^ x is a
// bijection for any fixed c, so those 8 lanes hit the 8 distinct 16-B slots of their half: 16 lanes,
// 16 distinct slots, every bank once. This is the f8 argument with "lane group = one q" replaced by
// "lane group = one h and one half of the 32 rows"; it never uses which c.
//
// Staging. global_load_lds_dwordx4 (glds16) writes LDS lane-linearly, so the permutation is applied
// to the lane's global SOURCE address: slot p = j * 512 + tid (row p >> 3, physical chunk p & 7) is fed
// from logical chunk (p & 7) ^ ((row >> 1) & 7). 8 glds16 per thread per K-tile (4 A + 4 B), issued as
// scalar base + one 32-bit lane offset (j * 64 rows does not change (row >> 1) & 7).
//
// Ring: two stages of 32 KiB A + 32 KiB B = 128 KiB of the 160 KiB; a third does not fit. Per K-tile t
// (buffer t & 1; F0 of step 0 was read at the end of tile t - 1):
//     6 ds_read_b128   F1 <- step 1;   8 MFMA on F0 (step 0);   s_waitcnt lgkmcnt(0)
//     6 ds_read_b128   F0 <- step 2;   8 MFMA on F1 (step 1);   s_waitcnt lgkmcnt(0)
//     6 ds_read_b128   F1 <- step 3;   8 MFMA on F0 (step 2);   s_waitcnt lgkmcnt(0)
//     s_barrier                        everyone finished reading buffer t & 1
//     stage(t + 2) -> buffer t & 1     8 glds16
//     s_waitcnt vmcnt(8)               own pieces of tile t + 1 landed; tile t + 2 stays in flight
//     s_barrier                        everyone's pieces of tile t + 1 landed
//     6 ds_read_b128   F0 <- tile t + 1, step 0
//     8 MFMA on F1 (step 3);           s_waitcnt lgkmcnt(0)
// Every lgkmcnt wait follows 8 MFMAs (8 x 16 passes) issued after the reads it waits for. The vmcnt
// wait is counted: it is 0 only when tile t + 1 is the last one (nothing left to stage), so a whole
// K-tile stays in flight behind the one consumed.
//
// As in f4_kernels.hip the schedule is held by empty asm statements (pin_acc, the lane-offset asm in
// stage) and fenced s_waitcnt builtins; re-inspect the .s (--save-temps) after any change: the loop
// has exactly the waits of the table, vmcnt(8) after the 8 glds16 and vmcnt(0) only on the path
// without a stage, 8 MFMAs between s_setprio 1 / 0, ScratchSize 0.
//
// Tile order: xcd_remap + grouped_tile (8-row bands). Epilogue: 32x32 accumulator layout, register j
// of a lane is row 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3), col lane & 31; plain global_store_dword.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage, gfx950): 189 VGPRs, 128 KiB LDS, no
// AGPRs, no scratch, no spills; occupancy 2 waves per SIMD = one workgroup per CU.
// gemm_i8_check_kernel: 74 VGPRs, 33312 B LDS, no scratch.
// ---------------------------------------------------------------------------------------
namespace i8 {
constexpr int BM = 256, BN = 256, BK = 128, THREADS = 512;
constexpr int OPER_BYTES = BM * BK;              // 32 KiB, one operand tile
constexpr int RING = 2;
constexpr int MAX_K = 65536;
}  // namespace i8

__global__ __launch_bounds__(i8::THREADS)
void gemm_i8_nt_kernel(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt, int* __restrict__ C, int M, int N,
                       int K) {
  constexpr int BM = i8::BM, BN = i8::BN, ROW = i8::BK, OPER_BYTES = i8::OPER_BYTES;
  constexpr int BUF_BYTES = 2 * OPER_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[i8::RING * BUF_BYTES];
  const int tiles_n = N / BN;
  const int nwg = (M / BM) * tiles_n;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, nwg), M / BM, tiles_n, 8, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  // staging: slot p = j * 512 + tid of an operand tile image is row j * 64 + (tid >> 3); this lane's
  // four pieces share one lane offset and differ by the uniform 64 * K. Uniform running pointers of
  // the next tile to stage.
  const int srow = tid >> 3, schunk = (tid & 7) ^ ((srow >> 1) & 7);
  const uint32_t soff = (uint32_t)srow * K + schunk * 16;
  const size_t sstep = (size_t)64 * K;
  const int8_t* ga = A + (size_t)tm * BM * K;
  const int8_t* gb = Bt + (size_t)tn * BN * K;
  char* const wave_dst = smem + wave * 1024;
  int staged = 0;
  auto stage = [&]() {
    char* dst = wave_dst + (staged & 1) * BUF_BYTES;
    // the empty asm keeps the 32 -> 64-bit extension of the lane offset next to its use
    uint32_t o = soff;
    asm volatile("" : "+v"(o));
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(ga + j * sstep + o, dst + j * 8192);
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(gb + j * sstep + o, dst + OPER_BYTES + j * 8192);
    ga += ROW;
    gb += ROW;
    ++staged;
  };
  // fragment reads: row i of a 32-row group, logical chunk 2s + h
  const int fi = lane & 31, fh = lane >> 5;
  const int pc0 = (fh ^ ((fi >> 1) & 7)) << 4;     // K-step s: pc0 ^ (s * 32)
  const int rA = (wr * 128 + fi) * ROW;                    // within the A tile
  const int rB = OPER_BYTES + (wc * 64 + fi) * ROW;        // within the buffer
  auto read_frags = [&](int t, int s, intx4 (&af)[4], intx4 (&bfr)[2]) {
    const char* buf = smem + (t & 1) * BUF_BYTES;
    const int pc = pc0 ^ (s * 32);
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = *reinterpret_cast<const intx4*>(buf + rA + m * 32 * ROW + pc);
#pragma unroll
    for (int n = 0; n < 2; ++n) bfr[n] = *reinterpret_cast<const intx4*>(buf + rB + n * 32 * ROW + pc);
  };

  intx16 acc[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[m][n][j] = 0;
  intx4 a0[4], b0[2], a1[4], b1[2];

  // An empty asm that "rewrites" the accumulators, so that the MFMAs of one K-step are not sunk below
  // the next step's wait or barrier to join the MFMAs there (which would keep three fragment sets live).
  auto pin_acc = [&]() {
#pragma unroll
    for (int m = 0; m < 4; ++m) asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]));
  };
#define I8_MFMA8(AF, BF)                                                                           \
  __builtin_amdgcn_s_setprio(1);                                                                   \
  _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                    \
  _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                    \
    acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AF[m], BF[n], acc[m][n], 0, 0, 0);           \
  __builtin_amdgcn_s_setprio(0);                                                                   \
  pin_acc();
  // s_waitcnt builtin (simm16: vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8]; all ones = no
  // wait) between compiler fences, as in f4_kernels.hip: the compiler's own wait insertion sees them.
#define I8_FENCED_WAIT(IMM)              \
  asm volatile("" ::: "memory");         \
  __builtin_amdgcn_s_waitcnt(IMM);       \
  asm volatile("" ::: "memory")
#define I8_WAIT_LDS() I8_FENCED_WAIT(0xC07F)
#define I8_WAIT_VM(N) I8_FENCED_WAIT(0x0F70 | (N))

  const int nt = K / i8::BK;
  stage();
  if (nt > 1) {
    stage();
    I8_WAIT_VM(8);
  } else {
    I8_WAIT_VM(0);
  }
  __builtin_amdgcn_s_barrier();
  read_frags(0, 0, a0, b0);
  I8_WAIT_LDS();
  for (int t = 0; t < nt; ++t) {
    read_frags(t, 1, a1, b1);
    I8_MFMA8(a0, b0)
    I8_WAIT_LDS();
    read_frags(t, 2, a0, b0);
    I8_MFMA8(a1, b1)
    I8_WAIT_LDS();
    read_frags(t, 3, a1, b1);
    I8_MFMA8(a0, b0)
    I8_WAIT_LDS();
    __builtin_amdgcn_s_barrier();                  // buffer t & 1 is free
    if (t + 2 < nt) {
      stage();
      I8_WAIT_VM(8);                               // tile t + 1 landed; tile t + 2 in flight
    } else {
      I8_WAIT_VM(0);
    }
    if (t + 1 < nt) {
      __builtin_amdgcn_s_barrier();                // tile t + 1 is in LDS
      read_frags(t + 1, 0, a0, b0);
    }
    I8_MFMA8(a1, b1)
    I8_WAIT_LDS();
  }
#undef I8_WAIT_VM
#undef I8_WAIT_LDS
#undef I8_FENCED_WAIT
#undef I8_MFMA8
  // epilogue: col = lane & 31, row = 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)
  int* Cblk = C + (size_t)tm * BM * N + (size_t)tn * BN;
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
// Dense check of the INT8 product, the counterpart of the other three on the same staging and reduce
// (probe_kernels.hip). The int32 reference of an element never touches the matrix pipe: v_dot4c_i32_i8
// on the VALU, 16 bytes at a time. check_finish<int> takes the difference in integers and only then
// converts, so a healthy product gives d2 == 0.0f exactly; ref itself is exact in fp32 up to 2^24
// (K <= 1024: |ref| <= 2^24). Needs M, N % 16 == 0, K % 16 == 0, K <= CHECK_MAX_K (host-checked).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CHECK_THREADS)
void gemm_i8_check_kernel(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt, const int* __restrict__ C,
                          int M, int N, int K, int inject, float* __restrict__ out2) {
  __shared__ __attribute__((aligned(16))) uint8_t la[CHECK_TILE * (CHECK_MAX_K + 16)];
  __shared__ __attribute__((aligned(16))) uint8_t lb[CHECK_TILE * (CHECK_MAX_K + 16)];
  const CheckPos t(N);
  check_stage_rows(A, Bt, t, K, la, lb);
  __syncthreads();
  const uint8_t* pa = la + t.r * (K + 16);
  const uint8_t* pb = lb + t.c * (K + 16);
  int ref0 = 0, ref1 = 0;
  for (int kc = 0; kc < K / 16; ++kc) {
    const intx4 a4 = *reinterpret_cast<const intx4*>(pa + kc * 16);
    const intx4 b4 = *reinterpret_cast<const intx4*>(pb + kc * 16);
    ref0 = __builtin_amdgcn_sdot4(a4[0], b4[0], ref0, false);
    ref1 = __builtin_amdgcn_sdot4(a4[1], b4[1], ref1, false);
    ref0 = __builtin_amdgcn_sdot4(a4[2], b4[2], ref0, false);
    ref1 = __builtin_amdgcn_sdot4(a4[3], b4[3], ref1, false);
  }
  check_finish(C, N, t, ref0 + ref1, inject, out2);
}

}  // namespace amdprobe
