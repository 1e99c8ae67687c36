// 2:4 structured-sparsity MFMA kernels of the readiness probe (gfx950). #included after f64_kernels.hip
// (uses probe_kernels.hip's xcd_remap, grouped_tile, glds16, mix32, bf16x8, floatx4 and ReadinessResult).
//
// v_smfmac_f32_16x16x64_bf16 is the one data path of the matrix pipe that no dense kernel reaches: a
// per-lane index register drives a 2-of-4 operand mux in front of the multipliers. Pruned-weight
// inference runs on it, and a device whose index decode or mux is broken passes every dense check.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amdprobe {

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// Sparse GEMM:  C[M][N] (fp32) = A[M][K] * Bt[N][K]^T with A 2:4 sparse along K and stored compressed:
//   vals[M][K/2] bf16   group g (dense k = 4g .. 4g + 3) of a row owns values 2g, 2g + 1: its first and
//                       second kept element in increasing k
//   meta[M][K/8] uint8  byte j = group 2j in bits 3:0, group 2j + 1 in bits 7:4; in a nibble bits 1:0
//                       are the position of the first kept element, bits 3:2 of the second
//   Bt[N][K]     bf16   dense
// Every product and every sum is formed by v_smfmac_f32_16x16x64_bf16; nothing is added in software.
//
// The instruction, as found on an MI355X (one non-zero per A row against Bt[n][k] = k + 1 reads the
// pairing off the product; the exact `index` tests of tests/test_gpu_sp_ops.py pin it). Lane (i = lane
// & 15, q = lane >> 4) supplies 8 compressed values of A row i (4 VGPRs), 16 dense values of B column i
// (8 VGPRs) and an index register. Call kk = 0..63 the K of one instruction.
//   A: compressed value j of lane group q stands for one of kk = 16q + 4 * (j >> 1) + {0, 1, 2, 3}, the
//      one its two index bits [2j + 1 : 2j] name: a lane group holds 16 CONSECUTIVE kk.
//   B: slot t of lane group q is kk = 8q + t for t < 8 and kk = 32 + 8q + (t - 8) for t >= 8: two runs
//      of 8, 32 apart, the operand of two dense 16x16x32 MFMAs side by side.
// So a compressed value is NOT multiplied by a B slot of its own lane group, as one might expect: the
// values 0..3 / 4..7 of A lane group q meet slots of B lane group (2q) & 3 / (2q + 1) & 3, in its first
// run for q < 2 and its second for q >= 2. 16-bit sources at this K depth consume 16 index bits, and
// abid (with cbsz 0) selects the low (0) or high (1) half of the index register. The 16x16 fp32 result
// has the layout of the dense 16x16 MFMAs: register j of a lane is row 4 * (lane >> 4) + j, column
// lane & 15. With the storage format above the metadata needs no translation: nibble t of a lane's 16
// bits is the nibble of its group t, and bits [2j + 1 : 2j] are the position of compressed value j.
//
// K mapping. K-tile = 128 dense k = two instruction K-steps s = 0, 1. A lane group q owns dense
// k in [32q, 32q + 32) of the tile, and step s the half [32q + 16s, 32q + 16s + 16) of it, which is
// kk = 16q .. 16q + 15 of that step: the 16 B vals[row][64T + 16q + 8s ..+8] and the 16 index bits of
// the groups 8q + 4s .. 8q + 4s + 3. The metadata of both steps of a lane is therefore ONE dword,
// meta[row][16T + 4q .. 4q + 3], and step s is selected with abid:s. B follows from the two tables:
// kk -> dense k = 32 * (kk >> 4) + 16s + (kk & 15), so the first run of B lane group q is the 16 B of
// Bt at byte 64 * (q >> 1) + 32s + 16 * (q & 1) of the tile's 256-B row and the second run the 16 B
// 128 further on.
//
// Work split. Block tile 256 (M) x 128 (N): per K-tile a block reads 256 x 128 B of vals and
// 128 x 256 B of Bt, 32 KiB each, which is the balanced point of the lopsided traffic (A is half
// width, so the tile is twice as tall as wide). 512 threads = 8 waves as 4 (M) x 2 (N); wave (wr, wc)
// owns rows wr * 64 + [0, 64), cols wc * 64 + [0, 64) = 4 x 4 tiles of 16x16: 16 accumulators x 4 = 64
// accumulator VGPRs, 16 SMFMACs per K-step. __launch_bounds__(512): one workgroup per CU, two waves
// per SIMD.
//
// LDS image. The unit of staging is a HALF-stage h = 2T + s: everything K-step s of K-tile T needs.
//   A half   256 rows x 64 B:  logical chunk q (16 B) of row r = vals bytes [128T + 32q + 16s, + 16)
//            stored at chunk q ^ ((r >> 2) & 3)
//   B half   128 rows x 128 B: logical chunk c = 2g + e = Bt bytes [256T + 64g + 32s + 16e, + 16),
//            the step-s half of A lane group g's dense k; stored at chunk c ^ ((r >> 1) & 7). The two
//            runs of B lane group q are the logical chunks q and 4 + q.
//   meta     256 rows x 16 B (even half-stages only): meta[row][16T .. 16T + 15], unswizzled
// = 16 + 16 + 4 KiB = 36 KiB per half-stage, ring of 4 half-stages = SP_RING (2) K-tiles = 144 KiB.
// Splitting the K-tile by step is what buys the ring depth: whole K-tiles of 64 KiB would give a ring
// of two and one K-tile of DMA cover; half-stages give four buffers and three half-steps of cover.
// Conflict freedom. A ds_read_b128 is served 16 lanes at a time; 16 consecutive lanes have one q and
// the rows i = 0..15 of a fragment group that starts at a multiple of 16 rows.
//   B half (128-B rows): the f8 / f64 argument as it stands. The 16 lanes ask for one logical chunk c
//   (q or 4 + q, one per instruction); the 256-B bank window holds two rows, even rows in its first
//   half; among the 8 rows of one parity (i >> 1) & 7 takes each value once and x -> c ^ x is a
//   bijection, so 16 lanes hit 16 distinct 16-B slots.
//   A half (64-B rows), derived here: the bank window holds FOUR rows, row i in quarter i & 3. The 4
//   rows of one quarter have (i >> 2) & 3 = 0, 1, 2, 3, and x -> q ^ x is a bijection on 0..3, so they
//   hit the 4 distinct slots of their quarter: 16 lanes, 16 distinct slots, every bank once.
//   meta: one ds_read_b32 per fragment group, byte address 16 * i + 4 * q = dword 4i + q: 64 lanes,
//   64 consecutive dwords.
//
// How metadata reaches the lanes: through LDS, with the operands. It is 16 B per row per K-tile, one
// eighth of the A bytes, and rides the same DMA as one more glds16 per thread per K-tile; a lane then
// needs one ds_read_b32 per fragment group per K-tile (4 per wave against 24 ds_read_b128). The
// alternative, a global_load_dword per fragment group a tile ahead, moves the same 4 KiB but as 16
// scattered 16-B pieces per wave instruction, puts VGPR loads into the vmcnt stream of the DMA (the
// counted waits below would depend on where the compiler schedules them) and holds a third register
// set; its latency is the DMA's. The 4 KiB region has 256 slots for 512 threads: waves w and w + 4
// write the same 16 B to the same slot, so that every wave issues the same number of DMAs and one
// count serves all.
//
// Staging. global_load_lds_dwordx4 (glds16) writes LDS lane-linearly, so the permutations are applied
// to the lane's global SOURCE address. A half: slot p = j * 512 + tid is row p >> 2 = j * 128 +
// (tid >> 2), physical chunk tid & 3, fed from logical chunk (tid & 3) ^ ((row >> 2) & 3). B half:
// slot p is row j * 64 + (tid >> 3), physical chunk tid & 7, fed from logical chunk c = (tid & 7) ^
// ((row >> 1) & 7), i.e. Bt byte 64 * (c >> 1) + 32s + 16 * (c & 1). j * 128 and j * 64 rows change
// neither swizzle term, so a lane has one offset per operand. 4 glds16 per thread per half-stage,
// plus the metadata one on even half-stages.
//
// Schedule. One SMFMAC is 32768 dense-equivalent flops; a K-step is 16 of them per wave against 4 + 8
// ds_read_b128 (12 KiB per wave, 96 KiB per CU per K-step: LDS is the busiest unit here, B is read
// at full width for a pipe that runs at the sparse rate). Fragments are double buffered by K-step:
// F0 = step 0 (A 16 + B 32 VGPRs), F1 = step 1, each read under the 16 SMFMACs of the other. Per
// half-step h (buffer h & 3; F[h & 1] was read during half-step h - 1):
//     12 ds_read_b128 (+ 4 ds_read_b32 when h is odd)   F[(h + 1) & 1] <- half-stage h + 1
//     16 SMFMAC on F[h & 1], abid = h & 1
//     s_waitcnt lgkmcnt(0)   this wave has finished reading buffer (h + 1) & 3
//     s_waitcnt vmcnt(9)     own pieces of half-stage h + 2 landed; h + 3 and h + 4 (4 + 5 DMAs, one
//                            of the two is even) stay in flight
//     s_barrier              everyone's pieces of h + 2 landed, everyone finished buffer (h + 1) & 3
//     stage(h + 5) -> buffer (h + 1) & 3
// written below as one loop iteration per K-tile (even half-step, then odd). The vmcnt wait is counted;
// near the end it is 4 (even h, K-tile T + 2 does not exist) or 0. A DMA issued at the end of
// half-step h is first needed at the barrier of half-step h + 3.
//
// The schedule is held as in f64_kernels.hip by empty asm statements (pin_acc) and fenced s_waitcnt
// builtins; re-inspect the .s (--save-temps) after any change.
//
// Tile order: xcd_remap + grouped_tile (8-row bands). Epilogue: register j of acc[m][n] is row
// 16m + 4 * (lane >> 4) + j, col 16n + (lane & 15) of the wave tile; plain global_store_dword.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage, gfx950): 183 VGPRs, 144 KiB LDS, no
// AGPRs, no scratch, no spills; occupancy 2 waves per SIMD = one workgroup per CU. In the .s the loop
// has 12 + 12 ds_read_b128 and one ds_read2st64_b32 pair per K-tile, two runs of 16 SMFMACs between
// s_setprio 1 / 0 (the second with abid:1), lgkmcnt(0) after each, vmcnt(9) / vmcnt(4) / vmcnt(0)
// before the barriers and no wait added by the compiler. sp24_expand_kernel: 16 VGPRs;
// hashed_fill_meta24_kernel: 40 VGPRs; no scratch.
//
// Measured on an MI355X (scripts/gemm_sp_bench.py, profiles/gemm_sp.md; 2 * M * N * K dense-equivalent
// flops): 1054 TFLOP/s median at 4096^3, 1103 at 8192^3, 0.78x / 0.76x the dense gemm_bf16_nt_256_kernel
// on the expanded A in the same run (1347 / 1461). It multiplies half the terms and is still the
// slower of the two: a barrier every 16 SMFMACs and full-width B fragments for a 64x64 wave tile are
// what the code shows; which of them costs was not measured.
// ---------------------------------------------------------------------------------------
namespace sp {
constexpr int BM = 256, BN = 128, BK = 128, THREADS = 512;
constexpr int A_HALF = BM * 64;                  // 16 KiB: one K-step of compressed A
constexpr int B_HALF = BN * 128;                 // 16 KiB: one K-step of Bt
constexpr int META_BYTES = BM * 16;              // 4 KiB: the metadata of one K-tile
constexpr int BUF_BYTES = A_HALF + B_HALF + META_BYTES;   // 36 KiB, one half-stage
constexpr int RING = 2;                          // K-tiles in the ring = 4 half-stages
constexpr int RING_BYTES = 2 * RING * BUF_BYTES; // 144 KiB
}  // namespace sp

__global__ __launch_bounds__(sp::THREADS)
void gemm_sp_bf16_nt_kernel(const __bf16* __restrict__ vals, const uint8_t* __restrict__ meta,
                            const __bf16* __restrict__ Bt, float* __restrict__ C, int M, int N, int K) {
  constexpr int BM = sp::BM, BN = sp::BN, A_HALF = sp::A_HALF, B_HALF = sp::B_HALF;
  constexpr int BUF_BYTES = sp::BUF_BYTES, RING_BYTES = sp::RING_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[RING_BYTES];
  const int tiles_n = N / BN;
  const int nwg = (M / BM) * tiles_n;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, nwg), M / BM, tiles_n, 8, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  // staging: this lane's byte offsets into the three panels and the uniform row steps between its two
  // pieces of an operand half. Uniform running pointers of the next half-stage and of its ring slot.
  const size_t abytes = (size_t)K, bbytes = 2 * (size_t)K, mbytes = (size_t)(K >> 3);   // row pitches
  const int arow = tid >> 2, aq = (tid & 3) ^ ((arow >> 2) & 3);
  const size_t aoff = (size_t)arow * abytes + aq * 32;
  const int brow = tid >> 3, bc = (tid & 7) ^ ((brow >> 1) & 7);
  const size_t boff = (size_t)brow * bbytes + (bc >> 1) * 64 + (bc & 1) * 16;
  const size_t moff = (size_t)(tid & 255) * mbytes;
  const size_t astep = 128 * abytes, bstep = 64 * bbytes;
  const char* ga = reinterpret_cast<const char*>(vals) + (size_t)tm * BM * abytes;
  const char* gb = reinterpret_cast<const char*>(Bt) + (size_t)tn * BN * bbytes;
  const char* gm = reinterpret_cast<const char*>(meta) + (size_t)tm * BM * mbytes;
  char* const wave_dst = smem + wave * 1024;
  char* const meta_dst = smem + A_HALF + B_HALF + (wave & 3) * 1024;
  int stage_off = 0;
  auto stage = [&](int s) {                        // s: the K-step of the half-stage, known at every call
    char* dst = wave_dst + stage_off;
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(ga + j * astep + aoff, dst + j * 8192);
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(gb + j * bstep + boff, dst + A_HALF + j * 8192);
    if (s == 0) {
      glds16(gm + moff, meta_dst + stage_off);
      gm += 16;
    }
    ga += s == 0 ? 16 : 112;
    gb += s == 0 ? 32 : 224;
    stage_off = stage_off + BUF_BYTES == RING_BYTES ? 0 : stage_off + BUF_BYTES;
  };
  // fragment reads: row i of a 16-row group; A logical chunk q, B logical chunks q and 4 + q
  const int fi = lane & 15, fq = lane >> 4;
  const int rA = (wr * 64 + fi) * 64 + ((fq ^ ((fi >> 2) & 3)) << 4);
  const int rB = A_HALF + (wc * 64 + fi) * 128 + ((fq ^ ((fi >> 1) & 7)) << 4);         // chunk 4 + q: ^ 64
  const int rM = A_HALF + B_HALF + (wr * 64 + fi) * 16 + fq * 4;
  auto read_frags = [&](int off, bf16x8 (&af)[4], bf16x16 (&bfr)[4]) {
    const char* buf = smem + off;
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = *reinterpret_cast<const bf16x8*>(buf + rA + m * 16 * 64);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const bf16x8 lo = *reinterpret_cast<const bf16x8*>(buf + rB + n * 16 * 128);
      const bf16x8 hi = *reinterpret_cast<const bf16x8*>(buf + (rB ^ 64) + n * 16 * 128);
      bfr[n] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    }
  };
  auto read_meta = [&](int off, int (&mt)[4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) mt[m] = *reinterpret_cast<const int*>(smem + off + rM + m * 16 * 16);
  };
  auto next_buf = [&](int off) { return off + BUF_BYTES == RING_BYTES ? 0 : off + BUF_BYTES; };

  floatx4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
  bf16x8 a0[4], a1[4];
  bf16x16 b0[4], b1[4];
  int mt[4], mt_n[4];

  // An empty asm that "rewrites" the accumulators, so that the SMFMACs of one K-step are not sunk below
  // the wait or barrier that follows them to join the SMFMACs there.
  auto pin_acc = [&]() {
#pragma unroll
    for (int m = 0; m < 4; ++m)
      asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]), "+v"(acc[m][2]), "+v"(acc[m][3]));
  };
#define SP_SMFMAC16(AF, BF, ABID)                                                                  \
  __builtin_amdgcn_s_setprio(1);                                                                   \
  _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                    \
  _Pragma("unroll") for (int n = 0; n < 4; ++n)                                                    \
    acc[m][n] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(AF[m], BF[n], acc[m][n], mt[m], 0, ABID); \
  __builtin_amdgcn_s_setprio(0);                                                                   \
  pin_acc();
  // s_waitcnt builtin (simm16: vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8]; all ones = no
  // wait) between compiler fences, as in f64_kernels.hip.
#define SP_FENCED_WAIT(IMM)              \
  asm volatile("" ::: "memory");         \
  __builtin_amdgcn_s_waitcnt(IMM);       \
  asm volatile("" ::: "memory")
#define SP_WAIT_LDS() SP_FENCED_WAIT(0xC07F)
#define SP_WAIT_VM(N) SP_FENCED_WAIT(0x0F70 | (N))

  const int nt = K / sp::BK;
  // prologue: half-stages 0..3 (5 + 4 + 5 + 4 DMAs); F0 and the metadata of K-tile 0; half-stage 4
  stage(0);
  stage(1);
  if (nt > 1) {
    stage(0);
    stage(1);
    SP_WAIT_VM(13);
  } else {
    SP_WAIT_VM(4);
  }
  __builtin_amdgcn_s_barrier();
  read_frags(0, a0, b0);
  read_meta(0, mt);
  SP_WAIT_LDS();
  if (nt > 1) {
    SP_WAIT_VM(9);
  } else {
    SP_WAIT_VM(0);
  }
  __builtin_amdgcn_s_barrier();                    // half-stage 1 is in LDS; buffer 0 is free
  if (nt > 2) stage(0);                            // half-stage 4 -> buffer 0
  int cur = 0;                                     // ring slot of half-stage 2T
  for (int T = 0; T < nt; ++T) {
    const int odd = next_buf(cur), nxt = next_buf(odd);
    // half-step 2T
    read_frags(odd, a1, b1);
    SP_SMFMAC16(a0, b0, 0)
    SP_WAIT_LDS();                                 // K-tile T is in registers
    if (T + 1 < nt) {
      if (T + 2 < nt) {
        SP_WAIT_VM(9);                             // half-stage 2T + 2 landed; 2T + 3, 2T + 4 in flight
        __builtin_amdgcn_s_barrier();
        stage(1);                                  // half-stage 2T + 5 -> slot `odd`
      } else {
        SP_WAIT_VM(4);                             // 2T + 3 in flight
        __builtin_amdgcn_s_barrier();
      }
      read_frags(nxt, a0, b0);
      read_meta(nxt, mt_n);
    }
    // half-step 2T + 1
    SP_SMFMAC16(a1, b1, 1)
    SP_WAIT_LDS();
    if (T + 1 < nt) {
#pragma unroll
      for (int m = 0; m < 4; ++m) mt[m] = mt_n[m];
      if (T + 2 < nt) {
        SP_WAIT_VM(9);                             // half-stage 2T + 3 landed; 2T + 4, 2T + 5 in flight
      } else {
        SP_WAIT_VM(0);
      }
      __builtin_amdgcn_s_barrier();                // slot `nxt` is free
      if (T + 3 < nt) stage(0);                    // half-stage 2T + 6 -> slot `nxt`
    }
    cur = nxt;
  }
#undef SP_WAIT_VM
#undef SP_WAIT_LDS
#undef SP_FENCED_WAIT
#undef SP_SMFMAC16
  // epilogue: col = lane & 15, row = 4 * (lane >> 4) + j
  float* Cblk = C + (size_t)tm * BM * N + (size_t)tn * BN;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wr * 64 + m * 16 + 4 * fq + j;
        const int col = wc * 64 + n * 16 + fi;
        Cblk[(size_t)row * N + col] = acc[m][n][j];
      }
}

// ---------------------------------------------------------------------------------------
// Expansion of a compressed A to the dense bf16 A[M][K] (VALU only). It is what lets gemm_check_kernel,
// the fp32 VALU check of the dense bf16 path, serve as the reference of the sparse product: neither
// the expansion nor the check touches the matrix pipe. One thread per metadata byte: two groups =
// 8 B of vals in, 16 B of A out, built with 64-bit shifts (a kept element at position p of its group
// is the group's 64-bit word's bits [16p + 15 : 16p]). An illegal nibble with first == second ORs two
// values into one element; nothing is read or written out of bounds for any nibble.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void sp24_expand_kernel(const uint2* __restrict__ vals, const uint8_t* __restrict__ meta, uint4* __restrict__ A,
                        size_t nbytes_meta) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes_meta; i += stride) {
    const uint2 v = vals[i];
    const uint32_t mb = meta[i];
    const uint64_t g0 = ((uint64_t)(v.x & 0xFFFFu) << (16 * (mb & 3))) | ((uint64_t)(v.x >> 16) << (16 * ((mb >> 2) & 3)));
    const uint64_t g1 = ((uint64_t)(v.y & 0xFFFFu) << (16 * ((mb >> 4) & 3))) | ((uint64_t)(v.y >> 16) << (16 * (mb >> 6)));
    A[i] = make_uint4((uint32_t)g0, (uint32_t)(g0 >> 32), (uint32_t)g1, (uint32_t)(g1 >> 32));
  }
}

// ---------------------------------------------------------------------------------------
// Hashed 2:4 metadata fill: every nibble is one of the six legal codes (first < second): 4 = (0, 1),
// 8 = (0, 2), 12 = (0, 3), 9 = (1, 2), 13 = (1, 3), 14 = (2, 3). The AND / ADD masks of
// hashed_fill_kernel cannot produce that set, hence a kernel of its own on the same hash and indexing:
// nibble t of a dword takes the 4 hash bits [4t + 3 : 4t], x, and becomes code (6 * x) >> 4 of the
// table (the codes 0, 2, 3, 5 get 3 of the 16 values of x, the codes 1 and 4 get 2). `res`, when
// given, is zeroed as there.
// ---------------------------------------------------------------------------------------
constexpr int FILL_META24 = FILL_F64 + 1;        // the `kind` of amdprobe_f8_fill, after fp64

__device__ __forceinline__ uint32_t meta24_word(uint32_t h) {
  uint32_t w = 0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const uint32_t code = (6u * ((h >> (4 * t)) & 15u)) >> 4;
    w |= ((0xED9C84u >> (4 * code)) & 15u) << (4 * t);
  }
  return w;
}

__global__ __launch_bounds__(256)
void hashed_fill_meta24_kernel(uint4* __restrict__ p, size_t n16, uint32_t seed, ReadinessResult* __restrict__ res) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n16; i += stride) {
    const uint64_t base = (i << 2) ^ ((uint64_t)seed << 40);
    p[i] = make_uint4(meta24_word(mix32(base)), meta24_word(mix32(base + 1)), meta24_word(mix32(base + 2)),
                      meta24_word(mix32(base + 3)));
  }
  if (tid == 0 && res != nullptr) *res = ReadinessResult{0.f, 0.f, 0ull, 0ull};
}

}  // namespace amdprobe
