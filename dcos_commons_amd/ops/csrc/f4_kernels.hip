// FP4 / MXFP4 MFMA kernels of the readiness probe (gfx950). #included after f8_kernels.hip (uses its
// intx4 / intx8, glds4 and probe_kernels.hip's floatx4, xcd_remap, grouped_tile, glds16 and the
// shared parts of the dense check).
//
// FP4 (OCP E2M1, with E8M0 block scales "MXFP4") goes through a part of the f8f6f4 operand path that
// the FP8 kernels never reach: format select cbsz:4 blgp:4, 16 bytes (four VGPRs, 32 packed nibbles)
// per lane and operand instead of 32, and half the FP8 issue cycles.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amdprobe {

// ---------------------------------------------------------------------------------------
// FP4 GEMM:  C[M][N] (fp32) = A[M][K] * Bt[N][K]^T. A and Bt are K-contiguous packed E2M1, two
// elements per byte, element 2j of a row in bits 3:0 of byte j (the OCP MX packing,
// torch.float4_e2m1fn_x2); a row is K/2 bytes. MX = true adds E8M0 block scales sa[M][K/32],
// sb[N][K/32] (value 2^(s - 127) per 32 K elements) which go to the scale inputs of
// v_mfma_scale_f32_16x16x128_f8f6f4; nothing is pre-multiplied. MX = false passes constant-zero
// scales (the unscaled v_mfma_f32_16x16x128_f8f6f4 ... cbsz:4 blgp:4).
//
// Work split. Block tile 256x256, K-tile 256 elements = 128-B rows = two 128-element MFMA substeps
// h = 0, 1. 512 threads = 8 waves as 2 (M) x 4 (N); wave (wr, wc) owns rows wr*128 + [0,128), cols
// wc*64 + [0,64) = 8 x 4 MFMA 16x16 tiles, 128 accumulator VGPRs. One workgroup per CU, two waves
// per SIMD.
//
// LDS bytes per MFMA. A substep needs 8 A + 4 B fragments for 32 MFMAs, each fragment ONE
// ds_read_b128 (16 B per lane): 12 KiB per wave per 32 MFMAs = 384 B per MFMA. The f8 kernel's
// 64x64 wave tile reads 8 fragments of two ds_read_b128 each per 16 MFMAs = 1024 B per MFMA, and
// its MFMA takes twice the cycles: per matrix-pipe cycle this kernel asks LDS for 0.75x the f8
// kernel's bytes (0.75x the fragments per MFMA, half the bytes per fragment, half the cycles). Per
// CU and K-tile: 8 waves x 24 reads x 1 KiB = 192 KiB of LDS reads against 2 waves x 64 MFMAs per
// SIMD.
//
// Fragments. Lane (i = lane & 15, q = lane >> 4) supplies row i of a 16-row group and the 32 K
// elements [128h + 32q, 128h + 32q + 32) of substep h: logical 16-B chunk 4h + q of the 128-B row,
// element k of the 32 in VGPR k / 8, bits 4 * (k % 8). So a lane holds exactly 32-element scale
// block q of the substep (unlike FP8, where a lane's bytes are halves of two blocks).
//
// LDS image: as the f8 kernel, 128-B rows unpadded, 16-B chunk c of tile row r stored at chunk
// c ^ ((r >> 1) & 7). Conflict freedom (argument in f8_kernels.hip): one ds_read_b128 is served 16
// lanes at a time, those 16 lanes read ONE logical chunk of rows i = 0..15, and x -> c ^ x spreads
// the 8 rows of each parity over the 8 slots of their half of the 256-B bank window, for any c.
//
// Staging. global_load_lds_dwordx4 writes LDS lane-linearly, so the permutation is applied to the
// lane's global SOURCE address: slot p = j * 512 + tid (row p >> 3, physical chunk p & 7) is fed
// from logical chunk (p & 7) ^ ((row >> 1) & 7). 8 glds16 per thread per K-tile (4 A + 4 B), issued
// as scalar base + one 32-bit lane offset.
//
// Scales (a deviation from LDS-DMA, for VGPRs). The scale of row i, block j of a substep is taken
// from lane i + 16j: lane (i, q) supplies block q, the block its own data is in (this and the
// fragment layout above are what the ISA text led to expect; the exact MX test confirmed both on
// MI355X). The MFMA selects one byte of a scale VGPR with opsel, so four tiles share a dword, byte
// m & 3 = tile m: two dwords for A's 8 m-tiles, one for B, per substep. A DMA of the [row][8] bytes
// (which would also need two dword loads per thread: 512 rows x 8 blocks = 1024 dwords per K-tile)
// leaves that packing to 12 ds_read_u8 and 9 VALU ops per substep whose temporaries do not fit next
// to 128 accumulators and two fragment sets (measured: 8 to 58 VGPRs spilled). Instead thread t
// loads the 4 block scales of A row t >> 1 and of B row t >> 1 (half t & 1) into two VGPRs and
// writes them TRANSPOSED, row 64g + 16e + i, block b -> byte ((16g + i) * 8 + b) * 4 + e, so that a
// lane gets each packed dword with one ds_read_b32 and no VALU work. 8 ds_write_b8 per thread per
// K-tile; the 2 x 4 KiB scale image sits behind the operand ring.
//
// Ring: two stages of 32 KiB A + 32 KiB B (+ 4 KiB scales) = 136 KiB of the 160 KiB; a third stage
// does not fit. Fragments are double buffered in registers by substep (F0 = h 0, F1 = h 1; 48
// VGPRs each), so the LDS reads of one substep run under the 32 MFMAs of the other. Per K-tile t
// (buffer t & 1; F0 of tile t was read at the end of tile t - 1):
//     (MX) 2 global_load_dword            scale registers <- tile t + 2
//     12 ds_read_b128 (+ 3 ds_read_b32)   F1 <- tile t, h = 1
//     32 MFMA on F0
//     s_waitcnt lgkmcnt(0); s_barrier     everyone finished reading buffer t & 1
//     stage(t + 2) -> buffer t & 1        8 glds16
//     s_waitcnt vmcnt(8)                  own pieces of tile t + 1 (and the scale registers, which are
//                                         operands of this wait) landed; tile t + 2 stays in flight
//     (MX) 8 ds_write_b8                  tile t + 2's scales -> scale image t & 1
//     s_barrier                           everyone's pieces of tile t + 1 landed
//     12 ds_read_b128 (+ 3 ds_read_b32)   F0 <- tile t + 1, h = 0
//     32 MFMA on F1
//     s_waitcnt lgkmcnt(0)                free (F0 was issued 32 MFMAs ago); see F4_WAIT_LDS
// The vmcnt wait is counted: it is 0 only when tile t + 1 is the last one (nothing left to stage),
// so a whole K-tile stays in flight behind the one consumed. The prologue issues scale loads and
// stage() of tile 0, waits vmcnt(8) for the scales, then the same for tile 1 (that second vmcnt(8)
// also retires tile 0).
//
// What the compiler is trusted with, and what to re-inspect in the .s (--save-temps) after ANY
// change to this kernel or to the toolchain. The schedule is held by empty or one-instruction asm
// statements (pin_acc, the lane-offset asm in stage / load_scales, the fenced wait builtins,
// F4_WAIT_SCALES); they steer this compiler's scheduler and wait insertion, they are not a contract.
//   1. Between each `global_load_dword vX` of load_scales and the `s_waitcnt vmcnt(8)` that names
//      vX, no instruction reads or copies vX (no v_mov, no v_lshrrev): the hardware does not
//      interlock on a pending VMEM result and the compiler does not know it is pending.
//   2. The loop has exactly the vmcnt waits of the table above, vmcnt(8) after the 8 glds16 and
//      vmcnt(0) only on the path without a stage; none inserted by the compiler.
//   3. No s_waitcnt between the F1 reads and the first MFMA on F0 in the loop header, and 32 MFMAs
//      between s_setprio 1 / 0 on both sides of the barriers.
//   4. ScratchSize 0 and the VGPR counts below.
//
// Tile order: xcd_remap + grouped_tile (8-row bands). Epilogue: 16x16 accumulator layout, row
// (lane >> 4) * 4 + j, col lane & 15.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage, gfx950): unscaled 235 VGPRs, 128 KiB
// LDS; MX 248 VGPRs, 136 KiB LDS; no AGPRs, no scratch, no spills; occupancy 2 waves per SIMD = one
// workgroup per CU. gemm_f4_check_kernel: 115 VGPRs, 17.5 KiB LDS, no scratch.
// ---------------------------------------------------------------------------------------
namespace f4 {
constexpr int BM = 256, BN = 256, BK = 256, THREADS = 512;
constexpr int ROW_BYTES = BK / 2;                // 128
constexpr int OPER_BYTES = BM * ROW_BYTES;       // 32 KiB, one operand tile
constexpr int SCALE_BYTES = (BM + BN) * 8;       // 4 KiB, MX only
constexpr int RING = 2;
constexpr int FMT = 4;                           // cbsz / blgp of E2M1
}  // namespace f4

template <bool MX, int OA, int OB>
__device__ __forceinline__ floatx4 mfma_f4(intx4 a, intx4 b, floatx4 c, int sa, int sb) {
  const intx8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  if constexpr (MX)
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, f4::FMT, f4::FMT, OA, sa, OB, sb);
  else
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, f4::FMT, f4::FMT, 0, 0, 0, 0);
}

template <bool MX>
__global__ __launch_bounds__(f4::THREADS)
void gemm_f4_nt_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt, float* __restrict__ C,
                       const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb, int M, int N, int K) {
  constexpr int BM = f4::BM, BN = f4::BN, ROW = f4::ROW_BYTES, OPER_BYTES = f4::OPER_BYTES;
  constexpr int BUF_BYTES = 2 * OPER_BYTES, SC_BYTES = f4::SCALE_BYTES, SC_BASE = f4::RING * BUF_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[f4::RING * (BUF_BYTES + (MX ? SC_BYTES : 0))];
  const int tiles_n = N / BN;
  const int nwg = (M / BM) * tiles_n;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, nwg), M / BM, tiles_n, 8, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int kbytes = K >> 1;                       // bytes per operand row

  // staging: slot p = j * 512 + tid of an operand tile image is row j * 64 + (tid >> 3); j * 64 does not
  // change (row >> 1) & 7, so this lane's four pieces share one lane offset and differ by the uniform
  // 64 * kbytes. Uniform (scalar) running pointers of the next tile to stage: every DMA is issued as
  // scalar base + one 32-bit lane offset and no per-piece 64-bit lane address is kept.
  const int srow = tid >> 3, schunk = (tid & 7) ^ ((srow >> 1) & 7);
  const uint32_t soff = (uint32_t)srow * kbytes + schunk * 16;
  const size_t sstep = (size_t)64 * kbytes;
  const uint8_t* ga = A + (size_t)tm * BM * kbytes;
  const uint8_t* gb = Bt + (size_t)tn * BN * kbytes;
  char* const wave_dst = smem + wave * 1024;
  int staged = 0;
  auto stage = [&]() {
    char* dst = wave_dst + (staged & 1) * BUF_BYTES;
    // the empty asm keeps the 32 -> 64-bit extension of the lane offset next to its use (hoisted out
    // of the loop it costs a VGPR pair and the scalar-base addressing form)
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
  // MX scales, register staged: thread t loads 4 block scales (half t & 1 of the K-tile's 8) of A row
  // t >> 1 and of B row t >> 1, one lane offset on two uniform bases, and writes them transposed:
  // row r = 64g + 16e + i (quad g of four 16-row tiles, tile e), block b -> byte ((16g + i) * 8 + b) * 4 + e.
  const int kb_row = K / 32;
  const uint32_t scoff = (uint32_t)(tid >> 1) * kb_row + (tid & 1) * 4;
  const uint8_t *gsa = nullptr, *gsb = nullptr;
  if constexpr (MX) {
    gsa = sa + (size_t)tm * BM * kb_row;
    gsb = sb + (size_t)tn * BN * kb_row;
  }
  const int scr = tid >> 1;
  const int scw = (((scr >> 6) * 16 + (scr & 15)) * 8 + (tid & 1) * 4) * 4 + ((scr >> 4) & 3);
  // asm, not a C++ load: while LDS-DMA is in flight the compiler turns every wait it inserts itself
  // into vmcnt(0), which would drain the tile just staged. So the compiler does not know that the two
  // result registers are pending (the hardware has no interlock on them either): every use of them
  // goes through F4_WAIT_SCALES first, which carries them as operands.
  auto load_scales = [&](uint32_t& va, uint32_t& vb) {
    uint32_t so = scoff;
    asm volatile("" : "+v"(so));
    asm volatile("global_load_dword %0, %2, %3\n\tglobal_load_dword %1, %2, %4"
                 : "=&v"(va), "=&v"(vb) : "v"(so), "s"(gsa), "s"(gsb) : "memory");
    gsa += 8;
    gsb += 8;
  };
  auto write_scales = [&](int t, uint32_t va, uint32_t vb) {
    uint8_t* d = reinterpret_cast<uint8_t*>(smem) + SC_BASE + (t & 1) * SC_BYTES + scw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k * 4] = (uint8_t)(va >> (8 * k));
      d[BM * 8 + k * 4] = (uint8_t)(vb >> (8 * k));
    }
  };
  // fragment reads: row i of a 16-row group, logical chunk 4h + q; scales: one dword = block 4h + q of
  // row i in the four tiles of a quad (A quads 2wr, 2wr + 1; B quad wc)
  const int fi = lane & 15, fq = lane >> 4;
  const int pc0 = (fq ^ ((fi >> 1) & 7)) << 4;     // substep 1: pc0 ^ 64
  const int rA = (wr * 128 + fi) * ROW;                    // within the A tile
  const int rB = OPER_BYTES + (wc * 64 + fi) * ROW;        // within the buffer
  const int sA = SC_BASE + ((wr * 32 + fi) * 8 + fq) * 4;
  const int sB = SC_BASE + BM * 8 + ((wc * 16 + fi) * 8 + fq) * 4;
  auto read_frags = [&](int t, int h, intx4 (&af)[8], intx4 (&bfr)[4], int (&sca)[2], int& scb) {
    const char* buf = smem + (t & 1) * BUF_BYTES;
    const int pc = pc0 ^ (h * 64);
#pragma unroll
    for (int m = 0; m < 8; ++m) af[m] = *reinterpret_cast<const intx4*>(buf + rA + m * 16 * ROW + pc);
#pragma unroll
    for (int n = 0; n < 4; ++n) bfr[n] = *reinterpret_cast<const intx4*>(buf + rB + n * 16 * ROW + pc);
    sca[0] = sca[1] = scb = 0;
    if constexpr (MX) {
      const char* sc = smem + (t & 1) * SC_BYTES + h * 16;
      sca[0] = *reinterpret_cast<const int*>(sc + sA);
      sca[1] = *reinterpret_cast<const int*>(sc + sA + 16 * 8 * 4);
      scb = *reinterpret_cast<const int*>(sc + sB);
    }
  };

  floatx4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
  intx4 a0[8], b0[4], a1[8], b1[4];
  int sa0[2], sb0, sa1[2], sb1;

  // An empty asm that "rewrites" the accumulators: without it the compiler sinks the first 32 MFMAs
  // of a K-tile below the barriers to join the second 32 (their results have no earlier use), which
  // keeps both fragment sets and the next one live at once and spills.
  auto pin_acc = [&]() {
#pragma unroll
    for (int m = 0; m < 8; ++m)
      asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]), "+v"(acc[m][2]), "+v"(acc[m][3]));
  };
#define F4_ROW(AF, BF, SCA, SCB, m)                                                        \
  acc[m][0] = mfma_f4<MX, (m) & 3, 0>(AF[m], BF[0], acc[m][0], SCA[(m) >> 2], SCB);        \
  acc[m][1] = mfma_f4<MX, (m) & 3, 1>(AF[m], BF[1], acc[m][1], SCA[(m) >> 2], SCB);        \
  acc[m][2] = mfma_f4<MX, (m) & 3, 2>(AF[m], BF[2], acc[m][2], SCA[(m) >> 2], SCB);        \
  acc[m][3] = mfma_f4<MX, (m) & 3, 3>(AF[m], BF[3], acc[m][3], SCA[(m) >> 2], SCB);
#define F4_MFMA32(AF, BF, SCA, SCB)                                                        \
  __builtin_amdgcn_s_setprio(1);                                                           \
  F4_ROW(AF, BF, SCA, SCB, 0) F4_ROW(AF, BF, SCA, SCB, 1) F4_ROW(AF, BF, SCA, SCB, 2)      \
  F4_ROW(AF, BF, SCA, SCB, 3) F4_ROW(AF, BF, SCA, SCB, 4) F4_ROW(AF, BF, SCA, SCB, 5)      \
  F4_ROW(AF, BF, SCA, SCB, 6) F4_ROW(AF, BF, SCA, SCB, 7)                                  \
  __builtin_amdgcn_s_setprio(0);                                                           \
  pin_acc();
  // Waits are the s_waitcnt builtin (simm16: vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8];
  // all ones = no wait), not asm text, so the compiler's own wait insertion sees them. It loses count
  // of LDS reads that are pending across the loop's back edge and would then wait for ALL reads, the
  // F1 reads just issued included, before the first MFMA on F0, which serialises what this pipeline
  // overlaps. With nothing pending at the back edge (the F0 reads were issued 32 MFMAs earlier, so
  // that wait is free) it places no wait there at all.
#define F4_FENCED_WAIT(IMM)              \
  asm volatile("" ::: "memory");         \
  __builtin_amdgcn_s_waitcnt(IMM);       \
  asm volatile("" ::: "memory")
#define F4_WAIT_LDS() F4_FENCED_WAIT(0xC07F)
#define F4_WAIT_VM(N) F4_FENCED_WAIT(0x0F70 | (N))
  // The counted wait for the scale registers of load_scales (and whatever else is older than the N
  // newest vector-memory operations). The registers are in/out operands of the wait itself: a memory
  // clobber orders memory accesses only, and without the operands the compiler hoisted the byte
  // extraction (v_lshrrev of the register) above the wait, i.e. read a register that may not have
  // landed. With them, nothing can read the registers between the load and this instruction.
#define F4_WAIT_SCALES(N, VA, VB) asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(VA), "+v"(VB) : : "memory")

  const int nt = K / f4::BK;
  // prologue: a tile's scale loads go out just ahead of its operand DMA and are waited for with
  // that DMA (8 operations) still in flight. Each pair of scale registers has ONE wait statement and
  // is not shared with the loop: a value that feeds two waits, or the loop's registers, gets copied
  // in front of the wait, which is a read of a pending register.
  uint32_t pa0 = 0, pb0 = 0, pa1 = 0, pb1 = 0;
  if constexpr (MX) load_scales(pa0, pb0);
  stage();
  if constexpr (MX) {
    F4_WAIT_SCALES(8, pa0, pb0);
    write_scales(0, pa0, pb0);
  }
  if (nt > 1) {
    if constexpr (MX) load_scales(pa1, pb1);
    stage();
    if constexpr (MX) {
      F4_WAIT_SCALES(8, pa1, pb1);                 // tile 0 has landed too: it is older
      write_scales(1, pa1, pb1);
    } else {
      F4_WAIT_VM(8);
    }
  } else {
    F4_WAIT_VM(0);
  }
  F4_WAIT_LDS();
  __builtin_amdgcn_s_barrier();
  read_frags(0, 0, a0, b0, sa0, sb0);
  F4_WAIT_LDS();
  for (int t = 0; t < nt; ++t) {
    uint32_t sra = 0, srb = 0;                     // per iteration: loaded, waited for and written in it
    if constexpr (MX)
      if (t + 2 < nt) load_scales(sra, srb);       // tile t + 2's, written to LDS after the first barrier
    read_frags(t, 1, a1, b1, sa1, sb1);
    F4_MFMA32(a0, b0, sa0, sb0)
    F4_WAIT_LDS();
    __builtin_amdgcn_s_barrier();                  // buffer t & 1 is free
    if (t + 2 < nt) {
      stage();
      if constexpr (MX) {                          // tile t + 1 and the scale registers; tile t + 2 in flight
        F4_WAIT_SCALES(8, sra, srb);
        write_scales(t, sra, srb);
      } else {
        F4_WAIT_VM(8);
      }
    } else {
      F4_WAIT_VM(0);
    }
    if (t + 1 < nt) {
      __builtin_amdgcn_s_barrier();                // tile t + 1 is in LDS
      read_frags(t + 1, 0, a0, b0, sa0, sb0);
    }
    F4_MFMA32(a1, b1, sa1, sb1)
    F4_WAIT_LDS();                                 // free: see F4_WAIT_LDS
  }
#undef F4_WAIT_SCALES
#undef F4_WAIT_VM
#undef F4_FENCED_WAIT
#undef F4_WAIT_LDS
#undef F4_MFMA32
#undef F4_ROW
  // epilogue: col = lane & 15, row = (lane >> 4) * 4 + j
  float* Cblk = C + (size_t)tm * BM * N + (size_t)tn * BN;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wr * 128 + m * 16 + (lane >> 4) * 4 + j;
        const int col = wc * 64 + n * 16 + (lane & 15);
        Cblk[(size_t)row * N + col] = acc[m][n][j];
      }
}

// ---------------------------------------------------------------------------------------
// Dense check of the FP4 product, the counterpart of gemm_f8_check_kernel on the same staging and
// finish (probe_kernels.hip), rows of K/2 bytes. The reference never touches the matrix pipe and
// uses no FP4 conversion hardware either: every nibble is decoded with integer bit arithmetic on
// the VALU (E2M1 magnitude codes 0..7 = 0, .5, 1, 1.5, 2, 3, 4, 6; bit 3 = sign), products are
// summed with fp32 FMAs 32 elements (16 bytes) at a time, and with scales each block's partial sum
// is multiplied by 2^(sa + sb - 254) with ldexpf. Needs M, N % 16 == 0, K % 32 == 0,
// K <= CHECK_MAX_K (host-checked).
// ---------------------------------------------------------------------------------------

__device__ __forceinline__ float e2m1_decode(uint32_t code) {
  const uint32_t mag = code & 7u;
  // mag >= 2: normal, 2^((mag >> 1) - 1) * (1 + (mag & 1) / 2); mag 1 = 0.5 (the one subnormal); mag 0 = 0
  const uint32_t bits = mag >= 2u ? ((126u + (mag >> 1)) << 23) | ((mag & 1u) << 22) : (mag ? 0x3F000000u : 0u);
  return __uint_as_float(bits | ((code & 8u) << 28));
}

__global__ __launch_bounds__(CHECK_THREADS)
void gemm_f4_check_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt, const float* __restrict__ C,
                          const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb, int M, int N, int K,
                          int inject, float* __restrict__ out2) {
  __shared__ __attribute__((aligned(16))) uint8_t la[CHECK_TILE * (CHECK_MAX_K / 2 + 16)];
  __shared__ __attribute__((aligned(16))) uint8_t lb[CHECK_TILE * (CHECK_MAX_K / 2 + 16)];
  __shared__ uint8_t lsa[CHECK_TILE * (CHECK_MAX_K / 32)], lsb[CHECK_TILE * (CHECK_MAX_K / 32)];
  const CheckPos t(N);
  const int r = t.r, c = t.c;
  const int kblocks = K / 32;                  // 32 elements = one 16-B chunk = one scale block
  const bool scaled = sa != nullptr;
  check_stage_rows(A, Bt, t, K / 2, la, lb);
  if (scaled) check_stage_scales(sa, sb, t, kblocks, lsa, lsb);
  __syncthreads();
  const uint8_t* pa = la + r * (K / 2 + 16);
  const uint8_t* pb = lb + c * (K / 2 + 16);
  float ref = 0.f;
  for (int kb = 0; kb < kblocks; ++kb) {
    const uint4 a4 = *reinterpret_cast<const uint4*>(pa + kb * 16);
    const uint4 b4 = *reinterpret_cast<const uint4*>(pb + kb * 16);
    const uint32_t aw[4] = {a4.x, a4.y, a4.z, a4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        p0 = fmaf(e2m1_decode(aw[w] >> (4 * e)), e2m1_decode(bw[w] >> (4 * e)), p0);
        p1 = fmaf(e2m1_decode(aw[w] >> (4 * e + 4)), e2m1_decode(bw[w] >> (4 * e + 4)), p1);
      }
    float p = p0 + p1;
    if (scaled) p = ldexpf(p, (int)lsa[r * kblocks + kb] + (int)lsb[c * kblocks + kb] - 254);
    ref += p;
  }
  check_finish(C, N, t, ref, inject, out2);
}

}  // namespace amdprobe
