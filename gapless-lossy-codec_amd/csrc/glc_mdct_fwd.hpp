// glc_mdct_fwd.hpp — K1, the windowed forward MDCT as an exact-order SGEMM on the vector ALU.
//
//   C[m][k] = fl( fl( sum_{i ascending} fl( fl(x[m,i]*w[i]) * T[k][i] ) ) * norm )
//
// replaces the window loop (src/codec.rs:476-481) and MdctTables::mdct_block (:359-374) of the
// reference for every frame-channel row m = (frame - frame_begin)*ch + c.  M = rows, N = 1024,
// K = 2048; the K loop is strictly ascending with ONE accumulator per output, multiply and add
// are separate instructions (v_pk_mul_f32 / v_pk_add_f32, never an FMA), there is no split-K.
//
// What is in this file - exactly the kernels libglc_hip.so instantiates (launch_mdct_forward in
// glc_kernels.hip); every other shape, schedule and ablation that was measured lives in
// tools/k1_variants.hpp beside the tuning harness tools/k1_tune.hip:
//   k_mdct_fwd_st      launches of >= 4096 rows (BASELINE config 2 = 8192): a wave's lanes hold 256 ROWS
//                      (4 each) and share 8 columns, so the table values are wave-uniform and come by scalar
//                      loads straight from the table into SGPRs; the windowed samples by one ds_read_b128
//                      per i-step from a 3-slot LDS ring; 4 i-steps per fetch, a group ahead.  256x128
//                      tile / 1024 threads (one workgroup per CU, priority by distance from the barrier) or
//                      256x64 / 512 (two per CU, priority by quarter of the i loop), chosen per launch by
//                      the fill of its last round of tiles; PCM tile by dwordx4 segments when the stream has
//                      1 / 2 / 4 / 8 channels (CH), one dword per (row, sample) otherwise (CH = 0).
//   k_mdct_mix_st      the 16-wave k_mdct_fwd_st in mixed-role form, for glc_encode_range_device without a coefficient
//                      tap: exact waves on the columns below the last band, bound waves (one v_pk_fma_f32 per packed
//                      multiply-add, no coefficients stored) on the rest - the screen of DESIGN section 2 - and, where
//                      the exact columns are no whole number of waves per SIMD, hybrid waves that hold column pairs of
//                      both kinds, so that the four SIMDs issue the same number of packed operations.  With
//                      k_mdct_fwd_small_cols, the 2 x 2 short-clip kernel over a column range and only the row tiles
//                      that hold a flagged row: the exact columns of the rows that failed the screen.
//   k_mdct_mx_st       the mixed-role form with the bound on the bf16 matrix pipe, for C0 = 384 (44.1 / 48 kHz) and 1 / 2 /
//                      4 / 8 channels: 128 x 256 tile, twelve exact waves with 2 rows x 8 columns per lane (the exact
//                      kernel's chain per column), four matrix waves with 32 rows x 160 bound columns each.
//   k_mdct_fwd_small_rows  the same repair built for latency, for launches in which few rows failed: one wave per
//                      (two failed rows, 64 columns) found from the quantiser's fail counts on a fixed grid, the rows in
//                      LDS, the table streamed by dwordx4 loads 112 i-steps ahead.
//   k_mdct_fwd_dma     the kernel of rounds 2 / 3 for the same launches, now behind
//                      glc_debug_set_mdct_variant(ctx, 1): 128x128 tile, 512 threads, 4x8 outputs per lane
//                      with lanes <-> columns, both operands from LDS (table tile by LDS-DMA two stages
//                      ahead); 8-9 % slower on real samples because the chip holds less clock under it.
//   k_mdct_fwd_sched   the opening rounds of glc_encode (2048 rows each, running beside each other), as <64,128,16,4>:
//                      64x128 tile, 256 threads, ONE workgroup per CU; hand-scheduled inline-asm i-steps (step4), LDS
//                      operand prefetch, XCD-aware tile map, register staging, classic double buffer.  (Rounds 1-3:
//                      every launch of 1793..4095 rows.)
//   k_mdct_fwd_small   below 3584 rows (4096 for channel counts without a segment loader): 2x2 / 2x4 outputs per
//                      lane (<= 640 rows / above) on 32x32 / 32x64 tiles, 256 threads,
//                      hand-scheduled with a register ring of LDS operands and counted lgkmcnt waits
//                      (short clips: one wave's 2048-step chain is everything; the step is the lane tile).
//   k_mdct_fwd         the same tiling left to hipcc's scheduler: no longer instantiated by the library
//                      (round 2 used <32,64,32,4,4,4,2> for <= 512 rows); kept as the plainest statement
//                      of the loop and for tools/k1_tune.hip.
//   mac2rows           the 2-row x 8-column multiply/add block; also the entry step of D1 (k_imdct_chan).
// How every body reads its PCM tile - descriptor, row origin, loaders, tile map - is stated once, ahead of the
// kernels ("The PCM tile loader"); DESIGN section 4 has a subsection of that name: what each helper owns, which kernel
// uses which form, and what is deliberately not shared.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "glc_kernels.h"

namespace glc {
namespace k1 {

constexpr int kHopI = 1024;
constexpr int kFrameI = 2048;

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// The PCM tile loader: how every kernel of this file turns a PcmView into its A operand, stated once (DESIGN
// section 4, "The PCM tile loader", says which kernel uses which form).  `ch` is passed in the type the caller
// divides by - pcm.ch, or the kernel's compile-time channel count - so that a helper costs what its copy did.
// ------------------------------------------------------------------------------------------
// element, from pcm.p, of (frame of `row`, i = 0, channel 0): a frame's 2048 samples start half a hop before it
template <typename Row, typename Ch>
__device__ __forceinline__ long long pcm_frame_first(const PcmView &pcm, long long frame_begin, Row row, Ch ch) {
  const long long f = frame_begin + row / ch;
  return (f * kHopI - kHopI / 2 - static_cast<long long>(pcm.t0)) * ch;
}
// one past the last element present, from pcm.p: the shard's end or the stream's
template <typename Ch>
__device__ __forceinline__ long long pcm_end(const PcmView &pcm, Ch ch) {
  long long e_end = static_cast<long long>(pcm.t_count) * ch;  // shard end (elements)
  const long long n_rel = static_cast<long long>(pcm.n_samples) - static_cast<long long>(pcm.t0) * ch;
  if (e_end > n_rel) e_end = n_rel;  // stream end
  return e_end;
}
// e_cnt elements from element e_base >= 0 as a raw buffer (2^28 elements is the most a byte offset reaches)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pcm_rsrc(const PcmView &pcm, long long e_base, long long e_cnt) {
  if (e_cnt < 0) e_cnt = 0;
  if (e_cnt > (1ll << 28)) e_cnt = 1ll << 28;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pcm.p + e_base), 0, static_cast<int>(e_cnt * 4), 0x00020000);
}

// The interleaved PCM of a row tile is read through ONE buffer descriptor whose hardware range check supplies the
// encoder's zero padding (512 leading zeros, tail, shard edges).  Its base is the tile's first element, or pcm.p
// where that lies before the stream; its records end with the shard or the stream.  An element before the base
// wraps to a huge unsigned byte offset, one past the end is >= the record count: both load 0.0, so every load is
// unconditional - and so is a row >= M, which loads from kPcmNoRow.  All inputs are blockIdx / kernarg scalars.
struct PcmTile {
  __amdgpu_buffer_rsrc_t rsrc;
  long long e_base;  // the base, in elements from pcm.p
};
constexpr unsigned kPcmNoRow = 0x80000000u;  // byte offset beyond every descriptor: what a row >= M loads from
template <typename Ch>
__device__ __forceinline__ PcmTile pcm_tile(const PcmView &pcm, long long frame_begin, int m0, Ch ch) {
  const long long e_first = pcm_frame_first(pcm, frame_begin, m0, ch);  // first frame of the tile
  const long long e_end = pcm_end(pcm, ch);
  const long long e_base = e_first < 0 ? 0 : e_first;
  return PcmTile{pcm_rsrc(pcm, e_base, e_end - e_base), e_base};
}
// off = byte offset from the tile's base of (row, i = a_i), where row < M (else it stays what it was: kPcmNoRow):
// the per-row loaders, any channel count.  (The segment form is one statement on pcm_frame_first: see SegLoader.)
template <typename Ch>
__device__ __forceinline__ void pcm_row_origin(unsigned &off, const PcmView &pcm, const PcmTile &t, long long frame_begin,
                                               unsigned row, unsigned M, Ch ch, int a_i) {
  if (row < M) {
    const long long c = row % ch;
    const long long e_row = pcm_frame_first(pcm, frame_begin, row, ch) + c;
    off = static_cast<unsigned>((e_row - t.e_base + a_i * static_cast<long long>(ch)) * 4);  // may wrap: that IS the padding
  }
}

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 says which blocks share an L2).  Give XCD x the
// contiguous tile range [x T / 8, (x + 1) T / 8) in (m_tile, n_tile) order: the PCM rows of an m-tile are then
// fetched by ONE XCD instead of all eight, and the table rows of a stage are shared in that XCD's L2 by all
// resident m-tiles, which sweep i together (measured: 4x less L2 fill traffic).  Speed only, never results.
// ANY: the grid need not divide by 8 (the map is then the identity); the other launchers' grids always do.
template <bool ANY = false>
__device__ __forceinline__ unsigned xcd_tile() {
  if (ANY && gridDim.x % 8u) return blockIdx.x;
  return (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
}

// The per-row loaders: N dwords of one row, `step` bytes apart from byte offset `off`.
// Builtin form (k_mdct_fwd, k_mdct_fwd_sched, small_body): hipcc places the loads and counts them.
template <int N>
__device__ __forceinline__ void pcm_load_rows(float (&x)[N], __amdgpu_buffer_rsrc_t rsrc, unsigned off, unsigned step) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    x[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + j * step, 0, 0));
}
// Asm form (k_mdct_fwd_dma, st_body): hipcc must not count these loads or move their first use (see lds_fetch4);
// pcm_wait_rows retires them, and everything else the wave has in flight, and ties every register of x
template <int N, int R>
__device__ __forceinline__ void pcm_issue_rows(float (&x)[R], __amdgpu_buffer_rsrc_t rsrc, unsigned o, unsigned a_step) {
  static_assert((N == 4 || N == 8) && N <= R, "per-row loader shapes");
  asm volatile(
      "buffer_load_dword %0, %4, %8, 0 offen\n\t"
      "buffer_load_dword %1, %5, %8, 0 offen\n\t"
      "buffer_load_dword %2, %6, %8, 0 offen\n\t"
      "buffer_load_dword %3, %7, %8, 0 offen"
      : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3])
      : "v"(o), "v"(o + a_step), "v"(o + 2 * a_step), "v"(o + 3 * a_step), "s"(rsrc)
      : "memory");
  if constexpr (N == 8)
    asm volatile(
        "buffer_load_dword %0, %4, %8, 0 offen\n\t"
        "buffer_load_dword %1, %5, %8, 0 offen\n\t"
        "buffer_load_dword %2, %6, %8, 0 offen\n\t"
        "buffer_load_dword %3, %7, %8, 0 offen"
        : "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7])
        : "v"(o + 4 * a_step), "v"(o + 5 * a_step), "v"(o + 6 * a_step), "v"(o + 7 * a_step), "s"(rsrc)
        : "memory");
}
__device__ __forceinline__ void pcm_wait_rows(float (&x)[4]) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3])::"memory");
}
__device__ __forceinline__ void pcm_wait_rows(float (&x)[8]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])::"memory");
}

// The segment loader, for streams of CH = 1 / 2 / 4 / 8 channels (CH then divides every tile height): a stage's BK
// samples x CH channels of one frame are 4 BK CH contiguous bytes, fetched by BK / 4 * CH lanes with one dwordx4
// each - 16x fewer cache-line touches in the texture addresser than the per-row loaders - and scattered, windowed,
// into the A tile As[slot][i][row], whose rows of i are AS floats apart.  One piece per lane: k_mdct_fwd_dma and
// k_mdct_mx_st.  The kernel states `off` itself, in one statement (pcm_frame_first of the frame's first row - the
// tile's base + o, where that row is < M): behind a call here k_mdct_fwd_dma took one more SGPR and the loops of
// k_mdct_mx_st other scalar registers.  st_body (one or two pieces) keeps these rules in its own statements, for the
// reason given there.
// SOME: only the lanes constructed with `loads` load and store (wave-uniform); every lane waits.
template <int CH, int BK, int AS, bool SOME = false>
struct SegLoader {
  static_assert(CH == 1 || CH == 2 || CH == 4 || CH == 8, "segment loader shapes");
  static constexpr int kLanes = BK / 4 * CH;  // lanes per frame segment
  int fl, o;     // lane -> (frame fl of the tile, floats o .. o + 3 of its BK x CH segment)
  bool on;       // this lane loads
  unsigned off;  // byte offset of the segment's float o at i = 0, from the tile's base
  f32x4 v;

  __device__ __forceinline__ SegLoader(int tid, bool loads)
      : fl(tid / kLanes), o((tid % kLanes) * 4), on(loads), off(kPcmNoRow), v{0.f, 0.f, 0.f, 0.f} {}
  // i0_bytes: i0 x the bytes between two samples of a channel, in the form the kernel has them (asm: as pcm_issue_rows)
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsrc, unsigned i0_bytes) {
    if (SOME && !on) return;
    const unsigned o0 = off + i0_bytes;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=&v"(v) : "v"(o0), "s"(rsrc) : "memory");
  }
  __device__ __forceinline__ void wait() {  // everything this wave has in flight
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v)::"memory");
  }
  template <typename ATile, typename Window>
  __device__ __forceinline__ void store(int i0, int slot, ATile &As, const Window &Ws) {
    if (SOME && !on) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = o + j;  // float e of the segment: sample i = e / CH of channel e % CH
      const int ii = e / CH;
      As[slot][ii * AS + fl * CH + e % CH] = mul_rn(v[j], Ws[i0 + ii]);  // block[i] = slice[i]*window[i], :480
    }
  }
};

// BM x BN output tile per workgroup, BK table rows per LDS stage, TM x TN outputs per lane
// (TM, TN in {4, 8}: one or two conflict-free ds_read_b128 per operand and i-step),
// UNROLL i-steps per loop body, MINW = min waves per SIMD for the register allocator.
template <int BM, int BN, int BK, int TM, int TN, int UNROLL, int MINW>
struct Cfg {
  static constexpr int kThreads = (BM / TM) * (BN / TN);
  static constexpr int kNtx = BN / TN;
  static constexpr int kNTiles = kHopI / BN;
  static constexpr int kAPer = BM * BK / kThreads;       // A elements staged per thread
  static constexpr int kAStride = kThreads / BM;          // i distance between them
  static constexpr int kBPer = BK * BN / 4 / kThreads;    // B float4 staged per thread
  static constexpr int kBRowsPer = kThreads / (BN / 4);   // table rows covered per float4 round
  static_assert(kThreads % BM == 0 && kAPer * kAStride == BK, "A staging shape");
  static_assert(kThreads % (BN / 4) == 0 && kBPer * kBRowsPer == BK, "B staging shape");
  static_assert((TM == 4 || TM == 8) && (TN == 4 || TN == 8), "lane tile");
  static_assert((BK & (BK - 1)) == 0 && BK % UNROLL == 0, "BK");
};

template <int BM, int BN, int BK, int TM, int TN, int UNROLL, int MINW>
__global__ __launch_bounds__((BM / TM) * (BN / TN), MINW) void k_mdct_fwd(DeviceTables tb, PcmView pcm,
                                                                         long long frame_begin,
                                                                         unsigned M,
                                                                         float *__restrict__ coef) {
  using C = Cfg<BM, BN, BK, TM, TN, UNROLL, MINW>;
  // i-major tiles: As[ii][row], Bs[ii][col]; every ds_read in the inner loop is a b128 whose
  // 16 lanes of a group cover one contiguous 256-B span (conflict-free).
  __shared__ __attribute__((aligned(16))) float As[2][BK * BM];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * BN];

  const int tid = threadIdx.x;
  // blockIdx.x % kNTiles picks the coefficient tile: blocks are dealt round-robin over the 8
  // XCDs, so each XCD's L2 keeps only 1024/BN/8 panels of T (speed only, never correctness).
  const int n_tile = blockIdx.x % C::kNTiles;
  const int m_tile = blockIdx.x / C::kNTiles;
  const int m0 = m_tile * BM;
  const int n0 = n_tile * BN;
  const int tx = tid % C::kNtx, ty = tid / C::kNtx;

  // --- A operand (the PCM tile loader, above)
  const long long ch = pcm.ch;
  const PcmTile a_tile = pcm_tile(pcm, frame_begin, m0, pcm.ch);
  const __amdgpu_buffer_rsrc_t a_rsrc = a_tile.rsrc;  // (what the stage lambdas take: a_tile stays out of their captures)
  // this thread stages ONE row (r = tid % BM) and kAPer of the BK i of a stage
  const int a_r = tid % BM;
  const int a_i = tid / BM;
  unsigned a_off = kPcmNoRow;
  pcm_row_origin(a_off, pcm, a_tile, frame_begin, m0 + a_r, M, pcm.ch, a_i);
  const unsigned a_step = static_cast<unsigned>(C::kAStride * ch * 4);  // bytes between this thread's i's
  const float *w_ptr = tb.window + a_i;
  // B operand: float4 (row = idx / (BN/4), col4 = idx % (BN/4)), idx = tid + kThreads j
  const int b_r = tid / (BN / 4), b_c4 = tid % (BN / 4);
  const float *b_ptr = tb.cos_t + n0 + static_cast<size_t>(b_r) * kHopI + b_c4 * 4;

  float a_stage[C::kAPer];
  float4 b_stage[C::kBPer];

  auto load_stage = [&](int i0) {
    pcm_load_rows(a_stage, a_rsrc, a_off + static_cast<unsigned>(i0) * static_cast<unsigned>(ch * 4), a_step);
#pragma unroll
    for (int j = 0; j < C::kAPer; ++j) a_stage[j] = mul_rn(a_stage[j], w_ptr[i0 + C::kAStride * j]);  // block[i] = slice[i]*window[i], :480
#pragma unroll
    for (int j = 0; j < C::kBPer; ++j)
      b_stage[j] = *reinterpret_cast<const float4 *>(b_ptr + static_cast<size_t>(i0 + C::kBRowsPer * j) * kHopI);
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < C::kAPer; ++j) As[buf][(a_i + C::kAStride * j) * BM + a_r] = a_stage[j];
#pragma unroll
    for (int j = 0; j < C::kBPer; ++j)
      *reinterpret_cast<float4 *>(&Bs[buf][(b_r + C::kBRowsPer * j) * BN + b_c4 * 4]) = b_stage[j];
  };

  float acc[TM][TN];
#pragma unroll
  for (int r = 0; r < TM; ++r)
#pragma unroll
    for (int c = 0; c < TN; ++c) acc[r][c] = 0.0f;  // `let mut s = 0.0f32`, :365

  load_stage(0);
  store_stage(0);
  __syncthreads();

  constexpr int kStages = kFrameI / BK;
#pragma unroll 1
  for (int s = 0; s < kStages; ++s) {
    const int buf = s & 1;
    // prefetch the next stage into registers (the last iteration re-fetches stage 0 into the
    // idle buffer: keeps the loop body branch-free)
    load_stage(((s + 1) & (kStages - 1)) * BK);

    const float *Ab = As[buf] + ty * 4;
    const float *Bb = Bs[buf] + tx * 4;
#pragma unroll UNROLL
    for (int ii = 0; ii < BK; ++ii) {
      float av[TM], bv[TN];
      {
        const float4 v = *reinterpret_cast<const float4 *>(&Ab[ii * BM]);
        av[0] = v.x; av[1] = v.y; av[2] = v.z; av[3] = v.w;
      }
      if constexpr (TM == 8) {
        const float4 v = *reinterpret_cast<const float4 *>(&Ab[ii * BM + BM / 2]);
        av[4] = v.x; av[5] = v.y; av[6] = v.z; av[7] = v.w;
      }
      {
        const float4 v = *reinterpret_cast<const float4 *>(&Bb[ii * BN]);
        bv[0] = v.x; bv[1] = v.y; bv[2] = v.z; bv[3] = v.w;
      }
      if constexpr (TN == 8) {
        const float4 v = *reinterpret_cast<const float4 *>(&Bb[ii * BN + BN / 2]);
        bv[4] = v.x; bv[5] = v.y; bv[6] = v.z; bv[7] = v.w;
      }
#pragma unroll
      for (int r = 0; r < TM; ++r)
#pragma unroll
        for (int c = 0; c < TN; ++c) acc[r][c] = add_rn(acc[r][c], mul_rn(av[r], bv[c]));  // :369
    }

    store_stage(buf ^ 1);
    __syncthreads();
  }

  // epilogue: out[k] = s * norm, :372
#pragma unroll
  for (int r = 0; r < TM; ++r) {
    const unsigned row = m0 + ((r < 4) ? (ty * 4 + r) : (BM / 2 + ty * 4 + (r - 4)));
    if (row >= M) continue;
    float *dst = coef + static_cast<size_t>(row) * kHopI + n0;
    float4 o;
    o.x = mul_rn(acc[r][0], tb.norm); o.y = mul_rn(acc[r][1], tb.norm);
    o.z = mul_rn(acc[r][2], tb.norm); o.w = mul_rn(acc[r][3], tb.norm);
    *reinterpret_cast<float4 *>(dst + tx * 4) = o;
    if constexpr (TN == 8) {
      o.x = mul_rn(acc[r][4], tb.norm); o.y = mul_rn(acc[r][5], tb.norm);
      o.z = mul_rn(acc[r][6], tb.norm); o.w = mul_rn(acc[r][7], tb.norm);
      *reinterpret_cast<float4 *>(dst + BN / 2 + tx * 4) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Hand-scheduled kernels (4x8 outputs per lane).  Same arithmetic, but the instruction order
// is pinned with inline asm because hipcc (ROCm 7.2) (a) places every v_pk_add directly behind
// the v_pk_mul it depends on and (b) sinks the LDS reads of the next i-step below the current
// step's math, so a wave stalls on both.  Here each i-step issues its 6 ds_read_b64 for the NEXT
// step first, then 2 groups of {8 v_pk_mul, 8 v_pk_add} (dependent instructions 8 apart), then
// one s_waitcnt: register set X feeds even steps, set Y odd steps (ping-pong, no copies).
// ------------------------------------------------------------------------------------------
struct Operands {  // one i-step's A (4 rows) and B (8 columns) values of this lane
  f32x2 a0, a1, b0, b1, b2, b3;
};

template <int BM, int BN>
__device__ __forceinline__ void lds_fetch4(Operands &o, unsigned a_addr, unsigned b_addr, int ii) {
  // 4-row lane tile: rows ty*4 .. ty*4+3
  asm volatile(
      "ds_read_b64 %0, %6 offset:%c8\n\t"
      "ds_read_b64 %1, %6 offset:%c9\n\t"
      "ds_read_b64 %2, %7 offset:%c10\n\t"
      "ds_read_b64 %3, %7 offset:%c11\n\t"
      "ds_read_b64 %4, %7 offset:%c12\n\t"
      "ds_read_b64 %5, %7 offset:%c13"
      : "=&v"(o.a0), "=&v"(o.a1), "=&v"(o.b0), "=&v"(o.b1), "=&v"(o.b2), "=&v"(o.b3)
      : "v"(a_addr), "v"(b_addr), "i"(ii * BM * 4), "i"(ii * BM * 4 + 8), "i"(ii * BN * 4), "i"(ii * BN * 4 + 8),
        "i"(ii * BN * 4 + BN * 2), "i"(ii * BN * 4 + BN * 2 + 8)
      : "memory");
}

__device__ __forceinline__ void lds_wait4(Operands &o) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(o.a0), "+v"(o.a1), "+v"(o.b0), "+v"(o.b1), "+v"(o.b2), "+v"(o.b3)
               :
               : "memory");
}

// rows (r, r+1) x 8 columns: c[r][j] += a.lo * b_j ; c[r+1][j] += a.hi * b_j   (j = column pair)
__device__ __forceinline__ void mac2rows(f32x2 (&c0)[4], f32x2 (&c1)[4], f32x2 a, f32x2 b0, f32x2 b1,
                                         f32x2 b2, f32x2 b3) {
  f32x2 t0, t1, t2, t3, t4, t5, t6, t7;
  asm volatile(
      "v_pk_mul_f32 %8, %16, %17 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %9, %16, %18 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %10, %16, %19 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %11, %16, %20 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %12, %16, %17 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %13, %16, %18 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %14, %16, %19 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %15, %16, %20 op_sel:[1,0]\n\t"
      "v_pk_add_f32 %0, %0, %8\n\t"
      "v_pk_add_f32 %1, %1, %9\n\t"
      "v_pk_add_f32 %2, %2, %10\n\t"
      "v_pk_add_f32 %3, %3, %11\n\t"
      "v_pk_add_f32 %4, %4, %12\n\t"
      "v_pk_add_f32 %5, %5, %13\n\t"
      "v_pk_add_f32 %6, %6, %14\n\t"
      "v_pk_add_f32 %7, %7, %15"
      : "+v"(c0[0]), "+v"(c0[1]), "+v"(c0[2]), "+v"(c0[3]), "+v"(c1[0]), "+v"(c1[1]), "+v"(c1[2]), "+v"(c1[3]),
        "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7)
      : "v"(a), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
}

// One whole i-step of a 4x8 lane tile as ONE asm statement (no compiler pads between groups):
// issue the next step's six ds_read_b64 (into n), do this step's 32 multiplies and 32 adds from
// c (dependent instructions 8 apart), then wait for the reads.  r<row><colpair> = accumulators.
template <int BM, int BN, bool FETCH>
__device__ __forceinline__ void step4(f32x2 (&acc)[4][4], const Operands &c, Operands &n, unsigned a_addr,
                                      unsigned b_addr, int ii_next) {
  f32x2 t0, t1, t2, t3, t4, t5, t6, t7;
  // named operands keep the string readable: [r<row><colpair>]
  if constexpr (FETCH) {
    asm volatile(
        "ds_read_b64 %[na0], %[aa] offset:%c[oa0]\n\t"
        "ds_read_b64 %[na1], %[aa] offset:%c[oa1]\n\t"
        "ds_read_b64 %[nb0], %[ba] offset:%c[ob0]\n\t"
        "ds_read_b64 %[nb1], %[ba] offset:%c[ob1]\n\t"
        "ds_read_b64 %[nb2], %[ba] offset:%c[ob2]\n\t"
        "ds_read_b64 %[nb3], %[ba] offset:%c[ob3]\n\t"
        "v_pk_mul_f32 %[t0], %[ca0], %[cb0] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t1], %[ca0], %[cb1] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t2], %[ca0], %[cb2] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t3], %[ca0], %[cb3] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t4], %[ca0], %[cb0] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t5], %[ca0], %[cb1] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t6], %[ca0], %[cb2] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t7], %[ca0], %[cb3] op_sel:[1,0]\n\t"
        "v_pk_add_f32 %[r00], %[r00], %[t0]\n\t"
        "v_pk_add_f32 %[r01], %[r01], %[t1]\n\t"
        "v_pk_add_f32 %[r02], %[r02], %[t2]\n\t"
        "v_pk_add_f32 %[r03], %[r03], %[t3]\n\t"
        "v_pk_add_f32 %[r10], %[r10], %[t4]\n\t"
        "v_pk_add_f32 %[r11], %[r11], %[t5]\n\t"
        "v_pk_add_f32 %[r12], %[r12], %[t6]\n\t"
        "v_pk_add_f32 %[r13], %[r13], %[t7]\n\t"
        "v_pk_mul_f32 %[t0], %[ca1], %[cb0] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t1], %[ca1], %[cb1] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t2], %[ca1], %[cb2] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t3], %[ca1], %[cb3] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t4], %[ca1], %[cb0] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t5], %[ca1], %[cb1] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t6], %[ca1], %[cb2] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t7], %[ca1], %[cb3] op_sel:[1,0]\n\t"
        "v_pk_add_f32 %[r20], %[r20], %[t0]\n\t"
        "v_pk_add_f32 %[r21], %[r21], %[t1]\n\t"
        "v_pk_add_f32 %[r22], %[r22], %[t2]\n\t"
        "v_pk_add_f32 %[r23], %[r23], %[t3]\n\t"
        "v_pk_add_f32 %[r30], %[r30], %[t4]\n\t"
        "v_pk_add_f32 %[r31], %[r31], %[t5]\n\t"
        "v_pk_add_f32 %[r32], %[r32], %[t6]\n\t"
        "v_pk_add_f32 %[r33], %[r33], %[t7]\n\t"
        "s_waitcnt lgkmcnt(0)"
        : [r00] "+v"(acc[0][0]), [r01] "+v"(acc[0][1]), [r02] "+v"(acc[0][2]), [r03] "+v"(acc[0][3]),
          [r10] "+v"(acc[1][0]), [r11] "+v"(acc[1][1]), [r12] "+v"(acc[1][2]), [r13] "+v"(acc[1][3]),
          [r20] "+v"(acc[2][0]), [r21] "+v"(acc[2][1]), [r22] "+v"(acc[2][2]), [r23] "+v"(acc[2][3]),
          [r30] "+v"(acc[3][0]), [r31] "+v"(acc[3][1]), [r32] "+v"(acc[3][2]), [r33] "+v"(acc[3][3]),
          [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4), [t5] "=&v"(t5),
          [t6] "=&v"(t6), [t7] "=&v"(t7), [na0] "=&v"(n.a0), [na1] "=&v"(n.a1), [nb0] "=&v"(n.b0),
          [nb1] "=&v"(n.b1), [nb2] "=&v"(n.b2), [nb3] "=&v"(n.b3)
        : [ca0] "v"(c.a0), [ca1] "v"(c.a1), [cb0] "v"(c.b0), [cb1] "v"(c.b1), [cb2] "v"(c.b2), [cb3] "v"(c.b3),
          [aa] "v"(a_addr), [ba] "v"(b_addr), [oa0] "i"(ii_next * BM * 4), [oa1] "i"(ii_next * BM * 4 + 8),
          [ob0] "i"(ii_next * BN * 4), [ob1] "i"(ii_next * BN * 4 + 8), [ob2] "i"(ii_next * BN * 4 + BN * 2),
          [ob3] "i"(ii_next * BN * 4 + BN * 2 + 8)
        : "memory");
  } else {
    asm volatile(
        "v_pk_mul_f32 %[t0], %[ca0], %[cb0] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t1], %[ca0], %[cb1] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t2], %[ca0], %[cb2] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t3], %[ca0], %[cb3] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t4], %[ca0], %[cb0] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t5], %[ca0], %[cb1] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t6], %[ca0], %[cb2] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t7], %[ca0], %[cb3] op_sel:[1,0]\n\t"
        "v_pk_add_f32 %[r00], %[r00], %[t0]\n\t"
        "v_pk_add_f32 %[r01], %[r01], %[t1]\n\t"
        "v_pk_add_f32 %[r02], %[r02], %[t2]\n\t"
        "v_pk_add_f32 %[r03], %[r03], %[t3]\n\t"
        "v_pk_add_f32 %[r10], %[r10], %[t4]\n\t"
        "v_pk_add_f32 %[r11], %[r11], %[t5]\n\t"
        "v_pk_add_f32 %[r12], %[r12], %[t6]\n\t"
        "v_pk_add_f32 %[r13], %[r13], %[t7]\n\t"
        "v_pk_mul_f32 %[t0], %[ca1], %[cb0] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t1], %[ca1], %[cb1] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t2], %[ca1], %[cb2] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t3], %[ca1], %[cb3] op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t4], %[ca1], %[cb0] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t5], %[ca1], %[cb1] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t6], %[ca1], %[cb2] op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %[t7], %[ca1], %[cb3] op_sel:[1,0]\n\t"
        "v_pk_add_f32 %[r20], %[r20], %[t0]\n\t"
        "v_pk_add_f32 %[r21], %[r21], %[t1]\n\t"
        "v_pk_add_f32 %[r22], %[r22], %[t2]\n\t"
        "v_pk_add_f32 %[r23], %[r23], %[t3]\n\t"
        "v_pk_add_f32 %[r30], %[r30], %[t4]\n\t"
        "v_pk_add_f32 %[r31], %[r31], %[t5]\n\t"
        "v_pk_add_f32 %[r32], %[r32], %[t6]\n\t"
        "v_pk_add_f32 %[r33], %[r33], %[t7]"
        : [r00] "+v"(acc[0][0]), [r01] "+v"(acc[0][1]), [r02] "+v"(acc[0][2]), [r03] "+v"(acc[0][3]),
          [r10] "+v"(acc[1][0]), [r11] "+v"(acc[1][1]), [r12] "+v"(acc[1][2]), [r13] "+v"(acc[1][3]),
          [r20] "+v"(acc[2][0]), [r21] "+v"(acc[2][1]), [r22] "+v"(acc[2][2]), [r23] "+v"(acc[2][3]),
          [r30] "+v"(acc[3][0]), [r31] "+v"(acc[3][1]), [r32] "+v"(acc[3][2]), [r33] "+v"(acc[3][3]),
          [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4), [t5] "=&v"(t5),
          [t6] "=&v"(t6), [t7] "=&v"(t7)
        : [ca0] "v"(c.a0), [ca1] "v"(c.a1), [cb0] "v"(c.b0), [cb1] "v"(c.b1), [cb2] "v"(c.b2), [cb3] "v"(c.b3));
  }
}

// 64x128 (BM x BN) tile, 4x8 outputs per lane, register staging, two LDS slots per operand tile.
template <int BM, int BN, int BK, int MINW>
__global__ __launch_bounds__((BM / 4) * (BN / 8)) __attribute__((amdgpu_waves_per_eu(MINW, MINW)))
void k_mdct_fwd_sched(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M,
                      float *__restrict__ coef) {
  constexpr int TM = 4;
  using C = Cfg<BM, BN, BK, TM, 8, 2, MINW>;
  __shared__ __attribute__((aligned(16))) float As[2][BK * BM];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * BN];

  const int tid = threadIdx.x;
  static_assert(C::kNTiles == 8, "tile map assumes 8 coefficient tiles");
  const unsigned g = xcd_tile();
  const int n_tile = g % C::kNTiles;
  const int m_tile = g / C::kNTiles;
  const int m0 = m_tile * BM;
  const int n0 = n_tile * BN;
  const int tx = tid % C::kNtx, ty = tid / C::kNtx;

  const long long ch = pcm.ch;
  const PcmTile a_tile = pcm_tile(pcm, frame_begin, m0, pcm.ch);
  const __amdgpu_buffer_rsrc_t a_rsrc = a_tile.rsrc;  // (what the stage lambdas take: a_tile stays out of their captures)
  const int a_r = tid % BM;
  const int a_i = tid / BM;
  unsigned a_off = kPcmNoRow;
  pcm_row_origin(a_off, pcm, a_tile, frame_begin, m0 + a_r, M, pcm.ch, a_i);
  const unsigned a_step = static_cast<unsigned>(C::kAStride * ch * 4);
  const float *w_ptr = tb.window + a_i;
  const int b_r = tid / (BN / 4), b_c4 = tid % (BN / 4);
  const float *b_ptr = tb.cos_t + n0 + static_cast<size_t>(b_r) * kHopI + b_c4 * 4;

  // staging registers: raw sample and window value are multiplied only when the stage is
  // written to LDS, so the wave waits for its global loads at the END of the stage
  float a_raw[C::kAPer], a_win[C::kAPer];
  f32x4 b_stage[C::kBPer];
  auto load_stage = [&](int i0) {
    pcm_load_rows(a_raw, a_rsrc, a_off + static_cast<unsigned>(i0) * static_cast<unsigned>(ch * 4), a_step);
#pragma unroll
    for (int j = 0; j < C::kAPer; ++j) a_win[j] = w_ptr[i0 + C::kAStride * j];
#pragma unroll
    for (int j = 0; j < C::kBPer; ++j)
      b_stage[j] = *reinterpret_cast<const f32x4 *>(b_ptr + static_cast<size_t>(i0 + C::kBRowsPer * j) * kHopI);
  };
  auto store_stage = [&](int buf) {
    // pin the first use of the staged registers behind the stage's math (volatile asm
    // statements keep their order): hipcc otherwise hoists the multiply, and with it the
    // vmcnt wait, into the middle of the stage
#pragma unroll
    for (int j = 0; j < C::kAPer; ++j) {
      float r = a_raw[j], w = a_win[j];
      asm volatile("" : "+v"(r), "+v"(w));
      As[buf][(a_i + C::kAStride * j) * BM + a_r] = mul_rn(r, w);  // block[i] = slice[i]*window[i], :480
    }
#pragma unroll
    for (int j = 0; j < C::kBPer; ++j) {
      f32x4 b = b_stage[j];
      asm volatile("" : "+v"(b));
      *reinterpret_cast<f32x4 *>(&Bs[buf][(b_r + C::kBRowsPer * j) * BN + b_c4 * 4]) = b;
    }
  };

  f32x2 acc[TM][4];
#pragma unroll
  for (int r = 0; r < TM; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = f32x2{0.0f, 0.0f};

  load_stage(0);
  store_stage(0);
  __syncthreads();

  // LDS byte addresses of this lane's operand columns (low 32 bits of a generic LDS pointer)
  const unsigned a_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&As[0][ty * 4]));
  const unsigned b_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&Bs[0][tx * 4]));

  constexpr int kStages = kFrameI / BK;
#pragma unroll 1
  for (int s = 0; s < kStages; ++s) {
    const int buf = s & 1;
    load_stage(((s + 1) & (kStages - 1)) * BK);
    const unsigned a_addr = a_lds0 + buf * (BK * BM * 4);
    const unsigned b_addr = b_lds0 + buf * (BK * BN * 4);
    Operands X, Y;
    lds_fetch4<BM, BN>(X, a_addr, b_addr, 0);
    lds_wait4(X);
#pragma unroll
    for (int ii = 0; ii < BK; ii += 2) {
      step4<BM, BN, true>(acc, X, Y, a_addr, b_addr, ii + 1);
      if (ii + 2 < BK) step4<BM, BN, true>(acc, Y, X, a_addr, b_addr, ii + 2);
      else step4<BM, BN, false>(acc, Y, X, a_addr, b_addr, 0);
    }
    store_stage(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < TM; ++r) {
    const unsigned row = m0 + ty * 4 + r;
    if (row >= M) continue;
    float *dst = coef + static_cast<size_t>(row) * kHopI + n0;
    float4 o;
    o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
    o.z = mul_rn(acc[r][1].x, tb.norm); o.w = mul_rn(acc[r][1].y, tb.norm);
    *reinterpret_cast<float4 *>(dst + tx * 4) = o;
    o.x = mul_rn(acc[r][2].x, tb.norm); o.y = mul_rn(acc[r][2].y, tb.norm);
    o.z = mul_rn(acc[r][3].x, tb.norm); o.w = mul_rn(acc[r][3].y, tb.norm);
    *reinterpret_cast<float4 *>(dst + BN / 2 + tx * 4) = o;
  }
}

template <int BM, int BN, int BK, int MINW>
inline hipError_t launch_sched(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M,
                               float *coef, hipStream_t s) {
  using C = Cfg<BM, BN, BK, 4, 8, 2, MINW>;
  if (M == 0) return hipSuccess;
  const unsigned m_tiles = (M + BM - 1) / BM;
  hipLaunchKernelGGL((k_mdct_fwd_sched<BM, BN, BK, MINW>), dim3(m_tiles * C::kNTiles), dim3(C::kThreads), 0, s, t, pcm,
                     static_cast<long long>(frame_begin), M, coef);
  return hipGetLastError();
}

#ifndef GLC_K1_A_STRIDE
#define GLC_K1_A_STRIDE 132  // floats between consecutive i rows of the A tile in LDS (128 = unpadded; tuning: k1_tune)
#endif
// ------------------------------------------------------------------------------------------
// LDS-DMA kernel (128x128 tile, 512 threads, 4x8 outputs per lane, 3-slot LDS ring).
// The table tile of stage s+2 is copied global -> LDS by `global_load_lds_dwordx4` while stages s
// and s+1 compute: two stages of latency budget, no VGPRs and no ds_write for the table.  The PCM
// tile (needs the window multiply) goes through registers one stage ahead, the window itself sits
// in LDS.  The PCM loads of the loop are inline asm (hipcc must not move their first use); one
// `s_waitcnt vmcnt(0)` per stage, in the middle of the stage, retires loads that are a stage old.
// Same arithmetic, same order.
// ------------------------------------------------------------------------------------------
// PRIO (speed only; which one ships is decided by tools/k1_tune.hip): issue priority as a schedule.  The
// two workgroups of a CU (2 + 2 waves on every SIMD) are arbitrated oldest-first, so left alone the
// older one takes every issue slot it can use and the younger one fills its gaps - and finishes the
// kernel alone, two waves to a SIMD.  A wave lowers its own priority as it gets through the i loop, so
// whichever workgroup is behind goes first:  1 = by quarter of the loop (3, 2, 1, 0);  2 / 3 / 4 = a
// cycle of four levels every 8 / 16 / 32 stages (the skew stays within a cycle).
// STAMP (tuning only): workgroup timeline into `stamps` - start, the four quarter points, end.
template <int MINW, int CH = 0, int PRIO = 0, bool STAMP = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(MINW, MINW)))
void k_mdct_fwd_dma(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M, float *__restrict__ coef,
                    unsigned long long *__restrict__ stamps) {
  // CH = 0: the per-row loader, one PCM dword per (row, i) and lane - any channel count.  CH = 1 / 2 / 4 / 8 (the
  // stream's channel count): the segment loader, one piece.
  // 512 threads, 2 workgroups per CU (56 KiB LDS each).
  constexpr int BM = 128, BN = 128, BK = 16, TM = 4, RING = 3;
  // A rows are kAS floats apart in LDS, 4 more than the tile is wide: the segment loader's four ds_write_b32
  // per lane put lanes of DIFFERENT i at the same column, and with a stride of 128 floats all of them fall
  // into one bank (8-way for stereo, 16-way for 4 / 8 channels: SQ_LDS_BANK_CONFLICT was 22 % of the
  // LDS-array cycles, profiles/r03_k1_pmc_before_prio.txt); the padding spreads them (2-way, which costs nothing).
  constexpr int kAS = GLC_K1_A_STRIDE;
  constexpr int kThreads = 4 * BM;
  constexpr int kAPer = 4, kAStride = 4;
  constexpr bool kSeg = CH != 0;  // segment loader
  static_assert(!kSeg || CH == 1 || CH == 2 || CH == 4 || CH == 8, "segment loader shapes");
  constexpr int kDma = (BK * BN * 4) / (kThreads * 16);  // table-DMA instructions per thread and stage
  static_assert(kDma == 1, "one table-DMA instruction per thread and stage");
  __shared__ __attribute__((aligned(16))) float As[RING][BK * kAS];
  __shared__ __attribute__((aligned(16))) float Bs[RING][BK * BN];
  __shared__ __attribute__((aligned(16))) float Ws[kFrameI];

  const int tid = threadIdx.x;
  const unsigned g = xcd_tile();
  const int n_tile = g % 8;
  const int m_tile = g / 8;
  const int m0 = m_tile * BM;
  const int n0 = n_tile * BN;
  const int tx = tid % 16, ty = tid / 16;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;

  for (int i = tid; i < kFrameI; i += kThreads) Ws[i] = tb.window[i];

  const long long ch = pcm.ch;
  const PcmTile a_tile = pcm_tile(pcm, frame_begin, m0, pcm.ch);
  const __amdgpu_buffer_rsrc_t a_rsrc = a_tile.rsrc;  // (what the stage lambdas take: a_tile stays out of their captures)
  // per-row loader: lane -> (row a_r of the tile, i = a_i + 4 j; a_i is the same for every lane of a wave)
  const int a_r = tid % BM;
  const int a_i = tid / BM;
  unsigned a_off = kPcmNoRow;
  const unsigned a_step = static_cast<unsigned>(kAStride * ch * 4);
  const unsigned i_bytes = static_cast<unsigned>(ch * 4);
  float a_raw[kAPer];
  SegLoader<kSeg ? CH : 1, BK, kAS> seg(tid, true);
  if constexpr (kSeg) {
    const unsigned row0 = m0 + seg.fl * CH;
    if (row0 < M) seg.off = static_cast<unsigned>((pcm_frame_first(pcm, frame_begin, row0, CH) - a_tile.e_base + seg.o) * 4);
  } else {
    pcm_row_origin(a_off, pcm, a_tile, frame_begin, m0 + a_r, M, pcm.ch, a_i);
  }
  // table DMA: wave w copies rows 2 w, 2 w + 1 of the stage's 16 x 128 tile (1 KiB, lane-linear)
  const float *b_src = tb.cos_t + n0 + static_cast<size_t>(2 * wave + (lane >> 5)) * kHopI + (lane & 31) * 4;

  auto issue_a = [&](int i0) {
    if constexpr (kSeg) return seg.issue(a_rsrc, static_cast<unsigned>(i0) * i_bytes);
    pcm_issue_rows<kAPer>(a_raw, a_rsrc, a_off + static_cast<unsigned>(i0) * i_bytes, a_step);
  };
  auto issue_b = [&](int i0, int slot) {
    __builtin_amdgcn_global_load_lds(b_src + static_cast<size_t>(i0) * kHopI, &Bs[slot][2 * wave * BN], 16, 0, 0);
  };
  auto store_a = [&](int i0, int slot) {
    if constexpr (kSeg) return seg.store(i0, slot, As, Ws);
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int ii = a_i + kAStride * j;
      As[slot][ii * kAS + a_r] = mul_rn(a_raw[j], Ws[i0 + ii]);  // block[i] = slice[i]*window[i], :480
    }
  };
  auto wait_staged = [&]() {  // everything this wave has in flight: PCM registers + table DMA of the next stage
    if constexpr (kSeg) return seg.wait();
    pcm_wait_rows(a_raw);
  };

  f32x2 acc[TM][4];
#pragma unroll
  for (int r = 0; r < TM; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = f32x2{0.0f, 0.0f};

  constexpr int kStages = kFrameI / BK;
  // prologue: stage 0 complete in slot 0, table of stage 1 in flight to slot 1, PCM of stage 1 in regs
  __syncthreads();  // Ws
  issue_a(0);
  issue_b(0, 0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
               : "+v"(a_raw[0]), "+v"(a_raw[1]), "+v"(a_raw[2]), "+v"(a_raw[3]), "+v"(seg.v)::"memory");
  store_a(0, 0);
  issue_a(BK);
  issue_b(BK, 1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  const unsigned a_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&As[0][ty * 4]));
  const unsigned b_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&Bs[0][tx * 4]));

  // Stage hand-off in the MIDDLE of a stage (round 2): the next stage's tiles are published by a
  // barrier after the first 8 i-steps, so the stage's last i-step prefetches the first operands of
  // the next stage and no wave starts a stage with an exposed LDS round trip.  The table DMA and the
  // PCM loads of stage s+2 are issued right after that barrier - every wave has then left stage s-1,
  // whose slot the DMA overwrites - and have 1.5 stages to land, so the mid-stage wait is a plain
  // vmcnt(0) on loads that are a whole stage old.  Slot use: stage s reads slot s % 3; As[(s+1) % 3]
  // is written before the barrier of stage s (last read in stage s-2), Bs[(s+2) % 3] after it.
  // Measured against the end-of-stage hand-off with a counted vmcnt(1) (round 1, kept as
  // k1x::k_mdct_fwd_dma in tools/k1_variants.hpp): the same time within run-to-run noise (0.58 ms,
  // profiles/r02_k1_tune_mid_stage.txt) - the hand-off is not where the idle issue slots come from -
  // so the simpler protocol (one plain wait on stage-old loads, no exposed fetch) is the one shipped.
  Operands X, Y;
  lds_fetch4<kAS, BN>(X, a_lds0, b_lds0, 0);
  lds_wait4(X);
  if constexpr (STAMP) {
    if (tid == 0) stamps[static_cast<size_t>(blockIdx.x) * 8] = __builtin_amdgcn_s_memrealtime();
  }
  if constexpr (PRIO != 0) __builtin_amdgcn_s_setprio(3);
#pragma unroll 1
  for (int s = 0; s < kStages; ++s) {
    if constexpr (PRIO >= 5) {
      // a ladder that gets finer towards the end (the tail of a launch is as long as its last rung):
      //   5: [0, 64) 3, [64, 96) 2, [96, 112) 1, [112, 128) 0      6: [0, 48) 3, [48, 96) 2, [96, 120) 1, [120, 128) 0
      constexpr int b1 = PRIO == 5 ? 64 : 48, b2 = 96, b3 = PRIO == 5 ? 112 : 120;
      if (s == b1) __builtin_amdgcn_s_setprio(2);
      else if (s == b2) __builtin_amdgcn_s_setprio(1);
      else if (s == b3) __builtin_amdgcn_s_setprio(0);
    } else if constexpr (PRIO != 0) {
      constexpr int kShift = PRIO == 1 ? 5 : PRIO == 2 ? 1 : PRIO == 3 ? 2 : 3;  // stages per level = 1 << kShift
      if ((s & ((1 << kShift) - 1)) == 0) {
        const int level = (s >> kShift) & 3;
        if (level == 0) __builtin_amdgcn_s_setprio(3);
        else if (level == 1) __builtin_amdgcn_s_setprio(2);
        else if (level == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
    }
    if constexpr (STAMP) {
      if (tid == 0 && (s & 31) == 0 && s) stamps[static_cast<size_t>(blockIdx.x) * 8 + (s >> 5)] = __builtin_amdgcn_s_memrealtime();
    }
    const int slot = s % 3, nslot = (s + 1) % 3;
    const unsigned a_addr = a_lds0 + slot * (BK * kAS * 4);
    const unsigned b_addr = b_lds0 + slot * (BK * BN * 4);
    const unsigned a_next = a_lds0 + nslot * (BK * kAS * 4);
    const unsigned b_next = b_lds0 + nslot * (BK * BN * 4);
#pragma unroll
    for (int ii = 0; ii < BK / 2; ii += 2) {
      step4<kAS, BN, true>(acc, X, Y, a_addr, b_addr, ii + 1);
      step4<kAS, BN, true>(acc, Y, X, a_addr, b_addr, ii + 2);
    }
    // stage s+1: its PCM registers and table DMA (both issued in the middle of stage s-1) have landed
    wait_staged();
    store_a(((s + 1) & (kStages - 1)) * BK, nslot);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's ds_writes of stage s+1 have landed
    __builtin_amdgcn_s_barrier();
    issue_b(((s + 2) & (kStages - 1)) * BK, (s + 2) % 3);  // the slot of stage s-1: every wave has left it
    issue_a(((s + 2) & (kStages - 1)) * BK);
#pragma unroll
    for (int ii = BK / 2; ii < BK; ii += 2) {
      step4<kAS, BN, true>(acc, X, Y, a_addr, b_addr, ii + 1);
      if (ii + 2 < BK) step4<kAS, BN, true>(acc, Y, X, a_addr, b_addr, ii + 2);
      else step4<kAS, BN, true>(acc, Y, X, a_next, b_next, 0);  // the first operands of stage s+1
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the wrap-around prefetches
  if constexpr (STAMP) {
    if (tid == 0) stamps[static_cast<size_t>(blockIdx.x) * 8 + 4] = __builtin_amdgcn_s_memrealtime();
  }

#pragma unroll
  for (int r = 0; r < TM; ++r) {
    const unsigned row = m0 + ty * 4 + r;
    if (row >= M) continue;
    float *dst = coef + static_cast<size_t>(row) * kHopI + n0;
    float4 o;
    o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
    o.z = mul_rn(acc[r][1].x, tb.norm); o.w = mul_rn(acc[r][1].y, tb.norm);
    *reinterpret_cast<float4 *>(dst + tx * 4) = o;
    o.x = mul_rn(acc[r][2].x, tb.norm); o.y = mul_rn(acc[r][2].y, tb.norm);
    o.z = mul_rn(acc[r][3].x, tb.norm); o.w = mul_rn(acc[r][3].y, tb.norm);
    *reinterpret_cast<float4 *>(dst + BN / 2 + tx * 4) = o;
  }
}

template <int MINW, int CH = 0, int PRIO = 0, bool STAMP = false>
inline hipError_t launch_dma(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M,
                             float *coef, hipStream_t s, unsigned long long *stamps = nullptr) {
  if (M == 0) return hipSuccess;
  if (CH != 0 && pcm.ch != static_cast<uint32_t>(CH)) return hipErrorInvalidValue;
  if (STAMP && !stamps) return hipErrorInvalidValue;
  const unsigned m_tiles = (M + 127) / 128;
  hipLaunchKernelGGL((k_mdct_fwd_dma<MINW, CH, PRIO, STAMP>), dim3(m_tiles * 8), dim3(512), 0, s, t, pcm,
                     static_cast<long long>(frame_begin), M, coef, stamps);
  return hipGetLastError();
}


// ------------------------------------------------------------------------------------------
// Scalar-table kernel (256 x 64 tile, 512 threads, 4 rows x 8 columns per lane, lanes <-> ROWS).
// The other kernels give a lane its own columns, so the table value is the per-lane operand and the
// sample the shared one - and a shared operand that is windowed on the fly cannot come from anywhere
// but LDS.  Turn the tile round: the 64 lanes of a wave hold 256 DIFFERENT rows and the SAME 8 columns.
// The 8 table values of an i-step are then wave-uniform and static - one s_load_dwordx8 straight from
// the table in global memory into SGPRs, no table tile in LDS at all - and the lane's 4 windowed samples
// are one ds_read_b128.  Per i-step and wave: 1 KiB out of LDS instead of 3 KiB, one operand of every
// v_pk_mul from the scalar file (tools/microbench_sgpr.hip: the same stream holds 3-5 % more clock
// that way).  Same products, same ascending-i adds, one accumulator per output.
// Scalar loads return out of order, so every wait is lgkmcnt(0); operands are therefore fetched TWO
// i-steps at a time, a whole pair ahead (as k_imdct_apply does with its records).
// ------------------------------------------------------------------------------------------
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x8 __attribute__((ext_vector_type(8)));

template <int D>
struct StOps {  // operands of D i-steps: 4 rows of this lane (VGPRs), 8 columns of this wave (SGPRs)
  f32x4 a[D];
  u32x8 b[D];
};

// II: i-step inside the stage (compile time: all offsets are immediates)
template <int II>
__device__ __forceinline__ void st_fetch_b(u32x8 &b, const unsigned *brow) {
  asm volatile("s_load_dwordx8 %0, %1, %c2" : "=&s"(b) : "s"(brow), "i"(II * kHopI * 4) : "memory");
}
template <int II, int AS>
__device__ __forceinline__ void st_fetch_a(f32x4 &a, unsigned a_addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=&v"(a) : "v"(a_addr), "i"(II * AS * 4) : "memory");
}
template <int II, int AS, int D>
__device__ __forceinline__ void st_fetch(StOps<D> &o, unsigned a_addr, const unsigned *brow) {
  static_assert(D == 2 || D == 4, "i-steps per fetch");
  st_fetch_b<II>(o.b[0], brow);
  st_fetch_b<II + 1>(o.b[1], brow);
  if constexpr (D == 4) {
    st_fetch_b<II + 2>(o.b[2], brow);
    st_fetch_b<II + 3>(o.b[3], brow);
  }
  st_fetch_a<II, AS>(o.a[0], a_addr);
  st_fetch_a<II + 1, AS>(o.a[1], a_addr);
  if constexpr (D == 4) {
    st_fetch_a<II + 2, AS>(o.a[2], a_addr);
    st_fetch_a<II + 3, AS>(o.a[3], a_addr);
  }
}

// scalar and vector results are tied in SEPARATE statements (an asm with one VGPR output makes all of
// its outputs divergent to LLVM, and the table values would be copied to VGPRs)
template <int D>
__device__ __forceinline__ void st_wait(StOps<D> &o) {
  if constexpr (D == 2) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(o.b[0]), "+s"(o.b[1])::"memory");
    asm volatile("" : "+v"(o.a[0]), "+v"(o.a[1])::"memory");
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(o.b[0]), "+s"(o.b[1]), "+s"(o.b[2]), "+s"(o.b[3])::"memory");
    asm volatile("" : "+v"(o.a[0]), "+v"(o.a[1]), "+v"(o.a[2]), "+v"(o.a[3])::"memory");
  }
}

// rows (r, r+1) x 8 columns, table pairs in SGPRs: the instruction block of mac2rows
__device__ __forceinline__ void mac2rows_st(f32x2 (&c0)[4], f32x2 (&c1)[4], f32x2 a, u32x2 b0, u32x2 b1, u32x2 b2,
                                            u32x2 b3) {
  f32x2 t0, t1, t2, t3, t4, t5, t6, t7;
  asm volatile(
      "v_pk_mul_f32 %8, %16, %17 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %9, %16, %18 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %10, %16, %19 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %11, %16, %20 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %12, %16, %17 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %13, %16, %18 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %14, %16, %19 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %15, %16, %20 op_sel:[1,0]\n\t"
      "v_pk_add_f32 %0, %0, %8\n\t"
      "v_pk_add_f32 %1, %1, %9\n\t"
      "v_pk_add_f32 %2, %2, %10\n\t"
      "v_pk_add_f32 %3, %3, %11\n\t"
      "v_pk_add_f32 %4, %4, %12\n\t"
      "v_pk_add_f32 %5, %5, %13\n\t"
      "v_pk_add_f32 %6, %6, %14\n\t"
      "v_pk_add_f32 %7, %7, %15"
      : "+v"(c0[0]), "+v"(c0[1]), "+v"(c0[2]), "+v"(c0[3]), "+v"(c1[0]), "+v"(c1[1]), "+v"(c1[2]), "+v"(c1[3]),
        "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7)
      : "v"(a), "s"(b0), "s"(b1), "s"(b2), "s"(b3));
}

// the fetch's i-steps: ascending i, for every output
template <int D>
__device__ __forceinline__ void st_mac(f32x2 (&acc)[4][4], const StOps<D> &o) {
#pragma unroll
  for (int d = 0; d < D; ++d) {
    mac2rows_st(acc[0], acc[1], o.a[d].xy, o.b[d].s01, o.b[d].s23, o.b[d].s45, o.b[d].s67);
    mac2rows_st(acc[2], acc[3], o.a[d].zw, o.b[d].s01, o.b[d].s23, o.b[d].s45, o.b[d].s67);
  }
}

// Bound waves of the mixed-role kernel (k_mdct_mix_st): the same operands, ONE v_pk_fma_f32 per packed
// multiply-add.  What they accumulate is not a coefficient of the stream - it only feeds the upper bound of
// the screen - so neither the fused rounding nor the order matters.
__device__ __forceinline__ void mac2rows_fma(f32x2 (&c0)[4], f32x2 (&c1)[4], f32x2 a, u32x2 b0, u32x2 b1, u32x2 b2,
                                             u32x2 b3) {
  asm volatile(
      "v_pk_fma_f32 %0, %8, %9, %0 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %1, %8, %10, %1 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %2, %8, %11, %2 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %3, %8, %12, %3 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %4, %8, %9, %4 op_sel:[1,0,0]\n\t"
      "v_pk_fma_f32 %5, %8, %10, %5 op_sel:[1,0,0]\n\t"
      "v_pk_fma_f32 %6, %8, %11, %6 op_sel:[1,0,0]\n\t"
      "v_pk_fma_f32 %7, %8, %12, %7 op_sel:[1,0,0]"
      : "+v"(c0[0]), "+v"(c0[1]), "+v"(c0[2]), "+v"(c0[3]), "+v"(c1[0]), "+v"(c1[1]), "+v"(c1[2]), "+v"(c1[3])
      : "v"(a), "s"(b0), "s"(b1), "s"(b2), "s"(b3));
}

// Hybrid waves of the mixed-role kernel: of the wave's four column pairs the first two are exact - mac2rows_st's
// separately rounded multiply, then add, per pair - and the other two are bound pairs (mac2rows_fma's fused op).
// The multiplies lead and the adds trail, so a product is as far from its add as in mac2rows_st.
__device__ __forceinline__ void mac2rows_hy(f32x2 (&c0)[4], f32x2 (&c1)[4], f32x2 a, u32x2 b0, u32x2 b1, u32x2 b2,
                                            u32x2 b3) {
  f32x2 t0, t1, t2, t3;
  asm volatile(
      "v_pk_mul_f32 %8, %12, %13 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %9, %12, %14 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %10, %12, %13 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %11, %12, %14 op_sel:[1,0]\n\t"
      "v_pk_fma_f32 %2, %12, %15, %2 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %3, %12, %16, %3 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %6, %12, %15, %6 op_sel:[1,0,0]\n\t"
      "v_pk_fma_f32 %7, %12, %16, %7 op_sel:[1,0,0]\n\t"
      "v_pk_add_f32 %0, %0, %8\n\t"
      "v_pk_add_f32 %1, %1, %9\n\t"
      "v_pk_add_f32 %4, %4, %10\n\t"
      "v_pk_add_f32 %5, %5, %11"
      : "+v"(c0[0]), "+v"(c0[1]), "+v"(c0[2]), "+v"(c0[3]), "+v"(c1[0]), "+v"(c1[1]), "+v"(c1[2]), "+v"(c1[3]),
        "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
      : "v"(a), "s"(b0), "s"(b1), "s"(b2), "s"(b3));
}

// Which columns a wave of the mixed-role kernel owns and what it does with them.
//
// hp = 0 (ne > 11, and wherever the balanced form is not built: mix_hybrid_pairs): waves
// [0, ne) are exact, [ne, 16) bound.  Waves sit on SIMD wave % 4, so the four SIMDs carry unequal numbers of exact
// waves unless ne is a multiple of 4 (2, 2, 1, 1 for ne = 6), and the fullest sets the pace between two barriers.
// hp = ne % 4 > 0 (ne <= 11): the BALANCED form.  With q = ne / 4, the wave with index k = wave / 4 on its SIMD
// is exact for k < q, HYBRID for k == q - hp of its four column pairs exact, 4 - hp bound - and bound above: every
// SIMD carries ne exact and 16 - ne bound pairs.  (Above ne = 11 a SIMD would be left without a pure bound wave,
// which the A sum needs.)
// Workgroup n_tile owns exact columns [8 ne n_tile, 8 ne (n_tile + 1)) and bound columns C0 + 8 (16 - ne) n_tile ...,
// C0 = 64 ne, in both forms; inside each range the waves take consecutive runs: 8 columns per exact wave, then
// 2 hp per hybrid wave; 8 - 2 hp per hybrid wave, then 8 per bound wave.  A run is what one scalar load fetches:
//   hp = 2   run 0 = the exact 4, run 1 = the bound 4 (the form the kernel is built for: mix_hybrid_pairs)
//   hp = 3   runs 0, 1 = an x4 and an x2 part of the exact 6 (the x4 on a multiple of 4 columns), run 2 = the bound 2
//   hp = 1   runs 0, 1 = an x4 and an x2 part of the bound 6, run 2 = the exact 2
// (the map is stated, and checked below, for every hp; the kernel holds loop copies for hp = 0 and 2 only).
// Every bound-carrying wave, hybrid ones included, owns one hf plane.
constexpr int kMixHybridMax = 11;  // largest ne the balanced form takes
struct MixWave {
  int kind;    // 0 exact, 1 bound, 2 hybrid
  int plane;   // hf plane of the wave's bound columns (none: -1)
  int col[3];  // first column of each run
  int len[3];  // columns of each run
  int exact;   // bit r: run r holds exact columns
};
// The exact pairs per hybrid wave a launch takes.  Only 2 is built: at ne = 6 (44.1 / 48 kHz) it measured faster than
// whole waves, at ne = 3 (96 kHz, 3 pairs) the balanced form measured no faster - the chip holds less clock under the
// fuller SIMDs (profiles/encode_balance_bench.txt) - and no rate has ne % 4 == 1; those keep whole waves.
__host__ __device__ constexpr int mix_hybrid_pairs(int ne) { return ne <= kMixHybridMax && ne % 4 == 2 ? 2 : 0; }
// first wave that carries bound columns; every wave from there on owns an hf plane
__host__ __device__ constexpr int mix_first_bound(int ne, int hp) { return hp ? ne / 4 * 4 : ne; }
// first wave with bound columns only: it also carries the A sum in workgroups n_tile < 4
__host__ __device__ constexpr int mix_a_wave(int ne, int hp) { return hp ? ne / 4 * 4 + 4 : ne; }
// hf planes of a launch (the A plane follows them)
__host__ __device__ constexpr int mix_planes(int ne, int hp) { return 8 * (16 - mix_first_bound(ne, hp)); }
__host__ __device__ constexpr MixWave mix_wave(int ne, int hp, int n_tile, int wave) {
  const int xb = 8 * ne * n_tile;                        // the workgroup's exact columns
  const int bb = 64 * ne + 8 * (16 - ne) * n_tile;       // ... and its bound columns
  const int fb = mix_first_bound(ne, hp);
  const int plane = (16 - fb) * n_tile + wave - fb;
  if (hp == 0) {
    if (wave < ne) return MixWave{0, -1, {xb + 8 * wave, 0, 0}, {8, 0, 0}, 1};
    return MixWave{1, plane, {bb + 8 * (wave - ne), 0, 0}, {8, 0, 0}, 0};
  }
  const int q = ne / 4, k = wave / 4, sd = wave % 4, odd = sd & 1;
  if (k < q) return MixWave{0, -1, {xb + 8 * wave, 0, 0}, {8, 0, 0}, 1};
  if (k > q) return MixWave{1, plane, {bb + 4 * (8 - 2 * hp) + 8 * (wave - 4 * q - 4), 0, 0}, {8, 0, 0}, 0};
  const int xr = xb + 32 * q + 2 * hp * sd;              // the hybrid wave's exact run
  const int br = bb + (8 - 2 * hp) * sd;                 // ... and its bound run
  if (hp == 2) return MixWave{2, plane, {xr, br, 0}, {4, 4, 0}, 1};
  // the 6 column run starts on 2 mod 4 columns on the odd SIMDs: x2 first there, x4 first on the even ones
  if (hp == 3) return MixWave{2, plane, {xr + (odd ? 2 : 0), xr + (odd ? 0 : 4), br}, {4, 2, 2}, 3};
  return MixWave{2, plane, {br + (odd ? 2 : 0), br + (odd ? 0 : 4), xr}, {4, 2, 2}, 4};
}
// no column left out, none covered twice, exact columns exactly [0, 64 ne), ne exact pairs per SIMD, one wave per plane
__host__ __device__ constexpr bool mix_map_ok(int ne, int hp) {
  int own[kHopI] = {};
  int plane_used[8 * 16] = {};
  int exact_pairs[4] = {};
  for (int j = 0; j < 8; ++j)
    for (int w = 0; w < 16; ++w) {
      const MixWave m = mix_wave(ne, hp, j, w);
      int cols = 0;
      for (int r = 0; r < 3; ++r) {
        const bool ex = (m.exact >> r) & 1;
        if (m.len[r] && (m.col[r] % (m.len[r] == 8 ? 8 : m.len[r]) || m.col[r] < 0 || m.col[r] + m.len[r] > kHopI)) return false;
        for (int c = m.col[r]; c < m.col[r] + m.len[r]; ++c) {
          if (own[c]++ || ex != (c < 64 * ne)) return false;
        }
        cols += m.len[r];
        if (ex && j == 0) exact_pairs[w % 4] += m.len[r] / 2;
      }
      if (cols != 8) return false;
      if ((m.kind == 0) != (m.plane < 0)) return false;
      if (m.plane >= 0 && (m.plane >= mix_planes(ne, hp) || plane_used[m.plane]++)) return false;
      if (m.kind == 2 && (m.exact & 1 ? m.len[0] + (hp == 3 ? m.len[1] : 0) : m.len[2]) != 2 * hp) return false;
    }
  for (int c = 0; c < kHopI; ++c)
    if (own[c] != 1) return false;
  for (int p = 0; p < mix_planes(ne, hp); ++p)
    if (plane_used[p] != 1) return false;
  if (hp)
    for (int sd = 0; sd < 4; ++sd)
      if (exact_pairs[sd] != ne) return false;
  return mix_a_wave(ne, hp) < 16 && mix_wave(ne, hp, 0, mix_a_wave(ne, hp)).kind == 1;
}
template <int NE>
constexpr bool mix_maps_ok() {  // whole waves for every ne, the balanced map wherever it exists (built or not)
  if constexpr (NE == 0) return true;
  else return mix_map_ok(NE, 0) && mix_map_ok(NE, NE <= kMixHybridMax ? NE % 4 : 0) && mix_maps_ok<NE - 1>();
}
static_assert(mix_maps_ok<15>(), "column and plane map of the mixed-role kernel");

// operands of 4 i-steps of a hybrid wave: the same 8 table values per i-step as StOps, as its two runs of 4 columns
struct HyOps {
  f32x4 a[4];
  u32x4 x[4], b[4];  // the exact run, the bound run
};
// trow: column 0 of the table row of the stage's first i-step; ox, ob: byte offsets of the wave's two runs in a row.
// One pointer and two offsets, not two pointers (and two more for the next stage): the 64 table values in flight
// leave little room in the scalar file.
template <int II>
__device__ __forceinline__ void hy_fetch_b(u32x4 &x, u32x4 &b, const unsigned *trow, unsigned ox, unsigned ob) {
  asm volatile("s_load_dwordx4 %0, %1, %2 offset:%c3" : "=&s"(x) : "s"(trow), "s"(ox), "i"(II * kHopI * 4) : "memory");
  asm volatile("s_load_dwordx4 %0, %1, %2 offset:%c3" : "=&s"(b) : "s"(trow), "s"(ob), "i"(II * kHopI * 4) : "memory");
}
template <int II, int AS>
__device__ __forceinline__ void hy_fetch(HyOps &o, unsigned a_addr, const unsigned *trow, unsigned ox, unsigned ob) {
  hy_fetch_b<II>(o.x[0], o.b[0], trow, ox, ob);
  hy_fetch_b<II + 1>(o.x[1], o.b[1], trow, ox, ob);
  hy_fetch_b<II + 2>(o.x[2], o.b[2], trow, ox, ob);
  hy_fetch_b<II + 3>(o.x[3], o.b[3], trow, ox, ob);
  st_fetch_a<II, AS>(o.a[0], a_addr);
  st_fetch_a<II + 1, AS>(o.a[1], a_addr);
  st_fetch_a<II + 2, AS>(o.a[2], a_addr);
  st_fetch_a<II + 3, AS>(o.a[3], a_addr);
}
__device__ __forceinline__ void hy_wait(HyOps &o) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+s"(o.x[0]), "+s"(o.x[1]), "+s"(o.x[2]), "+s"(o.x[3]), "+s"(o.b[0]), "+s"(o.b[1]), "+s"(o.b[2]),
                 "+s"(o.b[3])::"memory");
  asm volatile("" : "+v"(o.a[0]), "+v"(o.a[1]), "+v"(o.a[2]), "+v"(o.a[3])::"memory");
}
__device__ __forceinline__ void hy_mac(f32x2 (&acc)[4][4], const HyOps &o) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    mac2rows_hy(acc[0], acc[1], o.a[d].xy, o.x[d].xy, o.x[d].zw, o.b[d].xy, o.b[d].zw);
    mac2rows_hy(acc[2], acc[3], o.a[d].zw, o.x[d].xy, o.x[d].zw, o.b[d].xy, o.b[d].zw);
  }
}

// ROLE of a wave's copy of the i loop: 0 = exact (st_mac: the stream's arithmetic), 1 = bound (fused), 2 + j = bound,
// and the wave also sums |x w| of row j of each lane's 4 over the whole i loop (asum: the A of the screen's error
// term), kRoleHybrid = hybrid (hy_mac)
constexpr int kRoleHybrid = 6;
template <int ROLE, int D>
__device__ __forceinline__ void st_mac_role(f32x2 (&acc)[4][4], float &asum, const StOps<D> &o) {
  if constexpr (ROLE == 0) {
    st_mac(acc, o);
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      mac2rows_fma(acc[0], acc[1], o.a[d].xy, o.b[d].s01, o.b[d].s23, o.b[d].s45, o.b[d].s67);
      mac2rows_fma(acc[2], acc[3], o.a[d].zw, o.b[d].s01, o.b[d].s23, o.b[d].s45, o.b[d].s67);
      if constexpr (ROLE >= 2) asum = add_rn(asum, __builtin_fabsf(o.a[d][ROLE - 2]));
    }
  }
}
template <int V>
struct RoleTag {
  static constexpr int value = V;
};

// NW waves per workgroup (8: 256 x 64 tile, two workgroups per CU;  16: 256 x 128, one), BK i-steps per
// LDS stage, D i-steps per operand fetch.
// PRIO 1: priority by quarter of the i loop (between the two workgroups of a CU, as k_mdct_fwd_dma);
// PRIO 2: by distance from the last barrier (inside a workgroup: whoever is behind goes first).
// ABL (tuning only, wrong results): 1 = the table address does not advance, 2 = no staging and no barrier.
// STAMP (tuning only): workgroup timeline into `stamps` - entry, loop start, the quarter points, loop end, stores drained.
//
// MIX (k_mdct_mix_st, 16 waves): the mixed-role form for launches whose records can only depend on the columns
// below C0 = 64 ne when a row passes the screen.  Tile, staging, ring and barriers are the
// same; what changes is which columns a wave owns and what it does with them (mix_wave, above).  Workgroup
// n_tile = j owns exact columns [8 ne j, 8 ne (j + 1)) and bound columns C0 + 8 (16 - ne) j ....  EXACT waves run
// st_mac on 8 of the former and store coefficients.  BOUND waves run fused multiply-adds (half the issue slots) on 8
// of the latter and store none; per row the largest |sum| of the wave's columns goes to its plane hf[plane][row]
// (plain coalesced stores, every slot of the launch is written).  HYBRID waves (E > 0: E exact column pairs, 4 - E
// bound ones) do both with their two kinds of columns, so that every SIMD - waves sit on SIMD wave % 4 - carries ne
// exact and 16 - ne bound pairs and issues the same 2 ne + (16 - ne) packed operations per i-step; E = 0 is the
// layout with whole waves only (2, 2, 1, 1 exact waves per SIMD for ne = 6: 96, 96, 80, 80).  The sum of |x w| of a
// row - it does not depend on the columns - is formed by the first bound-only wave of workgroups j = 0 .. 3, workgroup
// j adding row j of each lane's four (one add per i-step; four in one workgroup would put that workgroup behind the
// other seven of the launch's single round) and storing it at hf[planes][m0 + 4 lane + j]: per row the same
// ascending f32 sum wherever it is formed.
// The role branch is wave-uniform and outside the i loop; every role runs the same barriers.
template <int CH, int PRIO, int D, int NW, int BK, int ABL, bool STAMP, bool MIX, int E = 0>
__device__ __forceinline__ void st_body(const DeviceTables &tb, const PcmView &pcm, long long frame_begin, unsigned M,
                                        float *__restrict__ coef, unsigned long long *__restrict__ stamps, unsigned ne,
                                        float *__restrict__ hf, unsigned long long hf_stride) {
  static_assert(!MIX || (NW == 16 && D == 4), "the mixed-role form is the 16-wave one");
  static_assert((E == 0 || E == 2) && (MIX || E == 0), "exact pairs of the hybrid waves: the forms that are built");
  if constexpr (STAMP) {
    if (threadIdx.x == 0) stamps[static_cast<size_t>(blockIdx.x) * 8] = __builtin_amdgcn_s_memrealtime();
  }
  // CH as in k_mdct_fwd_dma: 0 = one PCM dword per (row, i) and lane; 1 / 2 / 4 / 8 = the stream's
  // channel count, BK samples x CH channels of a frame fetched as BK / 4 * CH dwordx4.
  constexpr int BM = 256, BN = 8 * NW, RING = 3;
  constexpr int kAS = BM + 4;  // the same bank spread as GLC_K1_A_STRIDE (260 = 132 = 4 mod 64)
  constexpr int kThreads = NW * 64;
  constexpr int kNTiles = kHopI / BN;
  constexpr bool kSeg = CH != 0;
  static_assert(!kSeg || CH == 1 || CH == 2 || CH == 4 || CH == 8, "segment loader shapes");
  static_assert((BK == 16 || BK == 32) && BK % (2 * D) == 0, "stage depth");
  constexpr int kIGroups = kThreads / BM;          // per-row loader: i = a_i + kIGroups * j
  constexpr int kAPer = BK / kIGroups;             //   dwords per lane and stage
  constexpr int kPieces = BM * BK / 4 / kThreads;  // segment loader: dwordx4 per lane and stage
  static_assert(kAPer == 4 || kAPer == 8, "per-row loader shapes");
  static_assert(kPieces == 1 || kPieces == 2, "segment loader shapes");
  __shared__ __attribute__((aligned(16))) float As[RING][BK * kAS];
  __shared__ __attribute__((aligned(16))) float Ws[kFrameI];

  const int tid = threadIdx.x;
  const unsigned g = xcd_tile();
  const int n_tile = g % kNTiles;
  const int m_tile = g / kNTiles;
  const int m0 = m_tile * BM;
  const int n0 = n_tile * BN;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;

  for (int i = tid; i < kFrameI; i += kThreads) Ws[i] = tb.window[i];

  const long long ch = pcm.ch;
  const PcmTile a_tile = pcm_tile(pcm, frame_begin, m0, pcm.ch);
  const __amdgpu_buffer_rsrc_t a_rsrc = a_tile.rsrc;  // (what the stage lambdas take: a_tile stays out of their captures)
  // per-row loader: lane -> (row a_r of the tile, i = a_i + kIGroups * j)
  const int a_r = tid % BM;
  const int a_i = tid / BM;
  unsigned a_off[2] = {kPcmNoRow, kPcmNoRow};
  const unsigned a_step = static_cast<unsigned>(kIGroups * ch * 4);
  const unsigned i_bytes = static_cast<unsigned>(ch * 4);
  // segment loader: SegLoader's rules - (lane, p) -> (frame seg_fl + p * kSegHalf of the tile, 4 consecutive floats of
  // its BK x CH segment) - for one or two pieces, in this body's own statements: on SegLoader, in every form tried,
  // the i loops of the 16-wave instantiations came out with other registers and another instruction order
  // (profiles/k1_loader_isa.txt), and these are the kernels every large launch runs
  constexpr int kSegCh = kSeg ? CH : 1;
  constexpr int kSegLanes = BK / 4 * kSegCh;  // lanes per frame segment
  constexpr int kSegHalf = kThreads / kSegLanes;
  const int seg_fl = tid / kSegLanes;
  const int seg_o = (tid % kSegLanes) * 4;
  if constexpr (kSeg) {
#pragma unroll
    for (int p = 0; p < kPieces; ++p) {
      const unsigned row0 = m0 + (seg_fl + p * kSegHalf) * CH;
      if (row0 < M) a_off[p] = static_cast<unsigned>((pcm_frame_first(pcm, frame_begin, row0, CH) - a_tile.e_base + seg_o) * 4);
    }
  } else {
    pcm_row_origin(a_off[0], pcm, a_tile, frame_begin, m0 + a_r, M, pcm.ch, a_i);
  }

  float a_raw[8];
  f32x4 a_seg[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  auto issue_a = [&](int i0) {  // asm: hipcc must not count these loads (see lds_fetch4)
    if constexpr (kSeg) {
      const unsigned o0 = a_off[0] + static_cast<unsigned>(i0) * i_bytes;
      if constexpr (kPieces == 1) {
        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=&v"(a_seg[0]) : "v"(o0), "s"(a_rsrc) : "memory");
      } else {
        const unsigned o1 = a_off[1] + static_cast<unsigned>(i0) * i_bytes;
        asm volatile("buffer_load_dwordx4 %0, %2, %4, 0 offen\n\tbuffer_load_dwordx4 %1, %3, %4, 0 offen"
                     : "=&v"(a_seg[0]), "=&v"(a_seg[1])
                     : "v"(o0), "v"(o1), "s"(a_rsrc)
                     : "memory");
      }
      return;
    }
    pcm_issue_rows<kAPer>(a_raw, a_rsrc, a_off[0] + static_cast<unsigned>(i0) * i_bytes, a_step);
  };
  auto store_a = [&](int i0, int slot) {
    if constexpr (kSeg) {
#pragma unroll
      for (int p = 0; p < kPieces; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = seg_o + j;  // float e of the segment: sample i = e / CH of channel e % CH
          const int ii = e / CH;
          As[slot][ii * kAS + (seg_fl + p * kSegHalf) * CH + e % CH] = mul_rn(a_seg[p][j], Ws[i0 + ii]);  // :480
        }
      return;
    }
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      const int ii = a_i + kIGroups * j;
      As[slot][ii * kAS + a_r] = mul_rn(a_raw[j], Ws[i0 + ii]);  // block[i] = slice[i]*window[i], :480
    }
  };
  auto wait_staged = [&]() {
    if constexpr (kSeg) {
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(a_seg[0]), "+v"(a_seg[1])::"memory");
      return;
    }
    pcm_wait_rows(a_raw);
  };

  f32x2 acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = f32x2{0.0f, 0.0f};

  constexpr int kStages = kFrameI / BK;
  // prologue: stage 0 complete in slot 0 (the PCM of stage 1 is fetched where the i loop starts)
  __syncthreads();  // Ws
  issue_a(0);
  wait_staged();
  store_a(0, 0);

  const unsigned a_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&As[0][lane * 4]));
  // this wave's 8 columns of table row 0 (wave-uniform: the scalar loads' base)
  int col0 = n0 + 8 * wave, role = 0;
  MixWave mw{};
  if constexpr (MIX) {
    mw = mix_wave(static_cast<int>(ne), E, n_tile, wave);
    col0 = mw.col[0];
    role = mw.kind == 2 ? kRoleHybrid : mw.kind;
    // A does not depend on the columns: the first four workgroups of a row tile form it, workgroup j row j of each
    // lane's four - one add per i-step - so that no workgroup falls behind the others by more than that
    if (wave == mix_a_wave(static_cast<int>(ne), E) && n_tile < 4) role = 2 + n_tile;
  }
  // a hybrid wave's loads start from column 0 and add the byte offset of each of its runs
  const unsigned *b_base = reinterpret_cast<const unsigned *>(tb.cos_t) + (role == kRoleHybrid ? 0 : col0);
  const unsigned hy_ox = static_cast<unsigned>(mw.col[0]) * 4u, hy_ob = static_cast<unsigned>(mw.col[1]) * 4u;

  // Stage hand-off in the middle of a stage, as in k_mdct_fwd_dma: the samples of stage s+1 are
  // published by a barrier after the first BK / 2 i-steps, the stage's last fetch takes the first operands
  // of stage s+1, and the PCM loads of stage s+2 are issued behind the barrier.  Slot use: stage s reads
  // slot s % 3; As[(s+1) % 3] is written before the barrier of stage s (last read in stage s-2).
  float asum = 0.0f;
  // The i loop, once per role of the mixed form (one of them runs).  Every load an asm statement issues and a
  // LATER one waits for - PCM registers, operands - is issued and retired INSIDE it: the compiler does not know such
  // a load is in flight, and where the roles branch or join it may copy the destination registers, or reuse them,
  // before the data has landed.
  auto i_loop = [&](auto role_tag) {
  constexpr int ROLE = decltype(role_tag)::value;
  issue_a(BK);  // PCM of stage 1 into registers
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  constexpr bool kHy = ROLE == kRoleHybrid;
  std::conditional_t<kHy, HyOps, StOps<D>> X, Y;
  // one spelling of fetch / wait / multiply-add for both operand forms
  // (always inlined: the loads they issue are in flight when they return)
  auto fetch = [&](auto ii, auto &o, unsigned a_at, const unsigned *trow) __attribute__((always_inline)) {
    constexpr int II = decltype(ii)::value;
    if constexpr (kHy) hy_fetch<II, kAS>(o, a_at, trow, hy_ox, hy_ob);
    else st_fetch<II, kAS>(o, a_at, trow);
  };
  auto wait = [&](auto &o) __attribute__((always_inline)) {
    if constexpr (kHy) hy_wait(o);
    else st_wait(o);
  };
  fetch(RoleTag<0>{}, X, a_lds0, b_base);
  wait(X);
  if constexpr (STAMP) {
    if (tid == 0) stamps[static_cast<size_t>(blockIdx.x) * 8 + 1] = __builtin_amdgcn_s_memrealtime();
  }
  if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(3);
#pragma unroll 1
  for (int s = 0; s < kStages; ++s) {
    if constexpr (STAMP) {
      if (tid == 0 && s && s % (kStages / 4) == 0) stamps[static_cast<size_t>(blockIdx.x) * 8 + 1 + s / (kStages / 4)] = __builtin_amdgcn_s_memrealtime();
    }
    if constexpr (PRIO == 1) {
      constexpr int kQuarter = kStages / 4;
      if (s % kQuarter == 0) {
        const int level = (s / kQuarter) & 3;
        if (level == 0) __builtin_amdgcn_s_setprio(3);
        else if (level == 1) __builtin_amdgcn_s_setprio(2);
        else if (level == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
    }
    if constexpr (PRIO == 2) __builtin_amdgcn_s_setprio(0);  // half-way between two barriers
    const int slot = (ABL & 2) ? 0 : s % 3, nslot = (ABL & 2) ? 0 : (s + 1) % 3;
    const unsigned a_addr = a_lds0 + slot * (BK * kAS * 4);
    const unsigned a_next = a_lds0 + nslot * (BK * kAS * 4);
    const unsigned *brow = (ABL & 1) ? b_base : b_base + static_cast<size_t>(s) * (BK * kHopI);
    const unsigned *brow_next = (ABL & 1) ? b_base : b_base + static_cast<size_t>((s + 1) & (kStages - 1)) * (BK * kHopI);
    // the hand-off: PCM registers of stage s+1 (issued in the middle of stage s-1) have landed -> LDS,
    // lgkmcnt(0) (this wave's ds_writes and the operands in flight), barrier, PCM loads of stage s+2
#define GLC_ST_HANDOFF(NEXT)                                      \
  do {                                                            \
    wait_staged();                                                \
    store_a(((s + 1) & (kStages - 1)) * BK, nslot);               \
    wait(NEXT);                                                   \
    __builtin_amdgcn_s_barrier();                                 \
    if constexpr (PRIO == 2) __builtin_amdgcn_s_setprio(1);       \
    issue_a(((s + 2) & (kStages - 1)) * BK);                      \
  } while (0)
    // X holds the operands of i-steps [0, D) of the stage; groups alternate X, Y
#define GLC_ST_GROUP(CUR, NXT, II)                                                        \
  do {                                                                                    \
    if constexpr ((II) + D < BK) fetch(RoleTag<((II) + D) % BK>{}, NXT, a_addr, brow);   \
    else fetch(RoleTag<0>{}, NXT, a_next, brow_next);                                     \
    if constexpr (kHy) hy_mac(acc, CUR);                                                  \
    else st_mac_role<ROLE>(acc, asum, CUR);                                               \
    if constexpr ((II) + D == BK / 2 && !(ABL & 2)) GLC_ST_HANDOFF(NXT);                  \
    else wait(NXT);                                                                       \
  } while (0)
    GLC_ST_GROUP(X, Y, 0);
    GLC_ST_GROUP(Y, X, D);
    if constexpr (BK / D > 2) {
      GLC_ST_GROUP(X, Y, 2 * D);
      GLC_ST_GROUP(Y, X, 3 * D);
    }
    if constexpr (BK / D > 4) {
      GLC_ST_GROUP(X, Y, 4 * D);
      GLC_ST_GROUP(Y, X, 5 * D);
      GLC_ST_GROUP(X, Y, 6 * D);
      GLC_ST_GROUP(Y, X, 7 * D);
    }
    if constexpr (BK / D > 8) {
      GLC_ST_GROUP(X, Y, 8 * D);
      GLC_ST_GROUP(Y, X, 9 * D);
      GLC_ST_GROUP(X, Y, 10 * D);
      GLC_ST_GROUP(Y, X, 11 * D);
      GLC_ST_GROUP(X, Y, 12 * D);
      GLC_ST_GROUP(Y, X, 13 * D);
      GLC_ST_GROUP(X, Y, 14 * D);
      GLC_ST_GROUP(Y, X, 15 * D);
    }
#undef GLC_ST_GROUP
#undef GLC_ST_HANDOFF
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the wrap-around prefetch
  };  // i_loop
  if constexpr (MIX) {
    if (role == 0) i_loop(RoleTag<0>{});
    else if (role == 1) i_loop(RoleTag<1>{});
    else if (role == 2) i_loop(RoleTag<2>{});
    else if (role == 3) i_loop(RoleTag<3>{});
    else if (role == 4) i_loop(RoleTag<4>{});
    else if (role == 5) i_loop(RoleTag<5>{});
    else if constexpr (E != 0) i_loop(RoleTag<kRoleHybrid>{});
  } else {
    i_loop(RoleTag<0>{});
  }
  if constexpr (STAMP) {
    if (tid == 0) stamps[static_cast<size_t>(blockIdx.x) * 8 + 5] = __builtin_amdgcn_s_memrealtime();
  }

  if constexpr (MIX) {
    if (role != 0) {
      // rows m0 + 4 lane .. + 3 of the launch's padded row range (hf_stride = rows rounded up to whole tiles:
      // rows >= M were staged as zeros and store 0)
      const int c_lo = role == kRoleHybrid ? E : 0;  // a hybrid wave's first E pairs are coefficients
      f32x4 mx;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c >= c_lo) m = fmaxf(m, fmaxf(__builtin_fabsf(acc[r][c].x), __builtin_fabsf(acc[r][c].y)));
        mx[r] = m;
      }
      const size_t at = static_cast<size_t>(m0) + static_cast<size_t>(lane) * 4;
      *reinterpret_cast<f32x4 *>(hf + static_cast<unsigned>(mw.plane) * hf_stride + at) = mx;
      if (role >= 2 && role < kRoleHybrid)  // row role - 2 of the lane's four
        hf[static_cast<unsigned>(mix_planes(static_cast<int>(ne), E)) * hf_stride + at + static_cast<unsigned>(role - 2)] = asum;
      if (role != kRoleHybrid) return;
      if constexpr (E != 0) {
        // the coefficients of the exact run: 4 columns, on a multiple of 4
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned row = m0 + lane * 4 + r;
          if (row >= M) continue;
          float4 o;
          o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
          o.z = mul_rn(acc[r][1].x, tb.norm); o.w = mul_rn(acc[r][1].y, tb.norm);
          *reinterpret_cast<float4 *>(coef + static_cast<size_t>(row) * kHopI + mw.col[0]) = o;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned row = m0 + lane * 4 + r;
    if (row >= M) continue;
    float *dst = coef + static_cast<size_t>(row) * kHopI + col0;
    float4 o;
    o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
    o.z = mul_rn(acc[r][1].x, tb.norm); o.w = mul_rn(acc[r][1].y, tb.norm);
    *reinterpret_cast<float4 *>(dst) = o;
    o.x = mul_rn(acc[r][2].x, tb.norm); o.y = mul_rn(acc[r][2].y, tb.norm);
    o.z = mul_rn(acc[r][3].x, tb.norm); o.w = mul_rn(acc[r][3].y, tb.norm);
    *reinterpret_cast<float4 *>(dst + 4) = o;
  }
  if constexpr (STAMP) {  // this wave's stores have left the CU
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) stamps[static_cast<size_t>(blockIdx.x) * 8 + 6] = __builtin_amdgcn_s_memrealtime();
  }
}

template <int MINW, int CH = 0, int PRIO = 0, int D = 2, int NW = 8, int BK = 16, int ABL = 0, bool STAMP = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(MINW, MINW)))
void k_mdct_fwd_st(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M, float *__restrict__ coef,
                   unsigned long long *__restrict__ stamps) {
  st_body<CH, PRIO, D, NW, BK, ABL, STAMP, false>(tb, pcm, frame_begin, M, coef, stamps, 0u, nullptr, 0ull);
}

// the mixed-role form (see st_body and mix_wave): E = exact pairs of the hybrid waves (0: none, waves [0, ne) exact),
// hf = [mix_planes(ne, E) + 1][hf_stride] floats
template <int MINW, int CH = 0, int E = 0>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(MINW, MINW)))
void k_mdct_mix_st(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M, float *__restrict__ coef,
                   unsigned ne, float *__restrict__ hf, unsigned long long hf_stride) {
  st_body<CH, 2, 4, 16, 16, 0, false, true, E>(tb, pcm, frame_begin, M, coef, nullptr, ne, hf, hf_stride);
}

// hp: exact pairs of the hybrid waves, 0 or mix_hybrid_pairs(ne) (ScreenShape::hp: the workspace was sized for it)
template <int CH>
inline hipError_t launch_mix_st(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                                uint32_t ne, uint32_t hp, float *hf, uint64_t hf_stride, hipStream_t s) {
  if (M == 0) return hipSuccess;
  if (CH != 0 && pcm.ch != static_cast<uint32_t>(CH)) return hipErrorInvalidValue;
  if (ne < 1 || ne > 15 || hf_stride < M || hf_stride % 256) return hipErrorInvalidValue;
  if (hp != 0 && hp != static_cast<uint32_t>(mix_hybrid_pairs(static_cast<int>(ne)))) return hipErrorInvalidValue;
  const dim3 grid((M + 255) / 256 * 8), block(1024);
  const long long fb = static_cast<long long>(frame_begin);
  const unsigned long long st = hf_stride;
  if (hp == 2) hipLaunchKernelGGL((k_mdct_mix_st<4, CH, 2>), grid, block, 0, s, t, pcm, fb, M, coef, ne, hf, st);
  else hipLaunchKernelGGL((k_mdct_mix_st<4, CH, 0>), grid, block, 0, s, t, pcm, fb, M, coef, ne, hf, st);
  return hipGetLastError();
}

template <int MINW, int CH = 0, int PRIO = 0, int D = 2, int NW = 8, int BK = 16, int ABL = 0, bool STAMP = false>
inline hipError_t launch_st(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                            hipStream_t s, unsigned long long *stamps = nullptr) {
  if (M == 0) return hipSuccess;
  if (CH != 0 && pcm.ch != static_cast<uint32_t>(CH)) return hipErrorInvalidValue;
  if (STAMP && !stamps) return hipErrorInvalidValue;
  const unsigned m_tiles = (M + 255) / 256;
  hipLaunchKernelGGL((k_mdct_fwd_st<MINW, CH, PRIO, D, NW, BK, ABL, STAMP>), dim3(m_tiles * (kHopI / (8 * NW))), dim3(NW * 64), 0,
                     s, t, pcm, static_cast<long long>(frame_begin), M, coef, stamps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// k_mdct_mx_st: the MATRIX form of the mixed-role transform, for C0 = 384 (ne = 6: 44.1 and 48 kHz) and the channel
// counts of the segment loader.  The exact columns keep k_mdct_fwd_st's arithmetic - the same per-column chain of
// separately rounded multiplies and adds, the table values by scalar loads, mac2rows_st - and the bound columns
// leave the vector ALU: their sums e_k run on the bf16 matrix pipe, which executes beside it (DESIGN section 2,
// glc_kernels.h MatrixBound for the split, the segments and the error budget).
//   tile      128 rows x (96 exact + 160 bound) columns, 1024 threads, one workgroup per CU; workgroup j = 0 .. 3 of
//             a row tile owns exact columns [96 j, 96 j + 96) and bound columns [384 + 160 j, 384 + 160 j + 160)
//   waves     0 .. 11 exact: 8 columns each, the lane's 2 rows (2 lane, 2 lane + 1) - 16 packed operations per i-step,
//             three such waves on every SIMD;  12 .. 15 matrix, one per SIMD: 32 rows x the 160 bound columns as five
//             32 x 32 tiles, 15 v_mfma_f32_32x32x16_bf16 per K-block of 16 i-steps
//   operands  the windowed samples go through the 3-slot LDS ring of k_mdct_fwd_st (a stage = a K-block = 16 i-steps,
//             published by one barrier in the middle of the stage before).  The matrix waves read their rows' 8
//             samples per lane from the same stage, split them into two bf16 pieces (B operand: lane = row), and take
//             the table pieces - A operand, lane = column - from the fragment-ordered image DeviceTables::cos_bf:
//             10 KiB per workgroup and K-block, copied global -> LDS by the matrix waves (global_load_lds_dwordx4, one
//             instruction per fragment) two stages ahead into a 3-slot ring of its own
//   totals    80 accumulators per lane leave no registers for the segment totals at four waves per SIMD: they live in
//             LDS (80 KiB, each matrix wave its own 20 KiB, read-add-written every 8 K-blocks)
//   out       coefficients of the exact columns; hf[j][row] = max |total| over the workgroup's 160 bound columns
//             (+inf where a total is not finite: fmaxf in the quantiser would drop a NaN) - 4 planes - and, from
//             workgroup j = 0, A = sum |x w| at hf[4][row]: 16 partial sums per row (the lane's 8 i of every K-block,
//             then the two lane halves), any order being covered by the screen's slack
// LDS: 24.75 KiB samples + 8 KiB window + 30 KiB table pieces + 80 KiB totals = 142.75 KiB of 160.
// ------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MxOps {  // operands of 4 i-steps of an exact wave: 2 rows of this lane, 8 columns of this wave
  f32x2 a[4];
  u32x8 b[4];
};
template <int II, int AS>
__device__ __forceinline__ void mx_fetch_a(f32x2 &a, unsigned a_addr) {
  asm volatile("ds_read_b64 %0, %1 offset:%c2" : "=&v"(a) : "v"(a_addr), "i"(II * AS * 4) : "memory");
}
template <int II, int AS>
__device__ __forceinline__ void mx_fetch(MxOps &o, unsigned a_addr, const unsigned *brow) {
  st_fetch_b<II>(o.b[0], brow);
  st_fetch_b<II + 1>(o.b[1], brow);
  st_fetch_b<II + 2>(o.b[2], brow);
  st_fetch_b<II + 3>(o.b[3], brow);
  mx_fetch_a<II, AS>(o.a[0], a_addr);
  mx_fetch_a<II + 1, AS>(o.a[1], a_addr);
  mx_fetch_a<II + 2, AS>(o.a[2], a_addr);
  mx_fetch_a<II + 3, AS>(o.a[3], a_addr);
}
__device__ __forceinline__ void mx_wait(MxOps &o) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(o.b[0]), "+s"(o.b[1]), "+s"(o.b[2]), "+s"(o.b[3])::"memory");
  asm volatile("" : "+v"(o.a[0]), "+v"(o.a[1]), "+v"(o.a[2]), "+v"(o.a[3])::"memory");
}
__device__ __forceinline__ void mx_mac(f32x2 (&acc)[2][4], const MxOps &o) {
#pragma unroll
  for (int d = 0; d < 4; ++d) mac2rows_st(acc[0], acc[1], o.a[d], o.b[d].s01, o.b[d].s23, o.b[d].s45, o.b[d].s67);
}
// two f32 -> their bf16 roundings to nearest even, packed (lo in bits 0..15)
__device__ __forceinline__ unsigned mx_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

template <int CH>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_mdct_mx_st(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M, float *__restrict__ coef,
                  float *__restrict__ hf, unsigned long long hf_stride) {
  using MB = MatrixBound;
  static_assert(CH == 1 || CH == 2 || CH == 4 || CH == 8, "segment loader shapes");
  constexpr int BM = MB::kRows, BK = MB::kKBlock, RING = 3, NE = MB::kNe;
  constexpr int kAS = BM + 4;                           // the bank spread of k_mdct_fwd_st's A tile (132 = 4 mod 64)
  constexpr int kExactWaves = 12, kExactCols = 8 * kExactWaves;
  constexpr int kTiles = (kHopI - 64 * NE) / MB::kTile / MB::kGroups;  // 32-column tiles per workgroup: 5
  constexpr int kTilesAll = kTiles * MB::kGroups;
  constexpr int kFrags = kTiles * MB::kPieces;          // 1 KiB fragments per workgroup and K-block: 10
  constexpr int kStages = kFrameI / BK;
  constexpr int kLoaders = BM * BK / 4;                 // lanes of the segment loader: one dwordx4 each
  static_assert(kExactCols * MB::kGroups == 64 * NE && kTiles * MB::kGroups * MB::kTile == kHopI - 64 * NE, "column map");
  static_assert(kLoaders == 512 && kStages % MB::kSegBlocks == 0, "staging shape");
  __shared__ __attribute__((aligned(16))) float As[RING][BK * kAS];
  __shared__ __attribute__((aligned(16))) float Ws[kFrameI];
  __shared__ __attribute__((aligned(16))) uint4 Bt[RING][kFrags * 64];
  __shared__ __attribute__((aligned(16))) f32x4 Tot[4][kTiles * 4][64];

  const int tid = threadIdx.x;
  const unsigned g = xcd_tile<true>();  // 4 workgroups per row tile: any grid
  const int j = g % MB::kGroups;
  const int m0 = (g / MB::kGroups) * BM;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;

  for (int i = tid; i < kFrameI; i += 1024) Ws[i] = tb.window[i];

  const PcmTile a_tile = pcm_tile(pcm, frame_begin, m0, CH);
  const __amdgpu_buffer_rsrc_t a_rsrc = a_tile.rsrc;
  // the segment loader's lanes are waves 0 .. 7, one piece each
  SegLoader<CH, BK, kAS, true> seg(tid, wave < kLoaders / 64);
  {
    const unsigned row0 = m0 + seg.fl * CH;
    if (seg.on && row0 < M)
      seg.off = static_cast<unsigned>((pcm_frame_first(pcm, frame_begin, row0, CH) - a_tile.e_base + seg.o) * 4);
  }
  auto issue_a = [&](int i0) { seg.issue(a_rsrc, static_cast<unsigned>(i0) * static_cast<unsigned>(CH * 4)); };
  auto store_a = [&](int i0, int slot) { seg.store(i0, slot, As, Ws); };
  auto wait_staged = [&]() { seg.wait(); };

  if (wave < kExactWaves) {
    // ---------------------------------------------------------------- exact waves
    f32x2 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = f32x2{0.0f, 0.0f};
    __syncthreads();  // Ws
    issue_a(0);
    wait_staged();
    store_a(0, 0);
    const unsigned a_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&As[0][lane * 2]));
    const int col0 = kExactCols * j + 8 * wave;
    const unsigned *b_base = reinterpret_cast<const unsigned *>(tb.cos_t) + col0;
    issue_a(BK);  // PCM of stage 1 into registers
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    MxOps X, Y;
    mx_fetch<0, kAS>(X, a_lds0, b_base);
    mx_wait(X);
#pragma unroll 1
    for (int s = 0; s < kStages; ++s) {
      __builtin_amdgcn_s_setprio(0);  // half-way between two barriers
      const int slot = s % 3, nslot = (s + 1) % 3;
      const unsigned a_addr = a_lds0 + slot * (BK * kAS * 4);
      const unsigned a_next = a_lds0 + nslot * (BK * kAS * 4);
      const unsigned *brow = b_base + static_cast<size_t>(s) * (BK * kHopI);
      const unsigned *brow_next = b_base + static_cast<size_t>((s + 1) & (kStages - 1)) * (BK * kHopI);
      mx_fetch<4, kAS>(Y, a_addr, brow);
      mx_mac(acc, X);
      mx_wait(Y);
      mx_fetch<8, kAS>(X, a_addr, brow);
      mx_mac(acc, Y);
      // the hand-off, as in st_body: the PCM registers of stage s+1 -> LDS, barrier, PCM loads of stage s+2
      wait_staged();
      store_a(((s + 1) & (kStages - 1)) * BK, nslot);
      mx_wait(X);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
      issue_a(((s + 2) & (kStages - 1)) * BK);
      mx_fetch<12, kAS>(Y, a_addr, brow);
      mx_mac(acc, X);
      mx_wait(Y);
      mx_fetch<0, kAS>(X, a_next, brow_next);
      mx_mac(acc, Y);
      mx_wait(X);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the wrap-around prefetch
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned row = m0 + lane * 2 + r;
      if (row >= M) continue;
      float *dst = coef + static_cast<size_t>(row) * kHopI + col0;
      float4 o;
      o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
      o.z = mul_rn(acc[r][1].x, tb.norm); o.w = mul_rn(acc[r][1].y, tb.norm);
      *reinterpret_cast<float4 *>(dst) = o;
      o.x = mul_rn(acc[r][2].x, tb.norm); o.y = mul_rn(acc[r][2].y, tb.norm);
      o.z = mul_rn(acc[r][3].x, tb.norm); o.w = mul_rn(acc[r][3].y, tb.norm);
      *reinterpret_cast<float4 *>(dst + 4) = o;
    }
    return;
  }

  // ------------------------------------------------------------------ matrix waves
  __builtin_amdgcn_s_setprio(3);  // little to issue, and the other twelve waves wait for it at every barrier
  const int mw = wave - kExactWaves, half = lane >> 5, idx = lane & 31;
  f32x16 acc[kTiles];
#pragma unroll
  for (int c = 0; c < kTiles; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[c][e] = 0.0f;
#pragma unroll
  for (int q = 0; q < kTiles * 4; ++q) Tot[mw][q][lane] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the workgroup's fragments of K-block kb are 10 consecutive KiB of the image; this wave copies mw, mw + 4, mw + 8
  const uint4 *img = reinterpret_cast<const uint4 *>(tb.cos_bf) + static_cast<size_t>(kTiles * j * MB::kPieces) * 64 + lane;
  auto issue_t = [&](int kb, int slot) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int fr = mw + 4 * q;
      if (fr < kFrags)
        __builtin_amdgcn_global_load_lds(img + (static_cast<size_t>(kb) * (kTilesAll * MB::kPieces) + fr) * 64, &Bt[slot][fr * 64],
                                         16, 0, 0);
    }
  };
  __syncthreads();  // Ws
  issue_t(0, 0);
  issue_t(1, 1);
  issue_a(BK);  // (no loader among the matrix waves: the calls keep the two roles' hand-offs alike)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  float asum = 0.0f;
#pragma unroll 1
  for (int s = 0; s < kStages; ++s) {
    const int slot = s % 3;
    // this lane's row 32 mw + idx, i-steps 8 half .. 8 half + 7 of the K-block
    const float *ax = &As[slot][(8 * half) * kAS + 32 * mw + idx];
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = ax[e * kAS];
    u32x4 hi, lo;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      asum = add_rn(asum, add_rn(__builtin_fabsf(x[2 * p]), __builtin_fabsf(x[2 * p + 1])));
      const unsigned h = mx_cvt_pk_bf16(x[2 * p], x[2 * p + 1]);
      hi[p] = h;
      // a - a1 is exact in f32 (a1 holds the leading 8 bits of a, rounded)
      const float r0 = add_rn(x[2 * p], -__builtin_bit_cast(float, h << 16));
      const float r1 = add_rn(x[2 * p + 1], -__builtin_bit_cast(float, h & 0xFFFF0000u));
      lo[p] = mx_cvt_pk_bf16(r0, r1);
    }
    const bf16x8 x1 = __builtin_bit_cast(bf16x8, hi), x2 = __builtin_bit_cast(bf16x8, lo);
#pragma unroll
    for (int c = 0; c < kTiles; ++c) {
      const bf16x8 t1 = __builtin_bit_cast(bf16x8, Bt[slot][(2 * c) * 64 + lane]);
      const bf16x8 t2 = __builtin_bit_cast(bf16x8, Bt[slot][(2 * c + 1) * 64 + lane]);
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(t1, x1, acc[c], 0, 0, 0);
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(t2, x1, acc[c], 0, 0, 0);
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(t1, x2, acc[c], 0, 0, 0);
    }
    if (s % MB::kSegBlocks == MB::kSegBlocks - 1) {  // the segment ends: total += accumulator, accumulator = 0
#pragma unroll
      for (int c = 0; c < kTiles; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          f32x4 t = Tot[mw][c * 4 + v][lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            t[e] = add_rn(t[e], acc[c][v * 4 + e]);
            acc[c][v * 4 + e] = 0.0f;
          }
          Tot[mw][c * 4 + v][lane] = t;
        }
    }
    // the hand-off (the exact waves' is in the middle of their stage s): stage s+1's samples were staged by waves
    // 0 .. 7; this wave's table pieces of stage s+1 have landed; behind the barrier the pieces of stage s+2 set out
    // into the slot stage s-1 was read from
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue_t((s + 2) & (kStages - 1), (s + 2) % 3);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the wrap-around prefetch
  float h = 0.0f;
  bool bad = false;
#pragma unroll
  for (int q = 0; q < kTiles * 4; ++q) {
    const f32x4 t = Tot[mw][q][lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = __builtin_fabsf(t[e]);
      bad = bad || !(a <= 3.4028234663852886e38f);  // an infinity or a NaN: the row must fail
      h = fmaxf(h, a);
    }
  }
  if (bad) h = __builtin_inff();
  h = fmaxf(h, __shfl_xor(h, 32));
  asum = add_rn(asum, __shfl_xor(asum, 32));
  if (half == 0) {
    const size_t at = static_cast<size_t>(m0) + 32 * mw + idx;
    hf[static_cast<unsigned>(j) * hf_stride + at] = h;
    if (j == 0) hf[static_cast<unsigned>(MB::kGroups) * hf_stride + at] = asum;
  }
}

template <int CH>
inline hipError_t launch_mx_st(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                               float *hf, uint64_t hf_stride, hipStream_t s) {
  if (M == 0) return hipSuccess;
  if (pcm.ch != static_cast<uint32_t>(CH) || !t.cos_bf) return hipErrorInvalidValue;
  if (hf_stride < (M + MatrixBound::kRows - 1) / MatrixBound::kRows * MatrixBound::kRows) return hipErrorInvalidValue;
  const dim3 grid((M + MatrixBound::kRows - 1) / MatrixBound::kRows * MatrixBound::kGroups), block(1024);
  const unsigned long long st = hf_stride;
  hipLaunchKernelGGL((k_mdct_mx_st<CH>), grid, block, 0, s, t, pcm, static_cast<long long>(frame_begin), M, coef, hf, st);
  return hipGetLastError();
}


// ------------------------------------------------------------------------------------------
// Short clips (<= 1792 rows: BASELINE config 1 and every clip of the reference's own tests).  A launch
// this small cannot fill the chip; what it costs is ONE wave's chain of 2048 dependent i-steps, and the
// length of a step is the lane tile: 128 VALU cycles for 4 x 8 outputs, 16 for 2 x 2.  So the tile is
// cut until every SIMD of the chip has a wave of its own - 2 x 2 outputs per lane up to 256 rows, 2 x 4
// up to 512 (65 536 lanes either way) - in 256-thread workgroups (one wave per SIMD of a CU) on
// 32 x 32 / 32 x 64 tiles.  Same arithmetic, same order; hand-scheduled like the large kernels:
// operands come from LDS through a four-deep register ring with counted lgkmcnt waits (LDS returns in
// order), the next stage's global loads are in flight during the stage and only waited for at its end.
// (Round 2 left this range to hipcc on a 4 x 4 lane tile: 129 VGPRs + 80 B of scratch, 0.13 ms at 172 rows.)
// ------------------------------------------------------------------------------------------
#ifndef GLC_SMALL_PAIR
#define GLC_SMALL_PAIR 1  // k_mdct_fwd_small waits for its LDS operands once per two i-steps (tuning: k1_tune)
#endif
#ifndef GLC_SMALL_BK
#define GLC_SMALL_BK 32  // i-steps per LDS stage of k_mdct_fwd_small (64 measured 4 % slower: gpurun r3d2)
#endif
template <int TN>
struct SmallOps {  // operands of one i-step: a = 2 rows, b = TN columns
  f32x2 a;
  f32x2 b[TN / 2];
};

template <int TN, int BM, int BN>
__device__ __forceinline__ void small_fetch(SmallOps<TN> &o, unsigned a_addr, unsigned b_addr, int ii) {
  if constexpr (TN == 2) {
    asm volatile(
        "ds_read_b64 %0, %2 offset:%c4\n\t"
        "ds_read_b64 %1, %3 offset:%c5"
        : "=&v"(o.a), "=&v"(o.b[0])
        : "v"(a_addr), "v"(b_addr), "i"(ii * BM * 4), "i"(ii * BN * 4)
        : "memory");
  } else {
    asm volatile(
        "ds_read_b64 %0, %3 offset:%c5\n\t"
        "ds_read_b64 %1, %4 offset:%c6\n\t"
        "ds_read_b64 %2, %4 offset:%c7"
        : "=&v"(o.a), "=&v"(o.b[0]), "=&v"(o.b[1])
        : "v"(a_addr), "v"(b_addr), "i"(ii * BM * 4), "i"(ii * BN * 4), "i"(ii * BN * 4 + 8)
        : "memory");
  }
}

// wait until at most PENDING of this wave's LDS reads are outstanding, i.e. `o` (older than those) has landed
template <int TN, int PENDING>
__device__ __forceinline__ void small_wait(SmallOps<TN> &o) {
  if constexpr (TN == 2)
    asm volatile("s_waitcnt lgkmcnt(%c2)" : "+v"(o.a), "+v"(o.b[0]) : "i"(PENDING) : "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(%c3)" : "+v"(o.a), "+v"(o.b[0]), "+v"(o.b[1]) : "i"(PENDING) : "memory");
}

// c[r][j] += a_r * b_j: rows (a.x, a.y) x TN columns, multiply and add separately rounded
template <int TN>
__device__ __forceinline__ void small_mac(f32x2 (&acc)[2][TN / 2], const SmallOps<TN> &o) {
  if constexpr (TN == 2) {
    f32x2 t0, t1;
    asm volatile(
        "v_pk_mul_f32 %2, %4, %5 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %4, %5 op_sel:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\t"
        "v_pk_add_f32 %1, %1, %3"
        : "+v"(acc[0][0]), "+v"(acc[1][0]), "=&v"(t0), "=&v"(t1)
        : "v"(o.a), "v"(o.b[0]));
  } else {
    f32x2 t0, t1, t2, t3;
    asm volatile(
        "v_pk_mul_f32 %4, %8, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %5, %8, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %6, %8, %9 op_sel:[1,0]\n\t"
        "v_pk_mul_f32 %7, %8, %10 op_sel:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %4\n\t"
        "v_pk_add_f32 %1, %1, %5\n\t"
        "v_pk_add_f32 %2, %2, %6\n\t"
        "v_pk_add_f32 %3, %3, %7"
        : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
        : "v"(o.a), "v"(o.b[0]), "v"(o.b[1]));
  }
}

// i-steps II .. BK-1 of a stage, written out at compile time: wait for the oldest step of the ring
// (LDS returns in order: all but the younger steps' reads must have landed), use it, refill its slot
template <int TN, int BM, int BN, int BK, int D, int II>
__device__ __forceinline__ void small_steps(f32x2 (&acc)[2][TN / 2], SmallOps<TN> (&ring)[D], unsigned a_addr, unsigned b_addr) {
  if constexpr (II < BK) {
    constexpr int R = 1 + TN / 2;
#if GLC_SMALL_PAIR
    // two i-steps per wait: one s_waitcnt and one burst of LDS reads per 2 x 4 vector ops
    static_assert(BK % 2 == 0 && D % 2 == 0, "pairs");
    constexpr int younger = II + D <= BK ? D - 2 : BK - 2 - II;  // steps behind II + 1 still in flight
    static_assert(younger * R <= 15, "lgkmcnt is a 4-bit counter");
    small_wait<TN, younger * R>(ring[(II + 1) % D]);
    asm volatile("" : "+v"(ring[II % D].a), "+v"(ring[II % D].b[0]));  // (II landed before II + 1: LDS returns in order)
    if constexpr (TN == 4) asm volatile("" : "+v"(ring[II % D].b[1]));
    small_mac<TN>(acc, ring[II % D]);
    small_mac<TN>(acc, ring[(II + 1) % D]);
    if constexpr (II + D < BK) {
      small_fetch<TN, BM, BN>(ring[II % D], a_addr, b_addr, II + D);
      small_fetch<TN, BM, BN>(ring[(II + 1) % D], a_addr, b_addr, II + D + 1);
    }
    small_steps<TN, BM, BN, BK, D, II + 2>(acc, ring, a_addr, b_addr);
#else
    constexpr int younger = II + D <= BK ? D - 1 : BK - 1 - II;
    static_assert(younger * R <= 15, "lgkmcnt is a 4-bit counter");
    small_wait<TN, younger * R>(ring[II % D]);
    small_mac<TN>(acc, ring[II % D]);
    if constexpr (II + D < BK) small_fetch<TN, BM, BN>(ring[II % D], a_addr, b_addr, II + D);
    small_steps<TN, BM, BN, BK, D, II + 1>(acc, ring, a_addr, b_addr);
#endif
  }
}

// REPAIR (k_mdct_fwd_small_cols): only the coefficient tiles [n_tile0, n_tile0 + n_cnt) of the launch's rows, and
// of those only the row tiles that hold a flagged row (row_flag[M], written by the screened quantiser): the exact
// columns C0.. of the rows that failed the screen.  Every wave reads the tile's 32 flags itself, so the whole
// workgroup leaves together, before its first barrier.
template <int TN, bool REPAIR>
__device__ __forceinline__ void small_body(const DeviceTables &tb, const PcmView &pcm, long long frame_begin, unsigned M,
                                           float *__restrict__ coef, const unsigned *__restrict__ row_flag,
                                           unsigned n_tile0, unsigned n_cnt) {
  // D: i-steps of operands in flight (an LDS read takes ~250 cycles under no load, a 2 x 2 step 16 of VALU:
  // the ring is as deep as the 4-bit lgkmcnt allows - 7 x 2 or 5 x 3 younger reads)
  constexpr int BM = 32, BN = 16 * TN, BK = GLC_SMALL_BK, D = TN == 2 ? 8 : 6;
  constexpr int kNTiles = kHopI / BN;
  constexpr int kAStride = 8, kAPer = BK / kAStride;     // 256 threads = 32 rows x 8 i; i = a_i + 8 j
  constexpr int kBRowsPer = 256 / (BN / 4), kBPer = BK / kBRowsPer;
  static_assert(TN == 2 || TN == 4, "lane tile");
  __shared__ __attribute__((aligned(16))) float As[2][BK * BM];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * BN];

  const int tid = threadIdx.x;
  const int n_tile = REPAIR ? static_cast<int>(n_tile0 + blockIdx.x % n_cnt) : static_cast<int>(blockIdx.x % kNTiles);
  const int m_tile = REPAIR ? static_cast<int>(blockIdx.x / n_cnt) : static_cast<int>(blockIdx.x / kNTiles);
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int tx = tid % 16, ty = tid / 16;
  if constexpr (REPAIR) {
    const unsigned fr = static_cast<unsigned>(m0) + (tid & 31);
    const bool flagged = fr < M && row_flag[fr] == 1u;  // (2: an edge row, the side stream's)
    if (__ballot(flagged) == 0ull) return;
  }

  // A operand: the per-row loader, builtin form
  const long long ch = pcm.ch;
  const PcmTile a_tile = pcm_tile(pcm, frame_begin, m0, pcm.ch);
  const __amdgpu_buffer_rsrc_t a_rsrc = a_tile.rsrc;  // (what the stage lambdas take: a_tile stays out of their captures)
  const int a_r = tid % BM, a_i = tid / BM;
  unsigned a_off = kPcmNoRow;
  pcm_row_origin(a_off, pcm, a_tile, frame_begin, m0 + a_r, M, pcm.ch, a_i);
  const unsigned a_step = static_cast<unsigned>(kAStride * ch * 4);
  const float *w_ptr = tb.window + a_i;
  const int b_r = tid / (BN / 4), b_c4 = tid % (BN / 4);
  const float *b_ptr = tb.cos_t + n0 + static_cast<size_t>(b_r) * kHopI + b_c4 * 4;

  float a_raw[kAPer], a_win[kAPer];
  f32x4 b_stage[kBPer];
  auto load_stage = [&](int i0) {
    pcm_load_rows(a_raw, a_rsrc, a_off + static_cast<unsigned>(i0) * static_cast<unsigned>(ch * 4), a_step);
#pragma unroll
    for (int j = 0; j < kAPer; ++j) a_win[j] = w_ptr[i0 + kAStride * j];
#pragma unroll
    for (int j = 0; j < kBPer; ++j)
      b_stage[j] = *reinterpret_cast<const f32x4 *>(b_ptr + static_cast<size_t>(i0 + kBRowsPer * j) * kHopI);
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < kAPer; ++j) {
      float r = a_raw[j], w = a_win[j];
      asm volatile("" : "+v"(r), "+v"(w));  // first use of the staged registers stays behind the stage's math
      As[buf][(a_i + kAStride * j) * BM + a_r] = mul_rn(r, w);  // block[i] = slice[i]*window[i], :480
    }
#pragma unroll
    for (int j = 0; j < kBPer; ++j) {
      f32x4 b = b_stage[j];
      asm volatile("" : "+v"(b));
      *reinterpret_cast<f32x4 *>(&Bs[buf][(b_r + kBRowsPer * j) * BN + b_c4 * 4]) = b;
    }
  };

  f32x2 acc[2][TN / 2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < TN / 2; ++c) acc[r][c] = f32x2{0.0f, 0.0f};  // `let mut s = 0.0f32`, :365

  load_stage(0);
  store_stage(0);
  __syncthreads();

  const unsigned a_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&As[0][ty * 2]));
  const unsigned b_lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&Bs[0][tx * TN]));
  constexpr int kStages = kFrameI / BK;
#pragma unroll 1
  for (int s = 0; s < kStages; ++s) {
    const int buf = s & 1;
    load_stage(((s + 1) & (kStages - 1)) * BK);  // (the last iteration re-fetches stage 0 into the idle buffer)
    const unsigned a_addr = a_lds0 + buf * (BK * BM * 4);
    const unsigned b_addr = b_lds0 + buf * (BK * BN * 4);
    SmallOps<TN> ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) small_fetch<TN, BM, BN>(ring[d], a_addr, b_addr, d);
    small_steps<TN, BM, BN, BK, D, 0>(acc, ring, a_addr, b_addr);
    store_stage(buf ^ 1);
    __syncthreads();
  }

  // epilogue: out[k] = s * norm, :372
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned row = m0 + ty * 2 + r;
    if (row >= M) continue;
    float *dst = coef + static_cast<size_t>(row) * kHopI + n0 + tx * TN;
    if constexpr (TN == 2) {
      float2 o;
      o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
      *reinterpret_cast<float2 *>(dst) = o;
    } else {
      float4 o;
      o.x = mul_rn(acc[r][0].x, tb.norm); o.y = mul_rn(acc[r][0].y, tb.norm);
      o.z = mul_rn(acc[r][1].x, tb.norm); o.w = mul_rn(acc[r][1].y, tb.norm);
      *reinterpret_cast<float4 *>(dst) = o;
    }
  }
}

template <int TN>
__global__ __launch_bounds__(256) void k_mdct_fwd_small(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M,
                                                         float *__restrict__ coef) {
  small_body<TN, false>(tb, pcm, frame_begin, M, coef, nullptr, 0u, 0u);
}

template <int TN>
__global__ __launch_bounds__(256) void k_mdct_fwd_small_cols(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M,
                                                              float *__restrict__ coef, const unsigned *__restrict__ row_flag,
                                                              unsigned n_tile0, unsigned n_cnt) {
  small_body<TN, true>(tb, pcm, frame_begin, M, coef, row_flag, n_tile0, n_cnt);
}

// columns [col0, 1024) (col0 a multiple of the tile width) of the flagged rows' tiles
template <int TN>
inline hipError_t launch_small_cols(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                                    const unsigned *row_flag, uint32_t col0, hipStream_t s) {
  constexpr unsigned BN = 16 * TN;
  if (M == 0 || col0 >= static_cast<uint32_t>(kHopI)) return hipSuccess;
  if (col0 % BN || !row_flag) return hipErrorInvalidValue;
  const unsigned m_tiles = (M + 31) / 32, n_cnt = (kHopI - col0) / BN;
  hipLaunchKernelGGL((k_mdct_fwd_small_cols<TN>), dim3(m_tiles * n_cnt), dim3(256), 0, s, t, pcm,
                     static_cast<long long>(frame_begin), M, coef, row_flag, col0 / BN, n_cnt);
  return hipGetLastError();
}

template <int TN>
inline hipError_t launch_small(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                               hipStream_t s) {
  if (M == 0) return hipSuccess;
  const unsigned m_tiles = (M + 31) / 32;
  hipLaunchKernelGGL((k_mdct_fwd_small<TN>), dim3(m_tiles * (kHopI / (16 * TN))), dim3(256), 0, s, t, pcm,
                     static_cast<long long>(frame_begin), M, coef);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// k_mdct_fwd_small_rows: the repair of a launch in which FEW rows failed the screen (launch_encode_screened), built
// for latency.  What such a launch costs is one wave's chain of 2048 dependent adds per accumulator, so everything
// else is kept off that chain:
//   work item   R consecutive entries of the list of failed rows x one slab of 64 columns >= col0; one wave (a
//               workgroup of its own: the slabs of a row group run on different CUs, each pulling only its own
//               512 KiB of the table through its L1).  A lane owns ONE column and carries R accumulators, two to a
//               packed register: an i-step is R / 2 v_pk_mul_f32 and R / 2 v_pk_add_f32, separately rounded.
//   rows        the group's windowed rows, fl(x w), staged once in LDS ([pair][i][2]); the wave reads them as
//               broadcasts, 16 i-steps ahead.
//   table       tb.cos ([k][i], the values of cos_t bit for bit): a lane streams its own row with dwordx4 loads,
//               four i-steps each, 28 loads (112 i-steps) in flight - more than an Infinity-Cache round trip at the
//               step length reached; no LDS tile, no transposition, no address arithmetic inside the loop.
//   finding it  the grid is fixed.  Every wave sums the per-wave fail counts the screened quantiser left (lane l owns
//               a contiguous run of them), leaves if the sum is 0, and otherwise finds entry j of the list where the
//               running sum passes j: no atomics, no workspace of its own, nothing to clear.  Workgroups stride over
//               the items, so any number of failed rows is handled; every barrier is workgroup-uniform.
// Same products, same ascending-i adds, one accumulator per output: the bytes small_body writes.
// ------------------------------------------------------------------------------------------
constexpr int kRowsGrid = 1024;  // workgroups of a launch, whatever M: one wave per SIMD of the chip
#ifndef GLC_SMALL_ROWS_R
#define GLC_SMALL_ROWS_R 2  // failed rows of a work item: 2 or 4 (measured equal at four failed rows, profiles/encode_repair_bench.txt section 6; 2 is a stereo frame)
#endif
constexpr unsigned kRowsSlab = 64;  // columns of a work item: one per lane

// four table loads (16 i-steps) of this lane's row, `byte_off` from tp
__device__ __forceinline__ void rows_issue_t(f32x4 (&t)[4], const float *tp, int byte_off) {
  asm volatile(
      "global_load_dwordx4 %0, %4, off offset:%c5\n\t"
      "global_load_dwordx4 %1, %4, off offset:%c6\n\t"
      "global_load_dwordx4 %2, %4, off offset:%c7\n\t"
      "global_load_dwordx4 %3, %4, off offset:%c8"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
      : "v"(tp), "i"(byte_off), "i"(byte_off + 16), "i"(byte_off + 32), "i"(byte_off + 48)
      : "memory");
}

// wait until at most PENDING of this wave's table loads are outstanding (they return in order): `t` has landed
template <int PENDING>
__device__ __forceinline__ void rows_wait_t(f32x4 (&t)[4]) {
  asm volatile("s_waitcnt vmcnt(%c4)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]) : "i"(PENDING) : "memory");
}

template <int NP>
struct RowsX {  // the windowed samples of 16 i-steps: per pair of rows, 8 x {a_i, b_i, a_i+1, b_i+1}
  f32x4 v[NP][8];
};

template <int NP>
__device__ __forceinline__ void rows_issue_x(RowsX<NP> &x, unsigned xa, int byte_off) {
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int o = byte_off + p * kFrameI * 8;
    asm volatile(
        "ds_read_b128 %0, %8 offset:%c9\n\t"
        "ds_read_b128 %1, %8 offset:%c10\n\t"
        "ds_read_b128 %2, %8 offset:%c11\n\t"
        "ds_read_b128 %3, %8 offset:%c12\n\t"
        "ds_read_b128 %4, %8 offset:%c13\n\t"
        "ds_read_b128 %5, %8 offset:%c14\n\t"
        "ds_read_b128 %6, %8 offset:%c15\n\t"
        "ds_read_b128 %7, %8 offset:%c16"
        : "=&v"(x.v[p][0]), "=&v"(x.v[p][1]), "=&v"(x.v[p][2]), "=&v"(x.v[p][3]), "=&v"(x.v[p][4]), "=&v"(x.v[p][5]),
          "=&v"(x.v[p][6]), "=&v"(x.v[p][7])
        : "v"(xa), "i"(o), "i"(o + 16), "i"(o + 32), "i"(o + 48), "i"(o + 64), "i"(o + 80), "i"(o + 96), "i"(o + 112)
        : "memory");
  }
}

template <int NP>
__device__ __forceinline__ void rows_wait_x(RowsX<NP> &x) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int p = 0; p < NP; ++p)
    asm volatile(""
                 : "+v"(x.v[p][0]), "+v"(x.v[p][1]), "+v"(x.v[p][2]), "+v"(x.v[p][3]), "+v"(x.v[p][4]), "+v"(x.v[p][5]),
                   "+v"(x.v[p][6]), "+v"(x.v[p][7])::"memory");
}

// four i-steps of one pair of rows: acc = {s_a, s_b}; xa = {a_i, b_i, a_i+1, b_i+1}, xb the next two; t = T[k][i .. i+3].
// Each product is rounded, then added: the multiply of a step is issued ahead of the add of the step before it.
__device__ __forceinline__ void rows_mac4(f32x2 &acc, f32x4 xa, f32x4 xb, f32x4 t) {
  const f32x2 x0 = __builtin_shufflevector(xa, xa, 0, 1), x1 = __builtin_shufflevector(xa, xa, 2, 3);
  const f32x2 x2 = __builtin_shufflevector(xb, xb, 0, 1), x3 = __builtin_shufflevector(xb, xb, 2, 3);
  const f32x2 t01 = __builtin_shufflevector(t, t, 0, 1), t23 = __builtin_shufflevector(t, t, 2, 3);
  f32x2 p0, p1, p2, p3;
  asm volatile(
      "v_pk_mul_f32 %1, %5, %9 op_sel_hi:[1,0]\n\t"
      "v_pk_mul_f32 %2, %6, %9 op_sel:[0,1]\n\t"
      "v_pk_add_f32 %0, %0, %1\n\t"
      "v_pk_mul_f32 %3, %7, %10 op_sel_hi:[1,0]\n\t"
      "v_pk_add_f32 %0, %0, %2\n\t"
      "v_pk_mul_f32 %4, %8, %10 op_sel:[0,1]\n\t"
      "v_pk_add_f32 %0, %0, %3\n\t"
      "v_pk_add_f32 %0, %0, %4"
      : "+v"(acc), "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
      : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(t01), "v"(t23));
}

// FROM_ARGS: the list is not found but given - `er`, the launch's edge rows [0, n_pre) and [suf0, M) (glc_kernels.h
// edge_rows), entry j being row j or suf0 + (j - n_pre).  No scan, no walk, no flag load: row_flag and wave_fail are
// not read, and the grid is exactly the items.  `coef` is then not the launch's workspace but a buffer of the list's
// own, [er.n][1024]: entry j's coefficients go to its row j (with col0 = 0 all 1024 of them, so that nothing of the
// launch's transform is needed to quantise the row).
// NB: blocks of 16 i-steps in the ring of table registers (NB - 1 of them, 4 loads each, in flight): 8 is the latency
// form (28 loads, 128 registers of table values); 4 is the capped form of the edge transform (12 loads, 64 registers),
// which has to fit on a SIMD beside two resident waves of the screened quantiser.
template <int R, bool FROM_ARGS, int NB = 8>
__device__ __forceinline__ void small_rows_body(const DeviceTables &tb, const PcmView &pcm, long long frame_begin, unsigned M,
                                                float *__restrict__ coef, const unsigned *__restrict__ row_flag,
                                                const unsigned *__restrict__ wave_fail, unsigned col0, const EdgeRows er) {
  static_assert(R == 2 || R == 4, "rows of a group: whole packed pairs");
  constexpr int NP = R / 2;
  constexpr unsigned kNone = 0xFFFFFFFFu;
  __shared__ __attribute__((aligned(16))) float xs[NP * kFrameI * 2];  // [pair][i][2]
  __shared__ unsigned s_row[R], s_total;
  const unsigned lane = threadIdx.x;

  // the list of failed rows, implicitly: lane l owns the counts of quantiser waves [l per, (l + 1) per), 4 rows each
  const unsigned n_w = (M + 15u) / 16u * 4u;  // the counts k_quantize_screen<*, 1> wrote: a multiple of 4
  const unsigned per = ((n_w + 63u) / 64u + 3u) & ~3u;
  const unsigned w0 = lane * per;
  const uint4 *wf4 = reinterpret_cast<const uint4 *>(wave_fail);
  // the four counts at word w of this lane's run, 0 beyond the run or the launch: an unconditional load, so that a
  // trip's eight are in flight together (a wave that waited for each would spend a memory round trip per load)
  auto counts = [&](unsigned w) -> uint4 {
    const bool in = w < per && w0 + w < n_w;
    const uint4 c = wf4[in ? (w0 + w) >> 2 : 0u];
    return in ? c : uint4{0u, 0u, 0u, 0u};
  };
  unsigned cnt = 0, base = 0, n_fail = er.n;
  if constexpr (!FROM_ARGS) {
    for (unsigned w = 0; w < per; w += 32) {
      uint4 c[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) c[k] = counts(w + 4 * k);
#pragma unroll
      for (int k = 0; k < 8; ++k) cnt += c[k].x + c[k].y + c[k].z + c[k].w;
    }
    unsigned incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_up(incl, off);
      if (lane >= static_cast<unsigned>(off)) incl += v;
    }
    if (lane == 63) s_total = incl;
    __syncthreads();
    n_fail = __builtin_amdgcn_readfirstlane(s_total);
    base = incl - cnt;
  }
  if (n_fail == 0) return;  // nothing failed: the whole launch leaves here

  const unsigned n_slabs = (static_cast<unsigned>(kHopI) - col0) / kRowsSlab;
  const unsigned n_items = (n_fail + R - 1) / R * n_slabs;
  const long long e_end = pcm_end(pcm, pcm.ch);
  const unsigned xs0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(&xs[0]));

#pragma unroll 1
  for (unsigned item = blockIdx.x; item < n_items; item += gridDim.x) {
    const unsigned g = item / n_slabs, slab = item - g * n_slabs;
    // entries g R .. g R + R - 1 of the list: the lane whose run of counts holds entry j walks it to the wave, then
    // that wave's four flags to the row
    unsigned m[R];
    if constexpr (FROM_ARGS) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const unsigned j = g * R + q;
        m[q] = j >= er.n ? kNone : j < er.n_pre ? j : er.suf0 + (j - er.n_pre);
      }
      __syncthreads();  // the item before this one has read its rows out of xs
    } else {
    if (lane < R) s_row[lane] = kNone;
    __syncthreads();
    if (cnt != 0 && g * R + R > base && g * R < base + cnt) {
      unsigned run = base, word[R], rank[R];
#pragma unroll
      for (int q = 0; q < R; ++q) word[q] = kNone, rank[q] = 0;
      for (unsigned w = 0; w < per; w += 32) {
        uint4 c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = counts(w + 4 * k);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned ce[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
              const unsigned j = g * R + q;
              if (j >= run && j < run + ce[e]) word[q] = w0 + w + 4 * k + e, rank[q] = j - run;
            }
            run += ce[e];
          }
        }
      }
      // the four flags of each wave found: one aligned load (row_flag holds a multiple of 256 entries), all in flight
      uint4 f4[R];
#pragma unroll
      for (int q = 0; q < R; ++q) f4[q] = *reinterpret_cast<const uint4 *>(row_flag + (word[q] != kNone ? word[q] * 4u : 0u));
#pragma unroll
      for (int q = 0; q < R; ++q)
        if (word[q] != kNone) {
          const unsigned fl[4] = {f4[q].x, f4[q].y, f4[q].z, f4[q].w};
          unsigned seen = 0;
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (word[q] * 4u + e < M && fl[e] == 1u) {  // (2: an edge row, the side stream's)
              if (seen == rank[q]) s_row[q] = word[q] * 4u + e;
              ++seen;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < R; ++q) m[q] = __builtin_amdgcn_readfirstlane(s_row[q]);
    }

    // fl(x w) of the group's rows -> LDS.  Each row is read through a buffer descriptor of its own, based at the row's
    // first element, whose range check is the encoder's zero padding as PcmTile's is - so every load is unconditional
    // and all of them are issued before the first LDS write: one memory round trip for the whole group, not one per sample
    constexpr int kPer = kFrameI / 64;
    float wv[kPer], xv[R][kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) wv[t] = tb.window[lane + 64 * t];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const bool live = m[q] != kNone;
      const long long f = frame_begin + (live ? m[q] / pcm.ch : 0u);
      const long long e_row =
          (f * kHopI - kHopI / 2 - static_cast<long long>(pcm.t0)) * static_cast<long long>(pcm.ch) + (live ? m[q] % pcm.ch : 0u);
      const long long e_base = e_row < 0 ? 0 : e_row;
      // (a row the list does not have: nothing in range, all zeros)
      const __amdgpu_buffer_rsrc_t rsrc = pcm_rsrc(pcm, e_base, live ? e_end - e_base : 0);
      const unsigned off0 = static_cast<unsigned>((e_row - e_base) * 4);  // 0, or negative: wraps, that IS the padding
#pragma unroll
      for (int t = 0; t < kPer; ++t)
        xv[q][t] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off0 + (lane + 64u * t) * (pcm.ch * 4u), 0, 0));
    }
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int t = 0; t < kPer; ++t)
        xs[((q >> 1) * kFrameI + static_cast<int>(lane) + 64 * t) * 2 + (q & 1)] = mul_rn(xv[q][t], wv[t]);  // block[i] = slice[i]*window[i], :480
    __syncthreads();

    // the chain: 16 rounds of 8 blocks of 16 i-steps; 7 blocks of table loads in flight, the rows a block ahead
    const unsigned col = col0 + slab * kRowsSlab + lane;
    const float *row_t = tb.cos + static_cast<size_t>(col) * kFrameI;
    const float *tp = row_t;
    unsigned xa = xs0;
    f32x2 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = f32x2{0.0f, 0.0f};  // `let mut s = 0.0f32`, :365
    static_assert(NB == 4 || NB == 8, "an even ring that divides the 128 blocks of a row");
    f32x4 T[NB][4];
    RowsX<NP> X[2];
#pragma unroll
    for (int b = 0; b < NB - 1; ++b) rows_issue_t(T[b], tp, b * 64);
    rows_issue_x<NP>(X[0], xa, 0);
    rows_wait_x<NP>(X[0]);
    constexpr int kRounds = kFrameI / (16 * NB);
#pragma unroll 1
    for (int round = 0; round < kRounds; ++round) {
      // (the last round's look-ahead wraps to i = 0: in bounds, never used)
      const float *tp_next = round + 1 < kRounds ? tp + 16 * NB : row_t;
      const unsigned xa_next = round + 1 < kRounds ? xa + 16 * NB * 8 : xs0;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        rows_wait_t<4 * (NB - 2)>(T[b]);
        if (b == 0) rows_issue_t(T[NB - 1], tp, (NB - 1) * 64);
        else rows_issue_t(T[b - 1], tp_next, (b - 1) * 64);
        if (b < NB - 1) rows_issue_x<NP>(X[(b + 1) & 1], xa, (b + 1) * 128);
        else rows_issue_x<NP>(X[0], xa_next, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int p = 0; p < NP; ++p) rows_mac4(acc[p], X[b & 1].v[p][2 * j], X[b & 1].v[p][2 * j + 1], T[b][j]);
        rows_wait_x<NP>(X[(b + 1) & 1]);
      }
      tp = tp_next;
      xa = xa_next;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the wrap-around look-ahead

    // epilogue: out[k] = s * norm, :372
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (m[q] != kNone)
        coef[static_cast<size_t>(FROM_ARGS ? g * R + q : m[q]) * kHopI + col] = mul_rn(q & 1 ? acc[q >> 1].y : acc[q >> 1].x, tb.norm);
    // (the argument form's grid is exactly its items: one pass, so that nothing of the staging - 32 offsets, 32 window
    // values - is kept in registers through the chain for a next item)
    if constexpr (FROM_ARGS) break;
  }
}

template <int R>
__global__ __launch_bounds__(64) void k_mdct_fwd_small_rows(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M,
                                                             float *__restrict__ coef, const unsigned *__restrict__ row_flag,
                                                             const unsigned *__restrict__ wave_fail, unsigned col0) {
  small_rows_body<R, false>(tb, pcm, frame_begin, M, coef, row_flag, wave_fail, col0, EdgeRows{0u, M, 0u});
}

// The edge transform: columns [col0, 1024) of the launch's edge rows into their own buffer `coef` ([er.n][1024]), on
// the side stream: it reads the PCM and the tables and nothing a kernel of the launch writes.
template <int R>
__global__ __launch_bounds__(64) void k_mdct_edge_rows(DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M,
                                                        float *__restrict__ coef, unsigned col0, EdgeRows er) {
  small_rows_body<R, true, 8>(tb, pcm, frame_begin, M, coef, nullptr, nullptr, col0, er);
}

// ... and its capped form: the short table ring, and no more than kEdgeCapVgprs registers - what a SIMD has left beside
// two resident waves of k_quantize_screen<*, 1> (2 x 160 of 512), whose 512 workgroups are one round of the chip at two
// per CU; its 16 KiB of LDS fit beside their 2 x 68 KiB.  The cap that would fit beside a resident K1 workgroup (32
// registers) is out of reach of this chain: the table ring alone is 64.
constexpr int kEdgeCapVgprs = 192;
template <int R>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(kEdgeCapVgprs))) void k_mdct_edge_rows_capped(
    DeviceTables tb, PcmView pcm, long long frame_begin, unsigned M, float *__restrict__ coef, unsigned col0, EdgeRows er) {
  small_rows_body<R, true, 4>(tb, pcm, frame_begin, M, coef, nullptr, nullptr, col0, er);
}

// columns [col0, 1024) (col0 a multiple of 64) of the rows flagged in row_flag[M], found through wave_fail (the fail
// count of every quantiser wave of 4 rows, ceil(M / 16) * 4 words, 16-byte aligned): both as k_quantize_screen<*, 1>
// leaves them
template <int R>
inline hipError_t launch_small_rows(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                                    const unsigned *row_flag, const unsigned *wave_fail, uint32_t col0, hipStream_t s) {
  if (M == 0 || col0 >= static_cast<uint32_t>(kHopI)) return hipSuccess;
  if (col0 % 64u || !row_flag || !wave_fail) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_mdct_fwd_small_rows<R>), dim3(kRowsGrid), dim3(64), 0, s, t, pcm, static_cast<long long>(frame_begin), M,
                     coef, row_flag, wave_fail, col0);
  return hipGetLastError();
}

// columns [col0, 1024) of the edge rows `er` of a launch of M rows -> coef[er.n][1024]: one workgroup per item, nothing
// else in the grid
template <int R, bool CAPPED>
inline hipError_t launch_edge_rows(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                                   const EdgeRows &er, uint32_t col0, hipStream_t s) {
  if (M == 0 || er.n == 0 || col0 >= static_cast<uint32_t>(kHopI)) return hipSuccess;
  if (col0 % 64u || er.n_pre > er.suf0 || er.suf0 > M || er.n != er.n_pre + (M - er.suf0)) return hipErrorInvalidValue;
  const unsigned n_items = (er.n + R - 1) / R * ((static_cast<unsigned>(kHopI) - col0) / kRowsSlab);
  if (CAPPED)
    hipLaunchKernelGGL((k_mdct_edge_rows_capped<R>), dim3(n_items), dim3(64), 0, s, t, pcm, static_cast<long long>(frame_begin), M,
                       coef, col0, er);
  else
    hipLaunchKernelGGL((k_mdct_edge_rows<R>), dim3(n_items), dim3(64), 0, s, t, pcm, static_cast<long long>(frame_begin), M, coef,
                       col0, er);
  return hipGetLastError();
}

template <int BM, int BN, int BK, int TM, int TN, int UNROLL, int MINW>
inline hipError_t launch(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M,
                         float *coef, hipStream_t s) {
  using C = Cfg<BM, BN, BK, TM, TN, UNROLL, MINW>;
  if (M == 0) return hipSuccess;
  const unsigned m_tiles = (M + BM - 1) / BM;
  hipLaunchKernelGGL((k_mdct_fwd<BM, BN, BK, TM, TN, UNROLL, MINW>), dim3(m_tiles * C::kNTiles),
                     dim3(C::kThreads), 0, s, t, pcm, static_cast<long long>(frame_begin), M, coef);
  return hipGetLastError();
}

}  // namespace k1
}  // namespace glc
