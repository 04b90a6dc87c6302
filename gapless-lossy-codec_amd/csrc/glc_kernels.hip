// glc_kernels.hip — hand-written gfx950 (CDNA4) kernels of the codec hot path.
//
// Numerics contract: the reference transform is a dense 1024x2048 table
// contraction accumulated strictly in ascending index order with a separately rounded f32
// multiply and f32 add per term (rustc never fuses).  Every kernel below keeps that order and
// never lets the compiler contract a*b+c: the file is compiled with -ffp-contract=off and the
// accumulation is additionally written with __fmul_rn/__fadd_rn.  No v_fma/v_fmac/v_pk_fma may
// appear in the MDCT kernels (checked at build time by tools/check_isa.py) - with one exception that
// never produces a value of the stream: the bound waves of k_mdct_mix_st, and the bound column pairs of its hybrid
// waves, accumulate an UPPER BOUND of last-band magnitudes with v_pk_fma_f32 (the screen, above k_quantize; DESIGN
// section 2), and the matrix waves of k_mdct_mx_st the same bound with v_mfma_f32_32x32x16_bf16.
//
// Reference loops replaced (file:line into /root/reference):
//   K1 k_mdct_fwd      src/codec.rs:476-481 (window) + :359-374 (mdct_block)
//   K2 k_quantize      :488 (scale) + :188-240 (thresholds) + :270-311 (quantiser)
//   K3 k_decide_raw    :496-502 (raw plane) + :505-540 (size estimate, decision)
//   D1 k_imdct_rows    :626-644 (raw frames), :651-665 (dequant), :377-390 (imdct), :672-675
//   D2 k_overlap_add   :688-705 (overlap-add + interleave), :722-729 (tail)
#include <algorithm>
#include <type_traits>

#include "glc_common.h"
#include "glc_kernels.h"
#include "glc_mdct_fwd.hpp"

#pragma clang fp contract(off)

namespace glc {

namespace {

// What the K1 and D2 launchers share: the instantiation by channel count, f(CH) with CH = ch for 1 / 2 / 4 / 8 -
// the counts with a segment loader in K1 and a whole-chunk form in D2 - and CH = FALLBACK otherwise: 0, the form
// for any count, or 8 where the caller has already refused every other count.
template <int FALLBACK = 0, typename F>
auto by_channels(uint32_t ch, F &&f) {
  switch (ch) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, FALLBACK>{});
  }
}

constexpr int kHopI = 1024;
constexpr int kFrameI = 2048;

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }

// One zero-padded, de-interleaved PCM sample: padded[c][frame*1024 + i] of src/codec.rs:433-447.
__device__ __forceinline__ float pcm_at(const PcmView &v, int64_t frame, uint32_t c, int i) {
  const int64_t t = frame * kHopI + i - kHopI / 2;  // 512 leading zeros
  if (t < 0) return 0.0f;
  const uint64_t idx = static_cast<uint64_t>(t) * v.ch + c;
  if (idx >= v.n_samples) return 0.0f;  // trailing padding
  const uint64_t rel = static_cast<uint64_t>(t) - v.t0;
  if (static_cast<uint64_t>(t) < v.t0 || rel >= v.t_count) return 0.0f;  // outside the shard
  return v.p[rel * v.ch + c];
}

__device__ __forceinline__ short sat_i16(float x) {
  // f32::clamp(-32768, 32767) then `as i16`: truncation, NaN -> 0 (src/codec.rs:301,501)
  if (x != x) return 0;
  x = fminf(fmaxf(x, -32768.0f), 32767.0f);
  return static_cast<short>(static_cast<int>(x));
}

// K1 (forward MDCT) lives in glc_mdct_fwd.hpp.

// ------------------------------------------------------------------------------------------
// K2: scale, masking thresholds, quantiser (+ the raw-vs-compressed decision when a frame's
// channels all sit in one wave).  A wavefront owns 4 consecutive frame-channel rows.
//   phase 1  16 coefficients per lane and row: max|c| by shuffle (order-free), squares to LDS
//   phase 2  band sums in the reference's ascending order (src/codec.rs:212-214): lane l sums
//            bands (l & 15), +16, +32, +48 of row l >> 4, so the long last band (683 bins at
//            48 kHz) of the 4 rows runs in 4 lanes side by side instead of one lane per wave
//   phase 3  thresholds, noise floor, quantiser; {scale, nnz} into the record header
//   phase 4  FUSED (1 / 2 / 4 channels: a frame's rows are 1 / 2 / 4 consecutive rows of this
//            wave): size estimate and decision of src/codec.rs:505-521; a compressed frame gets
//            its dense i16 rows, a raw frame the channel-planar windowed i16 plane (:496-502, Q1)
//            - K3 is not launched at all.  Other channel counts: dense rows here, decision in K3.
// ------------------------------------------------------------------------------------------
constexpr int kQRows = 4;  // rows per wave

// The screen.  With L = edges[n_bands - 1] the start of the last band and C0 = L rounded up to
// 64, the mixed-role K1 leaves exact coefficients only below C0; of a column k >= C0 it leaves e_k, the same sum
// with fused multiply-adds, as max |e| per PLANE - the bound columns of one wave of the transform: 8 of them, or
// the 2 / 4 / 6 of a hybrid wave, or the 160 of a workgroup of the matrix form (k_mdct_mx_st, whose e_k is a sum of
// bf16 piece products within the same gamma_2048 sum |xw| of the real sum: glc_kernels.h MatrixBound); the screen only
// ever takes the maximum over all planes, so which columns a plane
// holds is the transform's business - and A = sum_i |fl(x_i w_i)|, the ascending f32 sum.  The stream's value is
// c_k = fl(s_k norm) with s_k the ascending f32 sum of the rounded products.  Both s_k and e_k differ from the
// real sum of xw_i T_ki by at most gamma_2048 sum_i |xw_i| |T_ki| (2048 roundings each at most: product and add
// per term there, one fused rounding per term here; gamma_n = n u / (1 - n u), u = 2^-24), and |T| <= 1, so
//     |c_k| <= (max_planes |e| + 2 gamma_2048 A) norm (1 + u),          2 gamma_2048 = 2.4417e-4 < kScreenCErr.
// kScreenSlack covers that (1 + u), the roundings of the bound's own five operations and those of the 2048 adds
// behind A (relative gamma_2048 = 1.3e-4, on a term that only adds); kScreenTiny the products that underflow
// (4096 operations, each off by less than 2^-126 even where subnormals are flushed: < 5e-35).
// A row PASSES iff (a) no exact bin in [L, C0) exceeds nfl = noise_floor * scale and (b) B <= nfl, B finite, with
// scale taken over [0, C0) alone.  Then every |c_k|, k >= L, is <= nfl < scale: the scale IS the row's (or both are
// the 1e-10 floor), every bin of the last band quantises to 0 whatever its threshold, and the band's ordered
// energy sum is never needed.  A NaN or an infinity anywhere in the row's samples makes A, hence B, non-finite:
// the row fails.  A row that fails is left to the repair (exact columns C0.., then this kernel's MODE 2).
constexpr float kScreenCErr = 2.45e-4f, kScreenSlack = 1.001f, kScreenTiny = 1e-33f;

struct ScreenArgs {
  const float *hf;        // [n_planes + 1][stride]: per bound-carrying wave of the transform max |e| of its columns >= C0, then A
  unsigned *row_flag;     // [M] 1 = the row's frame failed the screen and is the serial repair's, 2 = it failed and is an
                          // edge row (the side stream's), 0 = it passed (MODE 1 writes every entry, MODE 2 reads)
  unsigned *wave_fail;    // [waves of the MODE 1 launch] rows flagged 1 of each wave (every entry written)
  unsigned *host_stat;    // host-mapped {failed rows, rows, seq, -, u64 failed rows so far}: MODE 2 leaves the counts;
                          // the edge rows that failed are in none of them
  unsigned long long stride;
  unsigned c0, l0, n_planes, seq;
  unsigned long long edge_a, edge_b;  // frame f is an edge frame iff f < edge_a || f >= edge_b (glc_kernels.h edge_frames;
                                      // 0 and kNoEdge: none is)
  unsigned long long *edge_total;     // device: failed edge rows so far (read and written only by a launch that has edge rows)
};

// MODE 0: every row of the launch from exact coefficients.  1: the screened form - rows that pass, from the
// columns below C0; rows that fail are flagged and left alone, and so are the edge rows, whose screen is evaluated
// for the statistics only.  2: the repair - MODE 0 on the rows flagged 1 only.  3: MODE 0 on the edge rows only, one
// workgroup per group of 16 rows that holds one; `coef` is then the edge rows' own buffer, row j of it the j-th edge
// row (beside K1 and K2 on another stream: it reads nothing they write, and writes records they leave alone).
template <bool FUSED, int MODE>
__device__ __forceinline__ void quantize_body(const DeviceTables &tb, const float *__restrict__ coef, unsigned M,
                                              unsigned ch, unsigned long long rec_bytes, unsigned long long hdr_bytes,
                                              const PcmView &pcm, long long frame_begin,
                                              unsigned char *__restrict__ records, const ScreenArgs &sa) {
  __shared__ __attribute__((aligned(16))) float ssq[4][kQRows][kHopI];  // 64 KiB
  __shared__ float sbase[4][kQRows][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned blk = blockIdx.x;  // the group of 16 rows this workgroup quantises
  EdgeRows er{0u, M, 0u};     // the launch's edge rows: [0, n_pre) and [suf0, M)
  if constexpr (MODE != 0) er = edge_rows(sa.edge_a, sa.edge_b, static_cast<unsigned long long>(frame_begin), M, ch);
  if constexpr (MODE == 3) {
    const unsigned g_pre = (er.n_pre + 15u) / 16u, g_suf = er.suf0 / 16u > g_pre ? er.suf0 / 16u : g_pre;
    if (blk >= g_pre) blk = g_suf + (blk - g_pre);
  }
  const unsigned m0 = (blk * 4 + w) * kQRows;
  unsigned on = 0;  // MODE 1 / 2 / 3: bit r = row m0 + r is this launch's to write
  auto edge_row = [&](unsigned m) -> bool { return m < er.n_pre || m >= er.suf0; };
  if constexpr (MODE == 3) {
#pragma unroll
    for (int r = 0; r < kQRows; ++r)
      if (m0 + r < M && edge_row(m0 + r)) on |= 1u << r;
  }
  if constexpr (MODE == 2) {
    if (blk == 0 && w == 0) {  // the counts of the screened launch, for the host's guard and statistics
      const unsigned n_w = (M + 15) / 16 * 4;
      unsigned cnt = 0, ecnt = 0;
      // the edge rows that failed: not the serial repair's, so not in wave_fail; they count in the statistics alone,
      // in device memory (a launch without edge rows touches none of this)
      unsigned long long etot = 0;
      if (er.n) etot = *sa.edge_total;
      for (unsigned i = lane; i < n_w; i += 64) cnt += sa.wave_fail[i];
      for (unsigned i = lane; i < er.n; i += 64) ecnt += sa.row_flag[i < er.n_pre ? i : er.suf0 + (i - er.n_pre)] == 2u;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off), ecnt += __shfl_xor(ecnt, off);
      if (lane == 0) {
        // plain stores, in no order the host can rely on: it reads them unsynchronised, for a heuristic (the guard,
        // glc_api.hip screen_takes); the statistics call reads them after the stream has been waited for
        volatile unsigned *hs = sa.host_stat;
        volatile unsigned long long *tot = reinterpret_cast<volatile unsigned long long *>(sa.host_stat + 4);
        *tot = *tot + cnt;
        if (er.n) *sa.edge_total = etot + ecnt;
        hs[0] = cnt;
        hs[1] = M;
        hs[2] = sa.seq;
      }
    }
    // every wave reads the 16 flags of the workgroup's rows: the whole workgroup leaves, or none of it
    const unsigned fr = blk * 16 + lane;
    const bool flagged = lane < 16 && fr < M && sa.row_flag[fr] == 1u;
    const unsigned blk_on = static_cast<unsigned>(__ballot(flagged));
    if (blk_on == 0u) return;
    on = (blk_on >> (4 * w)) & 0xFu;
  }
  auto row_on = [&](int r) -> bool {
    if constexpr (MODE == 0) return m0 + r < M;
    else return (on >> r) & 1u;
  };

  // per-lane constants of the 16 bins this lane owns (the same bins in every row)
  float4 indiv4[4];
  unsigned short bo[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k0 = (lane + 64 * j) * 4;
    indiv4[j] = *reinterpret_cast<const float4 *>(tb.indiv + k0);
    const ushort4 b4 = *reinterpret_cast<const ushort4 *>(tb.band_of + k0);
    bo[j][0] = b4.x; bo[j][1] = b4.y; bo[j][2] = b4.z; bo[j][3] = b4.w;
  }

  float4 c4[kQRows][4];
  float scale[kQRows];
#pragma unroll
  for (int r = 0; r < kQRows; ++r) {
    const unsigned m = m0 + r;
    float amax = 0.0f;
    if (MODE == 1 ? m < M : row_on(r)) {
      const unsigned src_row = MODE == 3 ? (m < er.n_pre ? m : er.n_pre + (m - er.suf0)) : m;
      const float4 *src = reinterpret_cast<const float4 *>(coef + static_cast<size_t>(src_row) * kHopI);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (MODE == 1) {  // columns >= C0 (a multiple of 64) were not computed: they count as 0
          if ((lane + 64 * j) * 4 >= static_cast<int>(sa.c0)) {
            c4[r][j] = float4{0.f, 0.f, 0.f, 0.f};
            continue;
          }
        }
        const float4 v = src[lane + 64 * j];
        c4[r][j] = v;
        amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        float4 sq;  // each square is one rounding, order-free; only the SUM is ordered
        sq.x = mul_rn(v.x, v.x); sq.y = mul_rn(v.y, v.y); sq.z = mul_rn(v.z, v.z); sq.w = mul_rn(v.w, v.w);
        *reinterpret_cast<float4 *>(&ssq[w][r][(lane + 64 * j) * 4]) = sq;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) c4[r][j] = float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    scale[r] = fmaxf(amax, 1e-10f);  // :488 (and global_max at :198, :278)
  }
  if constexpr (MODE == 1) {
    // the screen: rows m0 .. m0 + 3 are one float4 of every hf plane
    float hfm[4] = {0.f, 0.f, 0.f, 0.f};
    for (unsigned o = lane; o < sa.n_planes; o += 64) {
      const float4 h = *reinterpret_cast<const float4 *>(sa.hf + o * sa.stride + m0);
      hfm[0] = fmaxf(hfm[0], h.x); hfm[1] = fmaxf(hfm[1], h.y); hfm[2] = fmaxf(hfm[2], h.z); hfm[3] = fmaxf(hfm[3], h.w);
    }
    const float4 a4 = *reinterpret_cast<const float4 *>(sa.hf + sa.n_planes * sa.stride + m0);
    const float asum[4] = {a4.x, a4.y, a4.z, a4.w};
    unsigned fail = 0;
#pragma unroll
    for (int r = 0; r < kQRows; ++r) {
      float h = hfm[r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) h = fmaxf(h, __shfl_xor(h, off));
      const float nfl = mul_rn(tb.noise_floor, scale[r]);
      bool hit = false;  // (a) an exact bin of the last band above the floor
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float cv[4] = {c4[r][j].x, c4[r][j].y, c4[r][j].z, c4[r][j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned k = (lane + 64 * j) * 4 + e;
          hit = hit || (k >= sa.l0 && k < sa.c0 && fabsf(cv[e]) > nfl);
        }
      }
      const float bound = add_rn(mul_rn(mul_rn(add_rn(h, mul_rn(kScreenCErr, asum[r])), tb.norm), kScreenSlack), kScreenTiny);
      const bool pass = __ballot(hit) == 0ull && bound <= nfl && bound < __builtin_inff();  // a NaN bound fails
      if (!pass) fail |= 1u << r;
    }
    unsigned valid = 0;
#pragma unroll
    for (int r = 0; r < kQRows; ++r)
      if (m0 + r < M) valid |= 1u << r;
    fail &= valid;
    if (FUSED) {  // a frame's rows are consecutive rows of this wave: one failing row fails its frame
      unsigned ff = 0;
#pragma unroll
      for (int r = 0; r < kQRows; ++r)
#pragma unroll
        for (int q = 0; q < kQRows; ++q)
          if (static_cast<unsigned>(q) / ch == static_cast<unsigned>(r) / ch && ((fail >> q) & 1u)) ff |= 1u << r;
      fail = ff & valid;
    }
    unsigned edge = 0;  // (FUSED: a frame's rows are all edge rows or none is)
#pragma unroll
    for (int r = 0; r < kQRows; ++r)
      if (((valid >> r) & 1u) && edge_row(m0 + r)) edge |= 1u << r;
    on = valid & ~fail & ~edge;
    if (lane < kQRows && m0 + lane < M) sa.row_flag[m0 + lane] = ((fail >> lane) & 1u) << ((edge >> lane) & 1u);
    if (lane == 0) sa.wave_fail[blk * 4 + w] = __builtin_popcount(fail & ~edge);
  }
  __syncthreads();

  {
    const int r = lane >> 4;
    if (row_on(r)) {
      const float *sq = ssq[w][r];
      for (unsigned b = lane & 15; b < tb.n_bands; b += 16) {
        if constexpr (MODE == 1) {
          if (b == tb.n_bands - 1) {  // every bin of the last band is known to quantise to 0
            sbase[w][r][b] = 0.0f;
            continue;
          }
        }
        const unsigned lo = tb.edges[b], hi = tb.edges[b + 1];
        float ss = 0.0f;
        unsigned i = lo;
        // head: up to 3 bins until the index is 16-byte aligned
        for (; i < hi && (i & 3u); ++i) ss = add_rn(ss, sq[i]);
        // body: 16 bins per step as four ds_read_b128, the next step's reads in flight while the
        // current 16 adds (a dependent chain, the reference's order) execute; ping-pong registers
#define GLC_ADD4(V) ss = add_rn(ss, V.x); ss = add_rn(ss, V.y); ss = add_rn(ss, V.z); ss = add_rn(ss, V.w)
        if (i + 16 <= hi) {
          const float4 *q4 = reinterpret_cast<const float4 *>(sq);
          float4 a0 = q4[i >> 2], a1 = q4[(i >> 2) + 1], a2 = q4[(i >> 2) + 2], a3 = q4[(i >> 2) + 3];
          while (i + 32 <= hi) {
            const float4 b0 = q4[(i >> 2) + 4], b1 = q4[(i >> 2) + 5], b2 = q4[(i >> 2) + 6], b3 = q4[(i >> 2) + 7];
            GLC_ADD4(a0); GLC_ADD4(a1); GLC_ADD4(a2); GLC_ADD4(a3);
            i += 16;
            if (i + 32 <= hi) {
              a0 = q4[(i >> 2) + 4]; a1 = q4[(i >> 2) + 5]; a2 = q4[(i >> 2) + 6]; a3 = q4[(i >> 2) + 7];
              GLC_ADD4(b0); GLC_ADD4(b1); GLC_ADD4(b2); GLC_ADD4(b3);
              i += 16;
            } else {
              a0 = b0; a1 = b1; a2 = b2; a3 = b3;
            }
          }
          GLC_ADD4(a0); GLC_ADD4(a1); GLC_ADD4(a2); GLC_ADD4(a3);
          i += 16;
        }
#undef GLC_ADD4
        for (; i < hi; ++i) ss = add_rn(ss, sq[i]);  // tail: fewer than 16 bins
        const float energy = sqrtf(ss / tb.band_len[b]);                                  // :214-215
        sbase[w][r][b] = mul_rn(mul_rn(mul_rn(energy, 0.01f), tb.cf), tb.band_pf[b]);      // :223
      }
    }
  }
  __syncthreads();

  short4 pk[kQRows][4];
  unsigned nnz[kQRows];
#pragma unroll
  for (int r = 0; r < kQRows; ++r) {
    const unsigned m = m0 + r;
    nnz[r] = 0;
    if (!row_on(r)) {
      if constexpr (MODE == 0) break;
      else continue;
    }
    const float sc = scale[r];
    const float nfl = mul_rn(tb.noise_floor, sc);  // :277
    const float peak_gate = mul_rn(sc, 0.3f);      // global_max * 0.3, :232
    const float peak_cap = mul_rn(sc, 0.05f);      // global_max * 0.05, :234
    unsigned cnt = 0;
    // the 16 band bases of this lane's bins, fetched together: left to the compiler, each of the 16 LDS reads
    // sits directly in front of its use and is waited for there (64 exposed LDS round trips per wave)
    float sb[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) sb[j][e] = sbase[w][r][bo[j][e]];
    asm volatile("" : "+v"(sb[0][0]), "+v"(sb[0][1]), "+v"(sb[0][2]), "+v"(sb[0][3]), "+v"(sb[1][0]), "+v"(sb[1][1]),
                      "+v"(sb[1][2]), "+v"(sb[1][3]), "+v"(sb[2][0]), "+v"(sb[2][1]), "+v"(sb[2][2]), "+v"(sb[2][3]),
                      "+v"(sb[3][0]), "+v"(sb[3][1]), "+v"(sb[3][2]), "+v"(sb[3][3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float cv[4] = {c4[r][j].x, c4[r][j].y, c4[r][j].z, c4[r][j].w};
      const float iv[4] = {indiv4[j].x, indiv4[j].y, indiv4[j].z, indiv4[j].w};
      short qv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = fabsf(cv[e]);
        float t = mul_rn(sb[j][e], iv[e]);                           // :228-229
        if (a > peak_gate) t = fminf(t, peak_cap);                  // :232-235
        const float thr = mul_rn(t, sc);                            // :288
        short q = 0;
        if (a > nfl && a > thr) {                                   // :291
          const float normalized = cv[e] / sc;                      // :299 (IEEE divide)
          q = sat_i16(roundf(mul_rn(normalized, 32768.0f)));        // :300-301
        }
        qv[e] = q;
        cnt += (q != 0);
      }
      pk[r][j].x = qv[0]; pk[r][j].y = qv[1]; pk[r][j].z = qv[2]; pk[r][j].w = qv[3];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    nnz[r] = cnt;
    if (lane == 0) {
      const unsigned frame = m / ch, c = m % ch;
      unsigned char *rec = records + static_cast<size_t>(frame) * rec_bytes;
      record_scale(rec, c) = sc;
      record_nnz(rec, c) = cnt;
    }
  }

  // phase 4: payload.  FUSED: the frame of row r spans rows r - r % ch .. + ch - 1 of this wave.
#pragma unroll
  for (int r = 0; r < kQRows; ++r) {
    const unsigned m = m0 + r;
    if (!row_on(r)) {
      if constexpr (MODE == 0) break;
      else continue;
    }
    const unsigned frame = m / ch, c = m % ch;
    unsigned char *rec = records + static_cast<size_t>(frame) * rec_bytes;
    bool use_raw = false;
    if (FUSED) {
      unsigned long long compressed = 8ull + 4ull * ch + 64ull;   // :513, :515
#pragma unroll
      for (int q = 0; q < kQRows; ++q)
        if (static_cast<unsigned>(q) / ch == static_cast<unsigned>(r) / ch) compressed += 8ull + 4ull * nnz[q];  // :507-511
      const unsigned long long raw_size = 2ull * kFrameI * ch;    // :518
      use_raw = static_cast<float>(compressed) >= mul_rn(static_cast<float>(raw_size), 0.85f);  // :521
      if (c == 0 && lane == 0) {
        record_raw(rec) = use_raw ? 1u : 0u;
        *reinterpret_cast<unsigned *>(rec + 4) = 0u;
      }
    }
    short *qrow = reinterpret_cast<short *>(rec + hdr_bytes) + static_cast<size_t>(c) * kFrameI;
    if (!use_raw) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<short4 *>(qrow + (lane + 64 * j) * 4) = pk[r][j];
    } else {
      // raw fallback plane of this row's channel, windowed once (:498-502)
      const long long fabs_ = frame_begin + frame;
      for (int i = lane; i < kFrameI; i += 64) {
        const float sw = mul_rn(pcm_at(pcm, fabs_, c, i), tb.window[i]);  // :500
        qrow[i] = sat_i16(mul_rn(sw, 32767.0f));                          // :501
      }
    }
  }
}

template <bool FUSED>
__global__ __launch_bounds__(256) void k_quantize(DeviceTables tb, const float *__restrict__ coef,
                                                   unsigned M, unsigned ch, unsigned long long rec_bytes,
                                                   unsigned long long hdr_bytes, PcmView pcm, long long frame_begin,
                                                   unsigned char *__restrict__ records) {
  quantize_body<FUSED, 0>(tb, coef, M, ch, rec_bytes, hdr_bytes, pcm, frame_begin, records, ScreenArgs{});
}

template <bool FUSED, int MODE>
__global__ __launch_bounds__(256) void k_quantize_screen(DeviceTables tb, const float *__restrict__ coef,
                                                          unsigned M, unsigned ch, unsigned long long rec_bytes,
                                                          unsigned long long hdr_bytes, PcmView pcm, long long frame_begin,
                                                          unsigned char *__restrict__ records, ScreenArgs sa) {
  quantize_body<FUSED, MODE>(tb, coef, M, ch, rec_bytes, hdr_bytes, pcm, frame_begin, records, sa);
}

// ------------------------------------------------------------------------------------------
// K3: one workgroup per frame: size estimate and raw-vs-compressed decision; raw frames get
// the channel-planar windowed i16 plane (quirk Q1) written over their payload.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_decide_raw(DeviceTables tb, PcmView pcm, long long frame_begin,
                                                     unsigned n_frames, unsigned long long rec_bytes,
                                                     unsigned long long hdr_bytes,
                                                     unsigned char *__restrict__ records) {
  const unsigned fr = blockIdx.x;
  if (fr >= n_frames) return;
  unsigned char *rec = records + static_cast<size_t>(fr) * rec_bytes;
  const unsigned ch = pcm.ch;
  unsigned long long compressed = 0;
  for (unsigned c = 0; c < ch; ++c)
    compressed += 8ull + 4ull * record_nnz(rec, c);  // :507-511
  compressed += 8ull + 4ull * ch;  // :513
  compressed += 64ull;             // :515
  const unsigned long long raw_size = 2ull * kFrameI * ch;  // :518
  const bool use_raw =
      static_cast<float>(compressed) >= mul_rn(static_cast<float>(raw_size), 0.85f);  // :521
  if (threadIdx.x == 0) {
    record_raw(rec) = use_raw ? 1u : 0u;
    *reinterpret_cast<unsigned *>(rec + 4) = 0u;
  }
  if (!use_raw) return;
  short *plane = reinterpret_cast<short *>(rec + hdr_bytes);
  const long long frame = frame_begin + fr;
  for (unsigned idx = threadIdx.x; idx < ch * kFrameI; idx += 256) {
    const unsigned c = idx / kFrameI, i = idx % kFrameI;
    const float s = mul_rn(pcm_at(pcm, frame, c, static_cast<int>(i)), tb.window[i]);  // :500
    plane[idx] = sat_i16(mul_rn(s, 32767.0f));                                         // :501
  }
}

// ------------------------------------------------------------------------------------------
// D1: one workgroup per frame-channel row, 8 outputs per lane.  out[i] = sum over k ascending
// of c[k]*T[k][i]; adding the +0.0 products of zero coefficients is the identity on the running
// sum (which is never -0.0), so iterating only the stored non-zeros in ascending k is
// bit-identical to the reference's dense loop and does nnz/1024 of the work.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_imdct_rows(DeviceTables tb, DecodeRows rows, unsigned row_begin,
                                                     unsigned M, unsigned ch, float *__restrict__ blocks) {
  __shared__ float s_val[kHopI];
  __shared__ unsigned short s_idx[kHopI];
  const unsigned r = blockIdx.x;
  if (r >= M) return;
  const unsigned m = row_begin + r;
  float *out = blocks + static_cast<size_t>(r) * kFrameI;
  const int tid = threadIdx.x;

  const long long raw_off = rows.row_raw[m];
  if (raw_off >= 0) {
    // raw frame: read as if interleaved (Q1), /32767, no window (Q2) — src/codec.rs:629-640
    const unsigned c = m % ch;
    const unsigned long long raw_len = rows.row_raw_len[m];
    const short *raw = rows.raw_pool + raw_off;
    for (int i = tid; i < kFrameI; i += 256) {
      const unsigned long long si = static_cast<unsigned long long>(i) * ch + c;
      float v = 0.0f;
      if (si < raw_len) v = static_cast<float>(raw[si]) / 32767.0f;
      out[i] = v;
    }
    return;
  }

  const unsigned long long p0 = rows.row_begin[m];
  const unsigned n = min(rows.row_cnt[m], static_cast<unsigned>(kHopI));  // canonical lists hold <= 1024
  const float scale = fmaxf(rows.row_scale[m], 1e-12f);  // :653
  for (unsigned j = tid; j < n; j += 256) {
    const unsigned pr = rows.pairs[p0 + j];
    const short q = static_cast<short>(pr >> 16);
    s_idx[j] = static_cast<unsigned short>(pr & 0xFFFFu);
    s_val[j] = mul_rn(static_cast<float>(q) / 32768.0f, scale);  // :663
  }
  __syncthreads();

  float4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  const float *T = tb.cos + tid * 4;
  for (unsigned j = 0; j < n; ++j) {
    const float cv = s_val[j];
    const float *trow = T + static_cast<size_t>(s_idx[j]) * kFrameI;
    const float4 t0 = *reinterpret_cast<const float4 *>(trow);
    const float4 t1 = *reinterpret_cast<const float4 *>(trow + 1024);
    a0.x = add_rn(a0.x, mul_rn(cv, t0.x)); a0.y = add_rn(a0.y, mul_rn(cv, t0.y));
    a0.z = add_rn(a0.z, mul_rn(cv, t0.z)); a0.w = add_rn(a0.w, mul_rn(cv, t0.w));
    a1.x = add_rn(a1.x, mul_rn(cv, t1.x)); a1.y = add_rn(a1.y, mul_rn(cv, t1.y));
    a1.z = add_rn(a1.z, mul_rn(cv, t1.z)); a1.w = add_rn(a1.w, mul_rn(cv, t1.w));
  }
  const float4 w0 = *reinterpret_cast<const float4 *>(tb.window + tid * 4);
  const float4 w1 = *reinterpret_cast<const float4 *>(tb.window + 1024 + tid * 4);
  float4 o0, o1;  // out[i] = s*norm (:388) then *= window[i] (:674)
  o0.x = mul_rn(mul_rn(a0.x, tb.norm), w0.x); o0.y = mul_rn(mul_rn(a0.y, tb.norm), w0.y);
  o0.z = mul_rn(mul_rn(a0.z, tb.norm), w0.z); o0.w = mul_rn(mul_rn(a0.w, tb.norm), w0.w);
  o1.x = mul_rn(mul_rn(a1.x, tb.norm), w1.x); o1.y = mul_rn(mul_rn(a1.y, tb.norm), w1.y);
  o1.z = mul_rn(mul_rn(a1.z, tb.norm), w1.z); o1.w = mul_rn(mul_rn(a1.w, tb.norm), w1.w);
  *reinterpret_cast<float4 *>(out + tid * 4) = o0;
  *reinterpret_cast<float4 *>(out + 1024 + tid * 4) = o1;
}

// ------------------------------------------------------------------------------------------
// D1, SHIPPED: plan + apply.  A unit of work is 8 consecutive frames of ONE channel (rows f*ch + c,
// f = f0 .. f0+7) decoded over the UNION of their coefficient indices, so that a table row is read
// from L2 once for the group.  Consecutive frames of one channel are the rows that share indices:
// tonal material keeps its partials from frame to frame, while two channels may carry different
// instruments.  Per row the arithmetic is the reference's: its stored non-zeros applied in ascending
// k; a row that lacks an index of the union multiplies the table row by its +0.0 and adds the signed
// zero, which is the identity on a running sum that is never -0.0 (the same identity the sparse skip
// of the one-row kernel rests on).
//   k_imdct_plan   one workgroup per (group, channel): the rows are dequantised into LDS, the ascending
//                  union of their indices is built and written to global memory as 64-byte records
//                  {8 coefficients (+0.0 = absent), byte offset of the table row of entry j+2}, with a
//                  header {n_u, live rows, offsets of entries 0 and 1, dense flag, rows of raw frames}
//                  and the unit's work for k_imdct_order.  Nothing here depends on where the blocks
//                  go: the records of a launch stay valid for as long as the context holds the
//                  stream's rows, and a repeated decode skips this kernel (glc_api.hip launch_d1).
//   k_imdct_order  ranks the units of a launch by work and deals them over the CUs (speed only).
//   k_imdct_apply  no LDS, no barrier: each wave owns 8 rows x 512 outputs.  The record of the next
//                  entry arrives by scalar loads (s_load_dwordx8 + s_load_dword) a whole entry ahead;
//                  the coefficient pairs feed v_pk_mul_f32 straight from SGPRs (lane-broadcast by
//                  op_sel); the table row of the entry after next is in flight by
//                  global_load_dwordx4 from an SGPR base.  The vector ALU executes the 64 packed
//                  multiplies / adds of an entry and nothing else; a row pair whose two coefficients
//                  are both absent is skipped by a scalar branch (SKIP), so groups that share few
//                  indices degrade gracefully instead of needing a second code path.
// ------------------------------------------------------------------------------------------
typedef float d1x2 __attribute__((ext_vector_type(2)));
typedef float d1x4 __attribute__((ext_vector_type(4)));
typedef unsigned d1u8 __attribute__((ext_vector_type(8)));
typedef unsigned d1u2 __attribute__((ext_vector_type(2)));
constexpr unsigned kPlanRecDwords = 16;       // 64-byte records
constexpr unsigned kPlanHdrDwords = 8;        // {n_u, live rows, table offsets of the first <= 4 entries, dense flag, pad}
constexpr unsigned kPlanRecCap = kHopI + 8;   // per group: the union holds <= 1024 entries; the apply loop reads a few past

__global__ __launch_bounds__(256) void k_imdct_plan(DecodeRows rows, unsigned row_begin, unsigned n_frames, unsigned ch,
                                                     unsigned group_begin, unsigned ahead, unsigned *__restrict__ plan_hdr,
                                                     unsigned *__restrict__ plan_rec, unsigned *__restrict__ plan_work) {
  constexpr int G = 8;
  __shared__ __attribute__((aligned(16))) float s_c[kHopI * G];
  __shared__ unsigned s_mask[kHopI / 32];
  __shared__ unsigned short s_u[kHopI + 8];
  __shared__ unsigned s_wsum[4];
  const int tid = threadIdx.x;
  // blockIdx = (frame group - fg_begin) * ch + channel: the batch covers whole frame groups
  const unsigned c = blockIdx.x % ch;
  const unsigned fr0 = (group_begin + blockIdx.x / ch) * G;
  const int lane = tid & 63, w = tid >> 6;
  // The kernel is a chain of latencies, so everything independent is issued together: the metadata
  // of the 8 rows by 8 lanes at once (broadcast by shuffles afterwards) while the LDS is zeroed, then
  // the first 256 pairs of ALL rows before any of them is scattered.
  long long raw_l = -1;
  unsigned long long p0_l = 0;
  unsigned n_l = 0, valid_l = 0;
  float scale_l = 0.0f;
  if (lane < G && fr0 + lane < n_frames) {
    const unsigned m = row_begin + (fr0 + lane) * ch + c;
    raw_l = rows.row_raw[m];
    p0_l = rows.row_begin[m];
    n_l = min(rows.row_cnt[m], static_cast<unsigned>(kHopI));  // canonical lists hold <= 1024
    scale_l = fmaxf(rows.row_scale[m], 1e-12f);                  // :653
    valid_l = 1;
  }
  {
    d1x4 *z = reinterpret_cast<d1x4 *>(s_c);
    for (int i = tid; i < kHopI * G / 4; i += 256) z[i] = d1x4{0.f, 0.f, 0.f, 0.f};
  }
  if (tid < kHopI / 32) s_mask[tid] = 0u;
  unsigned live = 0, rawm = 0;
  unsigned long long p0[G];
  unsigned n[G];
  float scale[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const unsigned valid = __shfl(valid_l, g);
    const long long raw_off = __shfl(raw_l, g);
    p0[g] = __shfl(p0_l, g);
    n[g] = __shfl(n_l, g);
    scale[g] = __shfl(scale_l, g);
    if (valid && raw_off >= 0) rawm |= 1u << g;
    else if (valid) live |= 1u << g;
    if (!(live & (1u << g))) n[g] = 0;
  }
  unsigned pr[G];
#pragma unroll
  for (int g = 0; g < G; ++g) pr[g] = static_cast<unsigned>(tid) < n[g] ? rows.pairs[p0[g] + tid] : 0xFFFFu;
  __syncthreads();  // LDS zeroed
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const unsigned idx = pr[g] & 0xFFFFu;
    if (idx < static_cast<unsigned>(kHopI)) {  // 0xFFFF = no pair for this thread (also what a reader must ignore, :660)
      const short q = static_cast<short>(pr[g] >> 16);
      s_c[idx * G + g] = mul_rn(static_cast<float>(q) / 32768.0f, scale[g]);  // :663
      atomicOr(&s_mask[idx >> 5], 1u << (idx & 31));
    }
    for (unsigned j = tid + 256; j < n[g]; j += 256) {  // lists longer than 256 entries
      const unsigned p = rows.pairs[p0[g] + j];
      const unsigned k = p & 0xFFFFu;
      if (k < static_cast<unsigned>(kHopI)) {
        s_c[k * G + g] = mul_rn(static_cast<float>(static_cast<short>(p >> 16)) / 32768.0f, scale[g]);
        atomicOr(&s_mask[k >> 5], 1u << (k & 31));
      }
    }
  }
  __syncthreads();
  // ascending union list: thread t owns bins 4t..4t+3; exclusive scan of the per-thread counts
  const unsigned nib = (s_mask[tid >> 3] >> ((tid & 7) * 4)) & 0xFu;
  const unsigned cnt = __popc(nib);
  unsigned incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) s_wsum[w] = incl;
  __syncthreads();
  unsigned base = 0, n_u = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned v = s_wsum[i];
    if (i < w) base += v;
    n_u += v;
  }
  {
    unsigned pos = base + incl - cnt;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (nib & (1u << b)) s_u[pos++] = static_cast<unsigned short>(tid * 4 + b);
  }
  __syncthreads();
  if (tid < 8) s_u[n_u + tid] = n_u ? s_u[n_u - 1] : static_cast<unsigned short>(0);  // run-ahead reads stay valid
  __syncthreads();
  unsigned *rec = plan_rec + static_cast<size_t>(blockIdx.x) * kPlanRecCap * kPlanRecDwords;
  for (unsigned j = tid; j < n_u; j += 256) {
    const unsigned k = s_u[j];
    d1x4 *dst = reinterpret_cast<d1x4 *>(rec + static_cast<size_t>(j) * kPlanRecDwords);
    dst[0] = *reinterpret_cast<const d1x4 *>(&s_c[k * G]);
    dst[1] = *reinterpret_cast<const d1x4 *>(&s_c[k * G + 4]);
    rec[static_cast<size_t>(j) * kPlanRecDwords + 8] = static_cast<unsigned>(s_u[j + ahead]) << 13;  // table row bytes = 8192
  }
  if (tid < 8) {
    unsigned *h = plan_hdr + static_cast<size_t>(blockIdx.x) * kPlanHdrDwords;
    // h[6]: 1 when the rows share most of their indices (union <= 2x the mean list), see k_imdct_apply
    unsigned total = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) total += n[g];
    const unsigned dense = n_u * G <= 2u * total ? 1u : 0u;
    // h[7]: rows of raw frames (written by k_imdct_raw_rows on every launch: the plan may outlive one, the blocks do not)
    h[tid] = tid == 0 ? n_u : tid == 1 ? live : tid < 2 + ahead ? static_cast<unsigned>(s_u[tid - 2]) << 13 : tid == 6 ? dense : tid == 7 ? rawm : 0u;
    // work of the unit for the placement below: packed operations it issues (stored non-zeros) plus
    // the per-entry overhead of walking its union (record fetch, table row)
    if (tid == 0) plan_work[blockIdx.x] = total + n_u + (rawm ? 64u : 0u);
  }
}

// Rows of raw frames of a launch (streams that have any): read as if interleaved (Q1), /32767, no window
// (Q2) - src/codec.rs:629-640.  One workgroup per row; rows of compressed frames return at once.  Its
// own kernel so that the apply kernel stays free of the division's fused expansion (tools/check_isa.py)
// and a kept plan (launch_d1) never leaves these blocks unwritten.
__global__ __launch_bounds__(256) void k_imdct_raw_rows(DecodeRows rows, unsigned row_begin, unsigned M, unsigned ch,
                                                         float *__restrict__ blocks) {
  const unsigned r = blockIdx.x;
  if (r >= M) return;
  const unsigned m = row_begin + r;
  const long long raw_off = rows.row_raw[m];
  if (raw_off < 0) return;
  const unsigned c = m % ch;
  const unsigned long long raw_len = rows.row_raw_len[m];
  const short *raw = rows.raw_pool + raw_off;
  float *out = blocks + static_cast<size_t>(r) * kFrameI;
  for (int i = threadIdx.x; i < kFrameI; i += 256) {
    const unsigned long long si = static_cast<unsigned long long>(i) * ch + c;
    float v = 0.0f;
    if (si < raw_len) v = static_cast<float>(raw[si]) / 32767.0f;
    out[i] = v;
  }
}

// Placement of the units of one launch (speed only).  All units of a launch of <= 1024 are resident at
// once, four to a CU, and the dispatcher deals an empty chip so that blocks b, b + 256, b + 512, b + 768
// share a CU (measured: tools/d1_tune.hip prints the hardware ids).  The kernel ends when its slowest CU
// does, so units are ranked by work (descending; ties by index, which makes the ranks a permutation)
// and dealt in a snake over the 256 CU slots: heaviest with lightest.  Units beyond the first 1024
// follow in descending order (they are dispatched as earlier ones finish: longest first).  A few
// microseconds, amortised over the decodes that reuse the plan (tools/d1_tune.hip: apply 80.4 -> 76.3 us
// at config 2).
constexpr unsigned kOrderMaxUnits = 4096;
// One WAVE per unit: its 64 lanes compare the unit's key with all n keys (each lane a strided share,
// read straight from L2), a wave reduction gives the rank.  (The first version - one THREAD per unit, every
// key compared from LDS - took 25 us for 1024 units: four workgroups, one wave per SIMD, 6 K vector
// instructions each at the single-wave issue rate.)
__global__ __launch_bounds__(256) void k_imdct_order(const unsigned *__restrict__ plan_work, unsigned n_units,
                                                      unsigned *__restrict__ order, unsigned ch, unsigned neighbours) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned u = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (u >= n_units) return;
  if (neighbours) {
    // (include/glc_debug.h variant 5, measurement only) the units that share a CU are consecutive frame
    // groups of one channel - similar unions, similar pace: they find each other's table rows in the CU's L1
    const unsigned n_fg = n_units / ch, rounds = n_units >> 8;
    const unsigned fg = u / ch, c = u - fg * ch;
    const unsigned v = c * n_fg + fg;  // channel-major
    if (lane == 0) order[(v % rounds) * 256u + v / rounds] = u;
    return;
  }
  const unsigned mine = plan_work[u];
  // rank = units with more work, or equal work and a lower index (ties by index make the ranks a permutation)
  unsigned cnt = 0;
  for (unsigned j = lane; j < n_units; j += 64u) {
    const unsigned k = plan_work[j];
    cnt += (k > mine || (k == mine && j < u)) ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  const unsigned rank = cnt;
  unsigned pos = rank;
  if (rank < 1024u) {
    const unsigned round = rank >> 8, p = rank & 255u;
    const unsigned in_round = min(256u, min(n_units, 1024u) - (round << 8));  // the last round may be partial
    pos = (round << 8) + ((round & 1u) ? in_round - 1u - p : p);
  }
  if (lane == 0) order[pos] = u;
}

// rows (r, r+1) x 8 columns, coefficient pair in SGPRs: the same instruction block as k1::mac2rows
__device__ __forceinline__ void d1_mac2rows_s(d1x2 (&c0)[4], d1x2 (&c1)[4], d1u2 a, d1x2 b0, d1x2 b1, d1x2 b2, d1x2 b3) {
  d1x2 t0, t1, t2, t3, t4, t5, t6, t7;
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
      : "s"(a), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
}

// The same block with a scalar branch around each row's half: a row that lacks the entry (+0.0, bits
// 0) costs two scalar instructions instead of 4 + 4 packed ones.  The branches live INSIDE the asm:
// written as C++ control flow around two asm blocks, hipcc re-allocates the 64 accumulators per arm
// and spills (128 VGPRs + scratch, 156 us instead of 108).
__device__ __forceinline__ void d1_mac2rows_fine_s(d1x2 (&c0)[4], d1x2 (&c1)[4], d1u2 a, d1x2 b0, d1x2 b1, d1x2 b2, d1x2 b3) {
  d1x2 t0, t1, t2, t3;
  asm volatile(
      "s_cmp_lg_u32 %13, 0\n\t"
      "s_cbranch_scc0 1f\n\t"
      "v_pk_mul_f32 %8, %12, %15 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %9, %12, %16 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %10, %12, %17 op_sel_hi:[0,1]\n\t"
      "v_pk_mul_f32 %11, %12, %18 op_sel_hi:[0,1]\n\t"
      "v_pk_add_f32 %0, %0, %8\n\t"
      "v_pk_add_f32 %1, %1, %9\n\t"
      "v_pk_add_f32 %2, %2, %10\n\t"
      "v_pk_add_f32 %3, %3, %11\n"
      "1:\n\t"
      "s_cmp_lg_u32 %14, 0\n\t"
      "s_cbranch_scc0 2f\n\t"
      "v_pk_mul_f32 %8, %12, %15 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %9, %12, %16 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %10, %12, %17 op_sel:[1,0]\n\t"
      "v_pk_mul_f32 %11, %12, %18 op_sel:[1,0]\n\t"
      "v_pk_add_f32 %4, %4, %8\n\t"
      "v_pk_add_f32 %5, %5, %9\n\t"
      "v_pk_add_f32 %6, %6, %10\n\t"
      "v_pk_add_f32 %7, %7, %11\n"
      "2:"
      : "+v"(c0[0]), "+v"(c0[1]), "+v"(c0[2]), "+v"(c0[3]), "+v"(c1[0]), "+v"(c1[1]), "+v"(c1[2]), "+v"(c1[3]),
        "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
      : "s"(a), "s"(a.x), "s"(a.y), "v"(b0), "v"(b1), "v"(b2), "v"(b3)
      : "scc");
}

// Two table rows per wave in registers: the one being applied and the next, in flight (four were
// measured and bought nothing: tools/d1_tune.hip, profiles/r02_d1_*).
template <bool SKIP, bool PRIO = true, bool FINE = true>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_imdct_apply(DeviceTables tb, const unsigned *__restrict__ plan_hdr, const unsigned *__restrict__ plan_rec,
                   const unsigned *__restrict__ order, unsigned n_frames, unsigned ch, unsigned group_begin, unsigned n_units,
                   float *__restrict__ blocks) {
  constexpr int G = 8, R = 2;
  // block -> unit (frame group, channel) of this batch.  (Speed only.)  All units of a launch of
  // <= 1024 are resident at once, four to a CU, and the dispatcher deals an empty chip so that blocks
  // b, b + 256, b + 512, b + 768 share a CU (measured: tools/d1_tune.hip prints the hardware ids).
  // Channels can differ in how many coefficients they keep (config 2: 985 against 1146 stored
  // non-zeros + union entries per unit), so the natural order - which hands a CU four units of ONE
  // channel whenever 256 % ch == 0 - leaves the slowest CU 14 % above the mean; rotating the channel
  // by the round (b / 256) of the frame group's first block gives every CU all channels (7 % above;
  // a full sort by work would reach 4 % but costs more than it returns: 10 us in the plan kernel).
  // ... or, when the launch has been ranked by work (k_imdct_order), the table says which unit this block takes.
  if (blockIdx.x >= n_units) return;
  unsigned fg, c;
  if (order) {
    const unsigned u = __builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    fg = u / ch;
    c = u - fg * ch;
  } else {
    fg = blockIdx.x / ch;
    c = (blockIdx.x - fg * ch + ((fg * ch) >> 8)) % ch;
  }
  const unsigned local = fg * ch + c;
  const unsigned fr0 = (group_begin + fg) * G;
  const unsigned *hdr = plan_hdr + static_cast<size_t>(local) * kPlanHdrDwords;
  const unsigned n_u = __builtin_amdgcn_readfirstlane(hdr[0]);
  const unsigned live = __builtin_amdgcn_readfirstlane(hdr[1]);
  if (!live) return;
  // The four waves of a SIMD are arbitrated oldest-first, so left alone they finish one after the
  // other and the last one runs by itself, with nobody to fill its scalar and wait slots.  Each wave
  // of a dense unit therefore lowers its own issue priority as it gets through its union (3 in the
  // first quarter ... 0 in the last): whoever is furthest behind goes first, the waves of a SIMD
  // progress together and keep covering each other's stalls to the end (config 2: D1 106 -> 92 us
  // with the per-row skip in place, 80 -> 76 us with fully shared indices; debug variant 3 is the
  // kernel without it).  Only for units whose rows share most indices, flagged by the plan kernel.
  const unsigned dense_unit = PRIO ? __builtin_amdgcn_readfirstlane(hdr[6]) : 0u;
  const unsigned q1 = n_u >> 2, q2 = n_u >> 1, q3 = q1 + q2;
  unsigned prio_next = dense_unit ? q1 : 0xFFFFFFFFu, prio_level = 0;  // scalar state: one compare per 4 entries
  // units that are not dense keep the top priority throughout: they are the long ones (the broadband
  // frames at a stream's edges double their union), and in a launch where every unit is like that
  // equal priorities change nothing
  if (PRIO) __builtin_amdgcn_s_setprio(3);
  const unsigned *rec = plan_rec + static_cast<size_t>(local) * kPlanRecCap * kPlanRecDwords;
  const unsigned col0 = static_cast<unsigned>(threadIdx.x) * 8u;  // 8 consecutive outputs per lane
  const unsigned lane_off = col0 * 4u;

  d1x2 acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int h = 0; h < 4; ++h) acc[g][h] = d1x2{0.f, 0.f};
  d1x4 t_lo[R], t_hi[R];
  d1u8 ca, cb, cc, cd;        // records of the pair being applied (ca, cb) and of the next pair (cc, cd)
  unsigned ka, kb, kc, kd;
  auto issue_tab = [&](d1x4 &lo, d1x4 &hi, unsigned koff) {
    const unsigned long long row = reinterpret_cast<unsigned long long>(tb.cos) + koff;  // scalar ALU
    asm volatile(
        "global_load_dwordx4 %0, %2, %3\n\t"
        "global_load_dwordx4 %1, %2, %3 offset:16"
        : "=&v"(lo), "=&v"(hi)
        : "v"(lane_off), "s"(row)
        : "memory");
  };
#pragma unroll
  for (int r = 0; r < R; ++r) issue_tab(t_lo[r], t_hi[r], __builtin_amdgcn_readfirstlane(hdr[2 + r]));  // entries 0, 1
  // Records are fetched TWO entries at a time, a whole pair of entries ahead: scalar loads return out
  // of order, so the only safe wait is lgkmcnt(0), which covers everything issued so far - fetching
  // every other entry doubles the time each fetch has before it is waited for (measured on the
  // config-2 batch: 107 -> 95 us, profiles/r02_d1_tune_real_rows.txt).  Scalar and vector operands
  // sit in SEPARATE asm statements: LLVM treats every output of an asm that has one VGPR output as
  // divergent, and a "divergent" row offset would be added on the vector ALU.
#define GLC_D1_FETCH2(C0, K0, C1, K1, J)                                                                          \
  do {                                                                                                          \
    const unsigned *nrec = rec + static_cast<size_t>(J) * kPlanRecDwords;                                        \
    asm volatile(                                                                                               \
        "s_load_dwordx8 %0, %4, 0x0\n\ts_load_dword %1, %4, 0x20\n\ts_load_dwordx8 %2, %4, 0x40\n\ts_load_dword %3, %4, 0x60" \
        : "=&s"(C0), "=&s"(K0), "=&s"(C1), "=&s"(K1)                                                             \
        : "s"(nrec)                                                                                             \
        : "memory");                                                                                            \
  } while (0)
#define GLC_D1_WAIT2(C0, K0, C1, K1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(C0), "+s"(K0), "+s"(C1), "+s"(K1)::"memory")
  // One entry.  S: its table slot; CC: its 8 coefficients; KC: table offset of entry J + R, whose row
  // refills slot S.  Of the table loads only those of the R - 1 following entries may be in flight.
#define GLC_D1_PAIR(S, P, A0, A1)                                                                                \
  do {                                                                                                          \
    if (SKIP && FINE) {                                                                                          \
      if (P.x | P.y) d1_mac2rows_fine_s(acc[A0], acc[A1], P, t_lo[S].xy, t_lo[S].zw, t_hi[S].xy, t_hi[S].zw);      \
    } else if (!SKIP || (P.x | P.y)) {                                                                           \
      d1_mac2rows_s(acc[A0], acc[A1], P, t_lo[S].xy, t_lo[S].zw, t_hi[S].xy, t_hi[S].zw);                         \
    }                                                                                                           \
  } while (0)
#define GLC_D1_ENTRY(S, CC, KC)                                                                                  \
  do {                                                                                                          \
    asm volatile("s_waitcnt vmcnt(2)" : "+v"(t_lo[S]), "+v"(t_hi[S])::"memory");                                  \
    const d1u2 p0 = CC.s01, p1 = CC.s23, p2 = CC.s45, p3 = CC.s67;                                               \
    GLC_D1_PAIR(S, p0, 0, 1);                                                                                    \
    GLC_D1_PAIR(S, p1, 2, 3);                                                                                    \
    GLC_D1_PAIR(S, p2, 4, 5);                                                                                    \
    GLC_D1_PAIR(S, p3, 6, 7);                                                                                    \
    issue_tab(t_lo[S], t_hi[S], KC);                                                                             \
  } while (0)
  GLC_D1_FETCH2(ca, ka, cb, kb, 0);
  unsigned j = 0;
#pragma unroll 1
  for (; j + 4 <= n_u; j += 4) {
    if (j >= prio_next) {  // crossed a quarter of the union: three times per wave
      ++prio_level;
      if (prio_level == 1) __builtin_amdgcn_s_setprio(2);
      else if (prio_level == 2) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
      prio_next = prio_level == 1 ? q2 : prio_level == 2 ? q3 : 0xFFFFFFFFu;
    }
    GLC_D1_WAIT2(ca, ka, cb, kb);
    GLC_D1_FETCH2(cc, kc, cd, kd, j + 2);
    GLC_D1_ENTRY(0, ca, ka);
    GLC_D1_ENTRY(1, cb, kb);
    GLC_D1_WAIT2(cc, kc, cd, kd);
    GLC_D1_FETCH2(ca, ka, cb, kb, j + 4);
    GLC_D1_ENTRY(0, cc, kc);
    GLC_D1_ENTRY(1, cd, kd);
  }
  if (j < n_u) {  // 1..3 entries left; (ca, cb) hold entries j, j + 1
    GLC_D1_WAIT2(ca, ka, cb, kb);
    GLC_D1_FETCH2(cc, kc, cd, kd, j + 2);
    GLC_D1_ENTRY(0, ca, ka);
    if (j + 1 < n_u) {
      GLC_D1_ENTRY(1, cb, kb);
      if (j + 2 < n_u) {
        GLC_D1_WAIT2(cc, kc, cd, kd);
        GLC_D1_ENTRY(0, cc, kc);
      }
    }
  }
#undef GLC_D1_ENTRY
#undef GLC_D1_PAIR
#undef GLC_D1_FETCH2
#undef GLC_D1_WAIT2
  // drain the run-ahead loads before their registers are reused
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ca), "+s"(cb), "+s"(cc), "+s"(cd), "+s"(ka), "+s"(kb), "+s"(kc), "+s"(kd)::"memory");
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(t_lo[0]), "+v"(t_hi[0]), "+v"(t_lo[1]), "+v"(t_hi[1])::"memory");

  const d1x4 w0 = *reinterpret_cast<const d1x4 *>(tb.window + col0), w1 = *reinterpret_cast<const d1x4 *>(tb.window + col0 + 4);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (!(live & (1u << g))) continue;
    float *out = blocks + static_cast<size_t>((fr0 + g) * ch + c) * kFrameI + col0;
    d1x4 o0, o1;  // out[i] = s*norm (:388) then *= window[i] (:674)
    o0.x = mul_rn(mul_rn(acc[g][0].x, tb.norm), w0.x); o0.y = mul_rn(mul_rn(acc[g][0].y, tb.norm), w0.y);
    o0.z = mul_rn(mul_rn(acc[g][1].x, tb.norm), w0.z); o0.w = mul_rn(mul_rn(acc[g][1].y, tb.norm), w0.w);
    o1.x = mul_rn(mul_rn(acc[g][2].x, tb.norm), w1.x); o1.y = mul_rn(mul_rn(acc[g][2].y, tb.norm), w1.y);
    o1.z = mul_rn(mul_rn(acc[g][3].x, tb.norm), w1.z); o1.w = mul_rn(mul_rn(acc[g][3].y, tb.norm), w1.w);
    *reinterpret_cast<d1x4 *>(out) = o0;
    *reinterpret_cast<d1x4 *>(out + 4) = o1;
  }
}

// ------------------------------------------------------------------------------------------
// D2: overlap-add + interleave.  blocks holds frames [blk_frame0, ...) as [frame][ch][2048];
// hop h = second half of frame h-1 (+0.0 before the first frame) + first half of frame h; the
// hop after the last frame is the bare overlap tail (no add, src/codec.rs:722-729).
// Three kernels - whole hops of one stream (k_overlap_add), kept spans of many streams by descriptor
// (k_overlap_add_strided) and its planar form (k_overlap_add_planar) - over ONE sum and ONE store.
// ------------------------------------------------------------------------------------------
// The sample at position `at` of the two half blocks: prev = second half of the frame before, cur = first half
// of the frame itself, either of which may be absent.
__device__ __forceinline__ float d2_sum(const float *prev, const float *cur, bool has_prev, bool has_cur, size_t at) {
  const float p = has_prev ? prev[at] : 0.0f;  // overlap starts as +0.0, :601
  return has_cur ? add_rn(p, cur[at]) : p;      // :695 / the bare tail, :727
}

// ... at interleaved index o of the hop ([ch][2048] blocks): 32-bit index arithmetic, shifts for CH = 1 / 2 / 4 / 8,
// one 32-bit division per sample for CH = 0 (any channel count).
template <int CH>
__device__ __forceinline__ float d2_sample(const float *prev, const float *cur, bool has_prev, bool has_cur, unsigned ch,
                                           unsigned o) {
  unsigned i, c;
  if constexpr (CH == 1) i = o, c = 0;
  else if constexpr (CH == 2) i = o >> 1, c = o & 1u;
  else if constexpr (CH == 4) i = o >> 2, c = o & 3u;
  else if constexpr (CH == 8) i = o >> 3, c = o & 7u;
  else i = o / ch, c = o - i * ch;
  return d2_sum(prev, cur, has_prev, has_cur, static_cast<size_t>(c) * kFrameI + i);
}

// Four consecutive output samples to dst: as one float4 / short4 when all four are kept and dst is aligned to
// the vector (ALIGNED), else the kept ones element by element.  T = short narrows as the reference's 16-bit
// writers do (convert_f32_to_i16: `(s * 32767.0).clamp(-32768.0, 32767.0) as i16`, src/audio.rs:11-16).
template <bool ALIGNED, typename T>
__device__ __forceinline__ void d2_store(const float (&v)[4], T *dst, const bool (&keep)[4]) {
  static_assert(std::is_same<T, float>::value || std::is_same<T, short>::value, "float or 16-bit PCM");
  using T4 = typename std::conditional<std::is_same<T, float>::value, float4, short4>::type;
  T q[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (std::is_same<T, float>::value) q[e] = v[e];
    else q[e] = sat_i16(mul_rn(v[e], 32767.0f));  // src/audio.rs:13-14
  }
  if (ALIGNED && keep[0] && keep[3]) {
    *reinterpret_cast<T4 *>(dst) = T4{q[0], q[1], q[2], q[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (keep[e]) dst[e] = q[e];
  }
}

// One workgroup row (blockIdx.y) per hop, four interleaved output samples per thread: coalesced 16-byte
// stores (8-byte ones of 16-bit PCM, so that the host boundary of a decode moves 2 bytes per sample), each
// block plane read in runs of consecutive samples.  (Round 2's kernel walked the output
// with a 64-bit grid-stride index: two 64-bit divisions per sample - 20 us at config 2, as long as the
// 100 MB it moves take at Infinity-Cache speed.)
// VEC = false: a destination that is only element-aligned (glc_decode_range_device takes any device pointer).
template <int CH, bool VEC, typename T>
__global__ __launch_bounds__(256) void k_overlap_add(const float *__restrict__ blocks, long long blk_frame0,
                                                      unsigned long long n_frames, unsigned ch,
                                                      unsigned long long hop_begin, T *__restrict__ out) {
  const unsigned per_hop = static_cast<unsigned>(kHopI) * ch;
  const unsigned o0 = (blockIdx.x * 256u + threadIdx.x) * 4u;  // first of this thread's 4 outputs inside the hop
  if (o0 >= per_hop) return;
  const unsigned long long h = hop_begin + blockIdx.y;
  const bool has_prev = h >= 1, has_cur = h < n_frames;
  // frame h-1 (second half) and frame h (first half) of the ring: [slot][ch][2048]
  const float *prev = blocks + (static_cast<size_t>(static_cast<long long>(h) - 1 - blk_frame0) * ch) * kFrameI + kHopI;
  const float *cur = blocks + (static_cast<size_t>(static_cast<long long>(h) - blk_frame0) * ch) * kFrameI;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = d2_sample<CH>(prev, cur, has_prev, has_cur, ch, o0 + e);
  constexpr bool all[4] = {true, true, true, true};
  d2_store<VEC>(v, out + static_cast<size_t>(blockIdx.y) * per_hop + o0, all);
}

// D2 by descriptor (the batch drivers): one workgroup row per KEPT output hop, described by a HopDescStrided (or a
// HopDesc, D: the same with a 32-bit destination) -
// the block slots of the frame before (second half) and of the frame itself (first half), either of which may
// be absent (-1: the first hop of a stream starts from +0.0, its last hop is the bare tail), and the span
// [first, first + cnt) of the hop's interleaved samples that survives the stream's gapless trim, which lands at
// out[dst ..).  dst is any element index and `out` any element-aligned pointer, so the threads are laid over the
// destination ADDRESS: chunk k of a hop is the four elements from the vector boundary at or below out + dst on,
// and goes out as one float4 / short4; only the first and the last chunk of a cut span can be partial, and those
// store element by element.  Same sums as k_overlap_add; T = short (glc_decode_batch_i16) narrows as it does.
template <int CH, typename T, typename D>
__global__ __launch_bounds__(256) void k_overlap_add_strided(const float *__restrict__ blocks, const D *__restrict__ desc,
                                                              unsigned ch, T *__restrict__ out) {
  const D d = desc[blockIdx.y];
  T *span = out + d.dst;
  const unsigned lead = static_cast<unsigned>(reinterpret_cast<uintptr_t>(span) / sizeof(T)) & 3u;
  const unsigned n_chunks = (lead + d.cnt + 3u) >> 2;
  const bool has_prev = d.prev >= 0, has_cur = d.cur >= 0;
  const float *prev = blocks + (static_cast<size_t>(has_prev ? d.prev : 0) * ch) * kFrameI + kHopI;
  const float *cur = blocks + (static_cast<size_t>(has_cur ? d.cur : 0) * ch) * kFrameI;
  T *base = span - lead;
  for (unsigned k = blockIdx.x * 256u + threadIdx.x; k < n_chunks; k += gridDim.x * 256u) {
    const int j0 = static_cast<int>(4u * k) - static_cast<int>(lead);  // first of the chunk, counted from the span's start
    float v[4];
    bool keep[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      keep[e] = j >= 0 && static_cast<unsigned>(j) < d.cnt;
      v[e] = d2_sample<CH>(prev, cur, has_prev, has_cur, ch, d.first + static_cast<unsigned>(keep[e] ? j : 0));
    }
    d2_store<true>(v, base + 4u * static_cast<size_t>(k), keep);
  }
}

// Planar: workgroup (blockIdx.x = plane c, blockIdx.y = hop).  The hop keeps the clip's interleaved samples
// [j0, j0 + cnt) (sample j is time j / ch of plane j % ch - the trim is counted in interleaved samples, so with 3 or
// 6 channels a hop's span starts at a different time in different planes); plane c gets the times t with
// j0 <= t * ch + c < j0 + cnt, at most 1025 of them, consecutive in memory.  A thread owns an aligned float4 of
// the plane: four consecutive times, whose samples are four consecutive entries of ONE block plane - position
// i0 + (t - t_lo) of block channel cc, one division per thread.  Only the first and the last chunk of a span
// can be partial; they store float by float.  T = short: the same over aligned short4 of the plane (8-byte
// boundaries), narrowed as d2_store narrows.
template <typename T>
__global__ __launch_bounds__(256) void k_overlap_add_planar(const float *__restrict__ blocks,
                                                             const HopDescStrided *__restrict__ desc, unsigned ch,
                                                             T *__restrict__ out) {
  const HopDescStrided d = desc[blockIdx.y];
  const unsigned c = blockIdx.x;
  const unsigned long long j1 = d.j0 + d.cnt;
  const unsigned long long t_lo = d.j0 > c ? (d.j0 - c + ch - 1) / ch : 0ull, t_hi = j1 > c ? (j1 - c + ch - 1) / ch : 0ull;
  if (t_hi <= t_lo) return;
  const unsigned n = static_cast<unsigned>(t_hi - t_lo);
  const unsigned o0 = d.first + static_cast<unsigned>(t_lo * ch + c - d.j0);  // the hop's interleaved index of (t_lo, c)
  const unsigned i0 = o0 / ch, cc = o0 - i0 * ch;
  const bool has_prev = d.prev >= 0, has_cur = d.cur >= 0;
  const float *prev = blocks + (static_cast<size_t>(has_prev ? d.prev : 0) * ch + cc) * kFrameI + kHopI + i0;
  const float *cur = blocks + (static_cast<size_t>(has_cur ? d.cur : 0) * ch + cc) * kFrameI + i0;
  T *span = out + d.dst + c * d.cstride + t_lo;
  const unsigned lead = static_cast<unsigned>(reinterpret_cast<uintptr_t>(span) / sizeof(T)) & 3u;
  const unsigned n_chunks = (lead + n + 3u) >> 2;
  T *base = span - lead;
  for (unsigned k = threadIdx.x; k < n_chunks; k += 256u) {
    const int j0 = static_cast<int>(4u * k) - static_cast<int>(lead);
    float v[4];
    bool keep[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      keep[e] = j >= 0 && static_cast<unsigned>(j) < n;
      v[e] = d2_sum(prev, cur, has_prev, has_cur, static_cast<unsigned>(keep[e] ? j : 0));
    }
    d2_store<true>(v, base + 4u * static_cast<size_t>(k), keep);
  }
}

// ------------------------------------------------------------------------------------------
// W1: integer PCM -> f32, what the reference's loaders do on the host (`s as f32 / (1 << (bits-1))
// as f32`, src/audio.rs:58, :79).  `(float)s` rounds to nearest even beyond 24 bits like `as f32`;
// the divisor is +-2^k, so the quotient is the product with `inv` = 1/divisor, which is exact too
// (no result is subnormal: |s| >= 1 gives at least 2^-31) - same bits, no division.
// Memory-bound: 6 (i16) or 8 (i32) bytes per sample.  The body starts where the DESTINATION is
// 16-byte aligned: a float4 store per thread from four samples, loaded as one 8- / 16-byte word
// when the source is aligned there too (VEC), else one by one.  The at most 3 + 3 samples in front
// of and behind the body are converted by the threads after the body's.
// ------------------------------------------------------------------------------------------
// The ONE conversion of an integer sample, for W1 and for the widening gather S1 (k_stage_clips*): the host
// boundary and the store cannot drift apart.
template <typename S>
__device__ __forceinline__ float pcm_widen1(S s, float inv) {
  return mul_rn(static_cast<float>(s), inv);
}

template <typename S, bool VEC>
__global__ __launch_bounds__(256) void k_pcm_widen(const S *__restrict__ in, float *__restrict__ out,
                                                    unsigned long long n, unsigned head, float inv) {
  const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * 256u + threadIdx.x;
  const unsigned long long n4 = (n - head) / 4u;  // float4s of the body (head <= n)
  if (g < n4) {
    const unsigned long long at = head + g * 4u;
    float4 v;
    if constexpr (VEC && sizeof(S) == 2) {
      const short4 s = *reinterpret_cast<const short4 *>(in + at);
      v = float4{pcm_widen1(s.x, inv), pcm_widen1(s.y, inv), pcm_widen1(s.z, inv), pcm_widen1(s.w, inv)};
    } else if constexpr (VEC) {
      const int4 s = *reinterpret_cast<const int4 *>(in + at);
      v = float4{pcm_widen1(s.x, inv), pcm_widen1(s.y, inv), pcm_widen1(s.z, inv), pcm_widen1(s.w, inv)};
    } else {
      v = float4{pcm_widen1(in[at], inv), pcm_widen1(in[at + 1], inv), pcm_widen1(in[at + 2], inv), pcm_widen1(in[at + 3], inv)};
    }
    *reinterpret_cast<float4 *>(out + at) = v;
    return;
  }
  const unsigned long long e = g - n4;  // 0 .. head-1: the head; then the tail behind the body
  const unsigned long long at = e < head ? e : 4u * n4 + e;
  if (at < n) out[at] = pcm_widen1(in[at], inv);
}

// ------------------------------------------------------------------------------------------
// The two-level exclusive scan of P1 / P2 and of R2: how many pairs, and how many rows of raw frames, lie in
// front of row m.  A row contributes ONE packed word - its pair count in the low RAW_SHIFT bits, or
// 1 << RAW_SHIFT for a row of a raw frame (the high 11 bits: fewer than 1024 such rows in front of a row of its
// block) - so one scan carries both counts.
//   scan_rows_1024   a workgroup of 256 threads scans 1024 rows: 4 per thread, Hillis-Steele over the 256 thread
//                    sums in LDS; loc[m] = the sum in front of row m inside its block, and the block's two
//                    sums go to blk / blk_raw.  count(m) is the word of row m < M (and whatever per-row
//                    stores its kernel wants made on the way).
//   scan_block_sums  ONE workgroup of 1024 threads: blk and blk_raw become their own exclusive scans, in
//                    chunks of 1024 with a carry; sums[] = the two totals.  No workgroup waits for another.
//   rows_before      (loc word, blk, blk_raw, m) -> {pairs, rows of raw frames} in front of row m
// P1 scans unsigned words (<= 1024 * 1024 pairs in a block: 21 bits; a wider word would double loc), R2 unsigned
// long long ones (cnt is what a blob claims: <= 1024 * (2^32 - 1), 53 bits).
// ------------------------------------------------------------------------------------------
constexpr int kP1RawShift = 21, kR2RawShift = 53;

template <typename W, int RAW_SHIFT, typename F>
__device__ __forceinline__ void scan_rows_1024(F count, unsigned M, W *__restrict__ loc, unsigned long long *__restrict__ blk,
                                               unsigned long long *__restrict__ blk_raw) {
  static_assert(RAW_SHIFT + 11 == 8 * sizeof(W), "pairs | 11 bits of raw rows fill the word");
  __shared__ W s_part[256];
  const unsigned base = blockIdx.x * 1024u + threadIdx.x * 4u;
  W v[4], sum = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const W n = base + j < M ? count(base + j) : W(0);
    v[j] = sum;  // exclusive within the thread
    sum += n;
  }
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // Hillis-Steele inclusive scan of the 256 thread sums
    const W t = threadIdx.x >= static_cast<unsigned>(off) ? s_part[threadIdx.x - off] : W(0);
    __syncthreads();
    s_part[threadIdx.x] += t;
    __syncthreads();
  }
  const W before = threadIdx.x ? s_part[threadIdx.x - 1] : W(0);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (base + j < M) loc[base + j] = before + v[j];
  if (threadIdx.x == 255) {
    blk[blockIdx.x] = s_part[255] & ((W(1) << RAW_SHIFT) - 1);
    blk_raw[blockIdx.x] = s_part[255] >> RAW_SHIFT;
  }
}

// A workgroup of 1024 threads: s[t] becomes the sum of the `mine` of threads 0 .. t (Hillis-Steele, inclusive).
__device__ __forceinline__ void scan_sum_1024(unsigned long long *s /* LDS, [1024] */, unsigned long long mine) {
  s[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const unsigned long long t = threadIdx.x >= static_cast<unsigned>(off) ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
}

__device__ __forceinline__ void scan_block_sums(unsigned long long *__restrict__ blk, unsigned long long *__restrict__ blk_raw,
                                                unsigned n, unsigned long long *s /* LDS, [1024] */,
                                                unsigned long long sums[2]) {
#pragma unroll 1
  for (int which = 0; which < 2; ++which) {
    unsigned long long *v = which ? blk_raw : blk;
    unsigned long long carry = 0;
    for (unsigned b0 = 0; b0 < n; b0 += 1024) {
      const unsigned i = b0 + threadIdx.x;
      const unsigned long long mine = i < n ? v[i] : 0ull;
      scan_sum_1024(s, mine);
      if (i < n) v[i] = carry + s[threadIdx.x] - mine;  // exclusive
      const unsigned long long chunk_total = s[1023];
      __syncthreads();
      carry += chunk_total;
    }
    sums[which] = carry;
  }
}

struct RowsBefore {
  unsigned long long pairs, raw;
};
template <int RAW_SHIFT, typename W>
__device__ __forceinline__ RowsBefore rows_before(W l, const unsigned long long *__restrict__ blk,
                                                  const unsigned long long *__restrict__ blk_raw, unsigned long long m) {
  return {blk[m >> 10] + (l & ((W(1) << RAW_SHIFT) - 1)), blk_raw[m >> 10] + (l >> RAW_SHIFT)};
}

// ------------------------------------------------------------------------------------------
// P1-P3: device-side compaction of frame records into the compact blob (glc_common.h
// CompactLayout `l`: every kernel takes the blob and its layout, none an offset of its own), so that the host
// boundary and the multi-GPU gather move (u16 idx, i16 q) pairs instead of dense 1024-bin rows.
//   P1  scan_rows_1024 over the pairs a row contributes (nnz, 0 for rows of raw frames); on the way the
//       per-row scale and count and the per-frame raw flag into the blob
//   P2  scan_block_sums, then the blob header the totals determine and the zeroed alignment gap in front
//       of the raw section
//   P3  one wave per row: ballot + popcount prefix keeps ascending k (src/codec.rs:303-306);
//       planes of raw-frame rows go to the raw section, which starts behind the pairs
// ------------------------------------------------------------------------------------------
// SEG (glc_encode_batch): row m belongs to frame m / ch of the round's REAL frames, whose record is number
// fmap[frame].x of the virtual stream's records - the junk frame behind every clip is in no one's map,
// so nothing of it is counted, packed or sent.  fmap[frame].y is the clip that starts at this frame
// (~0u: none): P3 leaves that clip's first pair and first raw row in dir[2 * clip], dir[2 * clip + 1].
template <bool SEG>
__global__ __launch_bounds__(256) void k_pack_scan_rows(const unsigned char *__restrict__ records, unsigned M,
                                                         unsigned ch, unsigned long long rec_bytes,
                                                         unsigned *__restrict__ loc,
                                                         unsigned long long *__restrict__ blk,
                                                         unsigned long long *__restrict__ blk_raw, CompactLayout l,
                                                         unsigned char *__restrict__ blob,
                                                         const uint2 *__restrict__ fmap) {
  float *scales = reinterpret_cast<float *>(blob + l.o_scale);
  unsigned *cnt = reinterpret_cast<unsigned *>(blob + l.o_cnt);
  unsigned char *is_raw = blob + l.o_israw;
  scan_rows_1024<unsigned, kP1RawShift>(
      [&](unsigned m) {
        const unsigned frame = m / ch, c = m % ch;
        const unsigned slot = SEG ? fmap[frame].x : frame;
        const unsigned char *rec = records + static_cast<size_t>(slot) * rec_bytes;
        const unsigned raw = record_raw(rec);
        const unsigned nnz = min(record_nnz(rec, c), static_cast<unsigned>(kHopI));
        scales[m] = record_scale(rec, c);
        cnt[m] = raw ? 0u : nnz;
        if (c == 0) is_raw[frame] = raw ? 1 : 0;
        return raw ? (1u << kP1RawShift) : nnz;
      },
      M, loc, blk, blk_raw);
}

__global__ __launch_bounds__(1024) void k_pack_scan_blocks(unsigned long long *__restrict__ blk,
                                                            unsigned long long *__restrict__ blk_raw, unsigned n,
                                                            unsigned long long *__restrict__ totals, unsigned ch,
                                                            unsigned long long n_frames, CompactLayout l,
                                                            unsigned char *__restrict__ blob) {
  __shared__ unsigned long long s[1024];
  unsigned long long sums[2];
  scan_block_sums(blk, blk_raw, n, s, sums);
  const unsigned long long n_pairs = sums[0], n_raw_rows = sums[1];
  const unsigned long long pairs_end = l.o_pairs + 4ull * n_pairs, raw_off = compact_raw_offset(l, n_pairs);
  if (threadIdx.x == 0) {
    totals[0] = n_pairs;
    totals[1] = n_raw_rows;
    *reinterpret_cast<CompactHeader *>(blob) = compact_header(ch, n_frames, n_pairs, n_raw_rows, raw_off + n_raw_rows * 4096ull);
  }
  if (threadIdx.x < 64 && pairs_end + threadIdx.x < raw_off) blob[pairs_end + threadIdx.x] = 0;  // deterministic padding
}

// What one wave does with row `qrow` (the 2048 i16 of channel c behind a record's header) in P3 and A3.  Row of a raw
// frame: its 2048-sample plane goes to raw_dst (planar order == row order, Q1).  Otherwise ballot + popcount
// prefix keeps ascending k: the first `room` non-zero bins below 1024 go to dst as (k | u16(q) << 16).  `room` is
// the count the scan saw: a record whose nnz field disagrees with its row cannot write past its slot.
__device__ __forceinline__ void pack_row(const short *__restrict__ qrow, bool raw, short4 *__restrict__ raw_dst,
                                         unsigned *__restrict__ dst, unsigned room, int lane) {
  if (raw) {
    const short4 *src = reinterpret_cast<const short4 *>(qrow);
    for (int i = lane; i < kFrameI / 4; i += 64) raw_dst[i] = src[i];
    return;
  }
  unsigned done = 0;
  for (int k0 = 0; k0 < kHopI; k0 += 64) {
    const short q = qrow[k0 + lane];
    const unsigned long long mask = __ballot(q != 0);
    if (q != 0) {
      const unsigned pos = done + __popcll(mask & ((1ull << lane) - 1ull));
      if (pos < room)
        dst[pos] = static_cast<unsigned>(k0 + lane) | (static_cast<unsigned>(static_cast<unsigned short>(q)) << 16);
    }
    done += __popcll(mask);
  }
  // fewer non-zeros than the nnz field claims: fill the rest of the slot (idx 0xFFFF is ignored by
  // every reader, src/codec.rs:660) so the blob never carries uninitialised bytes
  for (unsigned pos = done + lane; pos < room; pos += 64) dst[pos] = 0xFFFFu;
}

template <bool SEG>
__global__ __launch_bounds__(256) void k_pack_rows(const unsigned char *__restrict__ records, unsigned M,
                                                    unsigned ch, unsigned long long rec_bytes,
                                                    unsigned long long hdr_bytes, const unsigned *__restrict__ loc,
                                                    const unsigned long long *__restrict__ blk,
                                                    const unsigned long long *__restrict__ blk_raw,
                                                    const unsigned long long *__restrict__ totals, CompactLayout l,
                                                    unsigned char *__restrict__ blob, const uint2 *__restrict__ fmap,
                                                    unsigned long long *__restrict__ dir) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned m = blockIdx.x * 4 + w;
  if (m >= M) return;
  const RowsBefore at = rows_before<kP1RawShift>(loc[m], blk, blk_raw, m);
  const unsigned frame = m / ch, c = m % ch;
  unsigned slot = frame;
  if constexpr (SEG) {
    const uint2 fm = fmap[frame];
    slot = fm.x;
    if (c == 0 && lane == 0 && fm.y != ~0u) {  // a clip starts here: what the round holds in front of it
      dir[2ull * fm.y] = at.pairs;
      dir[2ull * fm.y + 1] = at.raw;
    }
  }
  const unsigned char *rec = records + static_cast<size_t>(slot) * rec_bytes;
  const short *qrow = reinterpret_cast<const short *>(rec + hdr_bytes) + static_cast<size_t>(c) * kFrameI;
  const bool raw = record_raw(rec) != 0;
  // the raw section starts behind the pairs; the room of a compressed row is the count P1 left in the blob
  short4 *raw_dst = raw ? reinterpret_cast<short4 *>(blob + compact_raw_offset(l, totals[0]) + at.raw * (kFrameI * 2ull)) : nullptr;
  const unsigned room = raw ? 0u : reinterpret_cast<const unsigned *>(blob + l.o_cnt)[m];
  pack_row(qrow, raw, raw_dst, reinterpret_cast<unsigned *>(blob + l.o_pairs) + at.pairs, room, lane);
}

// ------------------------------------------------------------------------------------------
// A1-A3: the pack of a round of glc_encode_batch_device_compact - ONE SELF-DESCRIBING BLOB PER CLIP (the single-stream
// CompactLayout of the clip's own frames, no directory), the blobs back to back in an arena from a cursor the
// device keeps.  fmap[frame] = {record slot, clip of the round} for EVERY real frame (R1's form), clips[k] =
// {first real frame, frames} of clip k of the round, entries[k] its glc_store_entry (include/glc.h) as four
// 64-bit words {offset, bytes, n_pairs, n_raw_rows | stored << 32}.
//   A1  scan_rows_1024 over the word a row contributes, values only: where a clip's sections lie is not known yet
//   A2  ONE workgroup: scan_block_sums; per clip its pairs and raw rows as differences of rows_before at its first
//       row and behind its last, its size from compact_layout / compact_raw_offset; the exclusive scan of the sizes
//       over the clips from the cursor rounded up to 64, in chunks of 1024 clips with a carry; the fit decision,
//       every entry, the header of every stored blob, and the cursor behind the last clip - stored or not
//   A3  one wave per real row: scale, count, raw flag and the row's list or plane (pack_row) at their clip-relative
//       places; the wave of a clip's first row zeroes the alignment gaps of its sections.  Rows of clips that did
//       not fit return at once: nothing of such a clip is written.
// Ordinary stores only; the cursor needs no atomics because rounds run in stream order.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned store_row_word(const unsigned char *__restrict__ rec, unsigned c) {
  const unsigned nnz = min(record_nnz(rec, c), static_cast<unsigned>(kHopI));
  return record_raw(rec) ? (1u << kP1RawShift) : nnz;
}

__global__ __launch_bounds__(256) void k_store_scan_rows(const unsigned char *__restrict__ records, unsigned M, unsigned ch,
                                                          unsigned long long rec_bytes, unsigned *__restrict__ loc,
                                                          unsigned long long *__restrict__ blk,
                                                          unsigned long long *__restrict__ blk_raw,
                                                          const uint2 *__restrict__ fmap) {
  scan_rows_1024<unsigned, kP1RawShift>(
      [&](unsigned m) { return store_row_word(records + static_cast<size_t>(fmap[m / ch].x) * rec_bytes, m % ch); }, M, loc, blk,
      blk_raw);
}

__global__ __launch_bounds__(1024) void k_store_place(unsigned long long *blk, unsigned long long *blk_raw, unsigned nblk,
                                                       const unsigned *__restrict__ loc, unsigned M, unsigned ch,
                                                       const uint2 *__restrict__ clips, unsigned n_clips,
                                                       unsigned long long *__restrict__ clip_base,
                                                       unsigned char *__restrict__ arena, unsigned long long arena_bytes,
                                                       unsigned long long *cursor, unsigned long long *__restrict__ entries) {
  __shared__ unsigned long long s[1024];
  unsigned long long sums[2];
  scan_block_sums(blk, blk_raw, nblk, s, sums);
  const unsigned long long all_pairs = sums[0], all_raw = sums[1];
  auto before = [=](unsigned long long row) {  // rows_before, also of the row behind the last
    const unsigned long long at = row < M ? row : M - 1;
    const RowsBefore r = rows_before<kP1RawShift>(loc[at], blk, blk_raw, at);
    return RowsBefore{row < M ? r.pairs : all_pairs, row < M ? r.raw : all_raw};
  };
  unsigned long long carry = align64(*cursor);  // every thread reads it here; thread 0 writes it behind the last barrier
  for (unsigned k0 = 0; k0 < n_clips; k0 += 1024) {
    const unsigned k = k0 + threadIdx.x;
    unsigned long long bytes = 0, n_pairs = 0, n_raw_rows = 0, n_frames = 0;
    if (k < n_clips) {
      const uint2 cl = clips[k];
      n_frames = cl.y;
      const unsigned long long r0 = static_cast<unsigned long long>(cl.x) * ch;
      const RowsBefore a = before(r0), b = before(r0 + n_frames * ch);
      n_pairs = b.pairs - a.pairs;
      n_raw_rows = b.raw - a.raw;
      clip_base[2ull * k] = a.pairs;
      clip_base[2ull * k + 1] = a.raw;
      bytes = compact_raw_offset(compact_layout(ch, n_frames), n_pairs) + n_raw_rows * (kFrameI * 2ull);
    }
    scan_sum_1024(s, bytes);
    const unsigned long long offset = carry + s[threadIdx.x] - bytes;  // exclusive: every size is a multiple of 64
    const unsigned long long chunk_total = s[1023];
    __syncthreads();
    carry += chunk_total;
    if (k < n_clips) {
      const bool stored = offset <= arena_bytes && bytes <= arena_bytes - offset;
      unsigned long long *e = entries + 4ull * k;
      e[0] = offset;
      e[1] = bytes;
      e[2] = n_pairs;
      e[3] = n_raw_rows | (stored ? 1ull << 32 : 0ull);
      if (stored) *reinterpret_cast<CompactHeader *>(arena + offset) = compact_header(ch, n_frames, n_pairs, n_raw_rows, bytes);
    }
  }
  if (threadIdx.x == 0) *cursor = carry;
}

__global__ __launch_bounds__(256) void k_store_rows(const unsigned char *__restrict__ records, unsigned M, unsigned ch,
                                                     unsigned long long rec_bytes, unsigned long long hdr_bytes,
                                                     const unsigned *__restrict__ loc, const unsigned long long *__restrict__ blk,
                                                     const unsigned long long *__restrict__ blk_raw,
                                                     const unsigned long long *__restrict__ clip_base,
                                                     const uint2 *__restrict__ fmap, const uint2 *__restrict__ clips,
                                                     const unsigned long long *__restrict__ entries,
                                                     unsigned char *__restrict__ arena) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned m = blockIdx.x * 4 + w;
  if (m >= M) return;
  const unsigned frame = m / ch, c = m % ch;
  const uint2 fm = fmap[frame];
  const unsigned long long *e = entries + 4ull * fm.y;
  if ((e[3] >> 32) == 0) return;  // the clip did not fit
  const uint2 cl = clips[fm.y];
  const CompactLayout l = compact_layout(ch, cl.y);
  unsigned char *blob = arena + e[0];
  const unsigned long long n_pairs = e[2], m_rel = m - static_cast<unsigned long long>(cl.x) * ch;
  RowsBefore at = rows_before<kP1RawShift>(loc[m], blk, blk_raw, m);
  at.pairs -= clip_base[2ull * fm.y];
  at.raw -= clip_base[2ull * fm.y + 1];
  const unsigned char *rec = records + static_cast<size_t>(fm.x) * rec_bytes;
  const bool raw = record_raw(rec) != 0;
  const unsigned room = raw ? 0u : store_row_word(rec, c);
  if (lane == 0) {
    reinterpret_cast<unsigned *>(blob + l.o_scale)[m_rel] = __float_as_uint(record_scale(rec, c));
    reinterpret_cast<unsigned *>(blob + l.o_cnt)[m_rel] = room;
    if (c == 0) blob[l.o_israw + (frame - cl.x)] = raw ? 1 : 0;
  }
  if (m_rel == 0) {  // the gaps behind the clip's fixed sections and in front of its raw section: < 64 bytes each
    const unsigned long long rows = static_cast<unsigned long long>(cl.y) * ch;
    const unsigned long long gap[4][2] = {{l.o_israw + cl.y, l.o_scale},
                                          {l.o_scale + 4 * rows, l.o_cnt},
                                          {l.o_cnt + 4 * rows, l.o_pairs},
                                          {l.o_pairs + 4 * n_pairs, compact_raw_offset(l, n_pairs)}};
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (gap[g][0] + lane < gap[g][1]) blob[gap[g][0] + lane] = 0;
  }
  const short *qrow = reinterpret_cast<const short *>(rec + hdr_bytes) + static_cast<size_t>(c) * kFrameI;
  pack_row(qrow, raw, reinterpret_cast<short4 *>(blob + compact_raw_offset(l, n_pairs) + at.raw * (kFrameI * 2ull)),
           reinterpret_cast<unsigned *>(blob + l.o_pairs) + at.pairs, room, lane);
}

// ------------------------------------------------------------------------------------------
// R1: frame records -> the row tables D1 reads (DecodeRows), without the host: what
// glc_frames_from_device_records + build_row_table + an upload give for the same records, for a decode
// queued right behind the encode that wrote them (glc_decode_device_records, glc_roundtrip_*).
// One wave per row.  Row m owns pairs [1024 m, 1024 m + 1024): a fixed stride instead of a scan over the
// rows, so nothing here waits for another workgroup (4 KiB of workspace per row, of which a tonal row
// touches a few hundred bytes).  Lane l owns the 16 bins 16 l .. 16 l + 15 of the dense row (two 16-byte
// loads); an inclusive shuffle scan of the lanes' non-zero counts gives every lane the place of its
// first pair, and since a lane's bins are contiguous and the lanes ascend, the list is in ascending k
// (src/codec.rs:303-306) with no sorting.  A record whose nnz field disagrees with its row is read as
// k_pack_rows reads it: the first min(nnz, 1024) non-zeros; where the row holds fewer, k_pack_rows pads
// its slot with entries every reader ignores (idx 0xFFFF) - here the list is simply that much shorter.
// Rows of raw frames point into the records themselves (the frame's planar i16 block is its raw_pcm,
// Q1): no copy.  stats (optional): {sum of min(nnz, 1024) over rows of compressed frames, raw frames},
// added to - one pair of atomics per workgroup, spread over kRowStatSlots counter pairs a cache line apart
// (2048 workgroups adding to ONE address took 21 us of the kernel's 30: same-address atomics queue up in L2).
// ------------------------------------------------------------------------------------------
// SEG (a round of glc_roundtrip_batch_device): row m is channel m % ch of REAL frame m / ch of a virtual stream
// of many clips, whose record is number fmap[m / ch].x among `records` and which belongs to clip fmap[m / ch].y
// (here EVERY frame names its clip, not only a clip's first); the junk frames between the clips are in no map
// and get no row.  row_raw points at the record's place in `records`.  stats is then per clip: kClipStatSlots
// counter pairs, kRowStatStride uint64_t apart, from stats + clip * kClipStatSlots * kRowStatStride on; a
// workgroup's four rows ascend through at most four clips and add once per clip they touch.
template <bool SEG>
__global__ __launch_bounds__(256) void k_rows_from_records(const unsigned char *__restrict__ records, unsigned M,
                                                            unsigned ch, unsigned long long rec_bytes,
                                                            unsigned long long hdr_bytes, unsigned *__restrict__ pairs,
                                                            unsigned long long *__restrict__ row_begin,
                                                            unsigned *__restrict__ row_cnt, float *__restrict__ row_scale,
                                                            long long *__restrict__ row_raw,
                                                            unsigned long long *__restrict__ row_raw_len,
                                                            unsigned long long *__restrict__ stats,
                                                            const uint2 *__restrict__ fmap) {
  __shared__ unsigned s_nnz[4], s_rawf[4], s_clip[4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned m = blockIdx.x * 4 + w;
  unsigned stat_nnz = 0, stat_raw = 0, stat_clip = ~0u;
  if (m < M) {
    unsigned frame = m / ch;
    const unsigned c = m - frame * ch;
    if constexpr (SEG) {
      const uint2 fm = fmap[frame];
      frame = fm.x;
      stat_clip = fm.y;
    }
    const unsigned char *rec = records + static_cast<size_t>(frame) * rec_bytes;
    const unsigned raw = record_raw(rec);
    const float scale = record_scale(rec, c);
    const unsigned room = min(record_nnz(rec, c), static_cast<unsigned>(kHopI));
    unsigned n_row = 0;
    if (raw) {
      stat_raw = c == 0 ? 1u : 0u;
    } else {
      stat_nnz = room;
      const uint4 *src = reinterpret_cast<const uint4 *>(rec + hdr_bytes + static_cast<size_t>(c) * (kFrameI * 2) + lane * 32);
      const uint4 a = src[0], b = src[1];
      const unsigned wd[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};  // bins 16 lane + 2 j (low half), + 2 j + 1 (high half)
      unsigned cnt = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) cnt += ((wd[j] & 0xFFFFu) ? 1u : 0u) + ((wd[j] >> 16) ? 1u : 0u);
      unsigned incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
      }
      n_row = min(static_cast<unsigned>(__shfl(incl, 63)), room);
      unsigned pos = incl - cnt;
      unsigned *dst = pairs + static_cast<size_t>(m) * kHopI;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned q = (j & 1) ? wd[j >> 1] >> 16 : wd[j >> 1] & 0xFFFFu;
        if (q != 0) {
          if (pos < room) dst[pos] = static_cast<unsigned>(lane * 16 + j) | (q << 16);
          ++pos;
        }
      }
    }
    if (lane == 0) {
      row_begin[m] = static_cast<unsigned long long>(m) * kHopI;
      row_cnt[m] = n_row;
      row_scale[m] = scale;
      // offset, in i16, of the frame's payload from `records` (the raw pool): header sizes are multiples of 16
      row_raw[m] = raw ? static_cast<long long>((static_cast<unsigned long long>(frame) * rec_bytes + hdr_bytes) >> 1) : -1ll;
      row_raw_len[m] = raw ? static_cast<unsigned long long>(kFrameI) * ch : 0ull;
    }
  }
  if constexpr (SEG) {
    if (lane == 0) s_nnz[w] = stat_nnz, s_rawf[w] = stat_raw, s_clip[w] = stat_clip;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned cur = s_clip[0], n = 0, r = 0;
      for (int i = 0; i <= 4; ++i) {
        if (i == 4 || s_clip[i] != cur) {  // the rows of `cur` in this workgroup end here
          if (cur != ~0u) {
            unsigned long long *slot =
                stats + (static_cast<size_t>(cur) * kClipStatSlots + blockIdx.x % kClipStatSlots) * kRowStatStride;
            if (n) atomicAdd(&slot[0], static_cast<unsigned long long>(n));
            if (r) atomicAdd(&slot[1], static_cast<unsigned long long>(r));
          }
          if (i == 4) break;
          cur = s_clip[i], n = 0, r = 0;
        }
        n += s_nnz[i], r += s_rawf[i];
      }
    }
  } else if (stats) {  // kernel argument: uniform
    if (lane == 0) s_nnz[w] = stat_nnz, s_rawf[w] = stat_raw;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned n = s_nnz[0] + s_nnz[1] + s_nnz[2] + s_nnz[3], r = s_rawf[0] + s_rawf[1] + s_rawf[2] + s_rawf[3];
      unsigned long long *slot = stats + static_cast<size_t>(blockIdx.x % kRowStatSlots) * kRowStatStride;
      if (n) atomicAdd(&slot[0], static_cast<unsigned long long>(n));
      if (r) atomicAdd(&slot[1], static_cast<unsigned long long>(r));
    }
  }
}

// ------------------------------------------------------------------------------------------
// R2: compact blobs -> the row tables D1 reads, without the host and without moving the payload (glc_kernels.h
// launch_rows_from_compact has the rules): the tables of rows [win[0], win[0] + win[1]) of each entry's blob, without
// a table entry for any row in front; a whole blob is the window {0, rows}.  The blob is almost the table already:
// cnt is row_cnt, scale is row_scale, the pairs are the rows' lists back to back - what is missing are the two
// exclusive scans (pairs and raw rows in front of a row; the shared scan above P1) and the checks build_row_table
// makes on the host, because D1 trusts its rows.  Sections are found with glc_common.h compact_sections, as the host
// finds them.
//   k_r2_headers      one thread per entry: glc_common.h compact_header_fault behind a capacity pre-check; fills
//                     the entry's CompactStatus, the two origin words with 0
//   k_r2w_prefix      (only when a window has rows in front) workgroup (x, entry) sums rows [4096 x, 4096 x + 4096)
//                     below win[0] - cnt of the rows of compressed frames, one per row of a raw frame, from the cnt
//                     and is_raw sections alone - in registers, across the wave by shuffles, across the four waves
//                     through LDS, and adds its two sums to the entry's origin words with one vector atomic each
//                     (64-bit integer adds: the result does not depend on their order)
//   k_r2_scan_rows    scan_rows_1024 over the windows' own cnt (nothing for a blob whose header failed).  The
//                     row's word waits in its row_raw_len slot for k_r2_rows.
//   k_r2_scan_blocks  scan_block_sums, then per entry the origin r2_row subtracts - the launch's running sums at
//                     the entry's first row MINUS the window's prefix (mod 2^64), so that r2_row finds the row's
//                     place in its blob - and for a header that failed the rows that rejects: the window's.  TOTALS
//                     (the launch's word, a launch of whole blobs): the entry's two sums against the totals its
//                     header promised (reported, they reject nothing)
//   k_r2_rows         one wave per row (r2_row): bounds, then the list in strides of 64 - lane l compares its bin
//                     with lane l - 1's (shuffle; lane 0 takes the previous stride's last) - and the row's arrays
// Rows of several entries follow each other (glc_decode_batch_device_compact): a row finds its entry by a binary
// search over the directory's first rows, and the scans simply run across the entries - an entry's origin is
// subtracted again.  The sums of a blob whose header failed are taken over nothing.
// An entry may own more table rows than its window has (the next entry's first_row lies further on: the fixed slots
// of glc_decode_crops_device_store, or an entry whose window is empty).  Row first_row + j with j >= win[1] is an
// empty row: the scans see the word 0, k_r2_rows writes {0, 0, 0.0f, -1, 0} and reports nothing.  WINDOW false (the
// scan-rows and rows kernels of a launch of whole blobs): win is {0, rows}, so that test and the offset are left out.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned r2_find_blob(const CompactBlob *__restrict__ dir, unsigned n_entries, unsigned m) {
  unsigned lo = 0, hi = n_entries;  // the last entry whose first_row <= m (first_row ascends from 0)
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (dir[mid].first_row <= m) lo = mid;
    else hi = mid;
  }
  return lo;
}

// verdict (null, or one word per entry: the draw planner's, k_store_plan_crops): the bits it gave an entry it emptied
// join kCompactBadHeader in the status this kernel writes wholesale.
__global__ __launch_bounds__(256) void k_r2_headers(const CompactBlob *__restrict__ dir, CompactBlob one, unsigned n_blobs,
                                                     unsigned ch, CompactStatus *__restrict__ status,
                                                     const unsigned *__restrict__ verdict) {
  const unsigned b = blockIdx.x * 256u + threadIdx.x;
  if (b >= n_blobs) return;
  const CompactBlob e = dir ? dir[b] : one;
  const unsigned long long nf = e.rows / ch;
  CompactStatus st{};
  st.first_bad_row = ~0ull;
  bool ok = e.cap >= compact_sections(nf, e.rows).o_pairs;  // the host has checked this: the fixed sections lie inside the capacity
  if (ok) {
    // a copy: one round of loads, and what is checked is what goes into the status (the blob is not trusted to stay put)
    const CompactHeader h = *reinterpret_cast<const CompactHeader *>(e.addr);
    ok = compact_header_fault(h, ch, nf, 0, /*exact=*/true, e.cap) == HeaderFault::kNone;
    if (ok) st.n_pairs = h.n_pairs, st.n_raw_rows = h.n_raw_rows, st.bytes = h.bytes;
  }
  st.header_ok = ok ? 1u : 0u;
  if (!ok) {  // every row is rejected
    st.flags = kCompactBadHeader | (verdict ? verdict[b] : 0u);
    st.n_bad_rows = e.rows;
    st.first_bad_row = 0;
  }
  status[b] = st;
}

// The word row `lm` of blob `e` (whose header passed) gives the scan: its cnt, or one row of a raw frame.
__device__ __forceinline__ unsigned long long r2_row_word(const CompactBlob e, unsigned ch, unsigned lm) {
  const CompactLayout l = compact_sections(e.rows / ch, e.rows);
  const unsigned char *blob = reinterpret_cast<const unsigned char *>(e.addr);
  return blob[l.o_israw + lm / ch] ? (1ull << kR2RawShift) : reinterpret_cast<const unsigned *>(blob + l.o_cnt)[lm];
}

template <bool WINDOW>
__global__ __launch_bounds__(256) void k_r2_scan_rows(const CompactBlob *__restrict__ dir, CompactBlob one, unsigned n_entries,
                                                       unsigned M, unsigned ch, const CompactStatus *__restrict__ status,
                                                       unsigned long long *__restrict__ loc,
                                                       unsigned long long *__restrict__ blk,
                                                       unsigned long long *__restrict__ blk_raw) {
  scan_rows_1024<unsigned long long, kR2RawShift>(
      [&](unsigned m) -> unsigned long long {
        const unsigned b = dir ? r2_find_blob(dir, n_entries, m) : 0u;
        const CompactBlob e = dir ? dir[b] : one;
        const unsigned j = m - e.first_row;  // row j of the entry's slot; behind the window: an empty row
        if ((WINDOW && j >= e.win[1]) || !status[b].header_ok) return 0ull;
        return r2_row_word(e, ch, WINDOW ? e.win[0] + j : j);
      },
      M, loc, blk, blk_raw);
}

template <bool TOTALS>
__global__ __launch_bounds__(1024) void k_r2_scan_blocks(const CompactBlob *__restrict__ dir, CompactBlob one, unsigned n_entries,
                                                          unsigned M, unsigned long long *__restrict__ blk,
                                                          unsigned long long *__restrict__ blk_raw, unsigned n,
                                                          const unsigned long long *__restrict__ loc,
                                                          CompactStatus *__restrict__ status) {
  __shared__ unsigned long long s[1024];
  unsigned long long sums[2];
  scan_block_sums(blk, blk_raw, n, s, sums);
  __syncthreads();  // this workgroup's own stores to blk / blk_raw are read below
  // per entry: the running sums at its first row and (TOTALS) behind its window's last one
  for (unsigned b = threadIdx.x; b < n_entries; b += 1024) {
    const CompactBlob e = dir ? dir[b] : one;
    const unsigned long long r0 = e.first_row, r1 = r0 + e.win[1];
    RowsBefore at0{sums[0], sums[1]}, at1 = at0;
    if (r0 < M) at0 = rows_before<kR2RawShift>(loc[r0], blk, blk_raw, r0);
    if (TOTALS && r1 < M) at1 = rows_before<kR2RawShift>(loc[r1], blk, blk_raw, r1);
    CompactStatus *st = status + b;
    st->pairs_before = at0.pairs - st->pairs_before;  // the window's prefix is there: k_r2w_prefix's sums, or k_r2_headers' 0
    st->raw_before = at0.raw - st->raw_before;
    if (!st->header_ok) {  // k_r2_headers reported the blob's rows
      st->n_bad_rows = e.win[1];
      st->first_bad_row = e.win[0];
    } else if constexpr (TOTALS) {
      unsigned f = st->flags;
      if (at1.pairs - at0.pairs != st->n_pairs) f |= kCompactPairSum;
      if (at1.raw - at0.raw != st->n_raw_rows) f |= kCompactRawSum;
      st->flags = f;
    }
  }
}

// What one wave of k_r2_rows does with row `lm` of blob `e`, table row `m` of the launch: the checks, the row's five
// table entries, and what it has to say in the status `st` of its entry.
__device__ __forceinline__ void r2_row(const CompactBlob &e, CompactStatus *st, unsigned ch, unsigned long long base_addr,
                                       unsigned lm, unsigned m, const unsigned long long *__restrict__ blk,
                                       const unsigned long long *__restrict__ blk_raw, unsigned long long *__restrict__ row_begin,
                                       unsigned *__restrict__ row_cnt, float *__restrict__ row_scale, long long *__restrict__ row_raw,
                                       unsigned long long *__restrict__ row_raw_len, int lane) {
  unsigned long long begin = 0, raw_len = 0;
  long long raw_at = -1;
  unsigned cnt = 0, bad = 0;
  float scale = 0.0f;
  if (st->header_ok) {
    const CompactLayout l = compact_sections(e.rows / ch, e.rows);
    const unsigned long long n_pairs = st->n_pairs, n_raw_rows = st->n_raw_rows;
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(e.addr);
    const unsigned c = lm % ch;
    const RowsBefore at = rows_before<kR2RawShift>(row_raw_len[m], blk, blk_raw, m);  // the scan left the row's word there
    const unsigned long long p = at.pairs - st->pairs_before, r = at.raw - st->raw_before;
    scale = reinterpret_cast<const float *>(blob + l.o_scale)[lm];
    if (blob[l.o_israw + lm / ch]) {
      // the frame's ch planes are its raw_pcm as it stands (Q1): they start at plane r - c
      const unsigned long long raw_off = compact_raw_offset(l, n_pairs), first = r - c;
      if (r >= c && first + ch <= n_raw_rows && raw_off + (first + ch) * 4096ull <= st->bytes) {
        raw_at = static_cast<long long>((e.addr - base_addr + raw_off) / 2ull + first * 2048ull);
        raw_len = 2048ull * ch;
      } else {
        bad = kCompactRawRange;
      }
    } else {
      const unsigned n = reinterpret_cast<const unsigned *>(blob + l.o_cnt)[lm];
      if (n > 1024u || p > n_pairs || n > n_pairs - p) {
        bad = kCompactRowBounds;
      } else {
        const unsigned *list = reinterpret_cast<const unsigned *>(blob + l.o_pairs) + p;
        unsigned last = 0, wrong = 0;  // `last`: the bin at the end of the stride before
        for (unsigned j0 = 0; j0 < n; j0 += 64) {
          const unsigned j = j0 + lane;
          const unsigned k = j < n ? list[j] & 0xFFFFu : 0xFFFFFFFFu;
          unsigned prev = __shfl_up(k, 1);
          if (lane == 0) prev = last;
          if (j < n && (k >= 1024u || (j > 0 && k <= prev))) wrong = 1;
          last = __shfl(k, 63);
        }
        if (__any(wrong)) {
          bad = kCompactNotCanonical;
        } else {
          begin = (e.addr - base_addr + l.o_pairs) / 4ull + p;
          cnt = n;
        }
      }
    }
  }
  if (lane == 0) {
    row_begin[m] = begin;
    row_cnt[m] = cnt;
    row_scale[m] = scale;
    row_raw[m] = raw_at;
    row_raw_len[m] = raw_len;
    if (bad) {
      atomicOr(&st->flags, bad);
      atomicAdd(reinterpret_cast<unsigned long long *>(&st->n_bad_rows), 1ull);
      atomicMin(reinterpret_cast<unsigned long long *>(&st->first_bad_row), static_cast<unsigned long long>(lm));
    }
  }
}

template <bool WINDOW>
__global__ __launch_bounds__(256) void k_r2_rows(const CompactBlob *__restrict__ dir, CompactBlob one, unsigned n_entries,
                                                  unsigned M, unsigned ch, unsigned long long base_addr,
                                                  const unsigned long long *__restrict__ blk,
                                                  const unsigned long long *__restrict__ blk_raw,
                                                  CompactStatus *__restrict__ status,
                                                  unsigned long long *__restrict__ row_begin, unsigned *__restrict__ row_cnt,
                                                  float *__restrict__ row_scale, long long *__restrict__ row_raw,
                                                  unsigned long long *__restrict__ row_raw_len) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m64 = static_cast<unsigned long long>(blockIdx.x) * 4ull + (threadIdx.x >> 6);
  if (m64 >= M) return;
  const unsigned m = static_cast<unsigned>(m64);
  const unsigned b = dir ? r2_find_blob(dir, n_entries, m) : 0u;
  const CompactBlob e = dir ? dir[b] : one;
  const unsigned j = m - e.first_row;
  if (WINDOW && j >= e.win[1]) {  // behind the window: the empty row, and nothing to report
    if (lane == 0) row_begin[m] = 0ull, row_cnt[m] = 0u, row_scale[m] = 0.0f, row_raw[m] = -1ll, row_raw_len[m] = 0ull;
    return;
  }
  r2_row(e, status + b, ch, base_addr, WINDOW ? e.win[0] + j : j, m, blk, blk_raw, row_begin, row_cnt, row_scale, row_raw, row_raw_len,
         lane);
}

constexpr unsigned kR2wPrefixRows = 4096;  // rows in front of a window that one workgroup of k_r2w_prefix sums

__global__ __launch_bounds__(256) void k_r2w_prefix(const CompactBlob *__restrict__ dir, CompactBlob one, unsigned b0, unsigned ch,
                                                     CompactStatus *__restrict__ status) {
  __shared__ unsigned long long s_pairs[4], s_raw[4];
  const unsigned b = b0 + blockIdx.y;
  const CompactBlob e = dir ? dir[b] : one;
  const unsigned long long r0 = static_cast<unsigned long long>(blockIdx.x) * kR2wPrefixRows;
  CompactStatus *st = status + b;
  if (r0 >= e.win[0] || !st->header_ok) return;  // the whole workgroup
  const CompactLayout l = compact_sections(e.rows / ch, e.rows);
  const unsigned char *is_raw = reinterpret_cast<const unsigned char *>(e.addr) + l.o_israw;
  const unsigned *cnt = reinterpret_cast<const unsigned *>(e.addr + l.o_cnt);
  const unsigned long long end = min(static_cast<unsigned long long>(e.win[0]), r0 + kR2wPrefixRows);
  unsigned long long pairs = 0, raw = 0;
  for (unsigned long long lm = r0 + threadIdx.x; lm < end; lm += 256) {  // below win[0] <= rows: inside the fixed sections
    if (is_raw[lm / ch]) raw += 1;
    else pairs += cnt[lm];
  }
  for (int off = 32; off; off >>= 1) pairs += __shfl_down(pairs, off), raw += __shfl_down(raw, off);
  if ((threadIdx.x & 63) == 0) s_pairs[threadIdx.x >> 6] = pairs, s_raw[threadIdx.x >> 6] = raw;
  __syncthreads();
  if (threadIdx.x == 0) {
    pairs = s_pairs[0] + s_pairs[1] + s_pairs[2] + s_pairs[3];
    raw = s_raw[0] + s_raw[1] + s_raw[2] + s_raw[3];
    if (pairs) atomicAdd(reinterpret_cast<unsigned long long *>(&st->pairs_before), pairs);
    if (raw) atomicAdd(reinterpret_cast<unsigned long long *>(&st->raw_before), raw);
  }
}

// ------------------------------------------------------------------------------------------
// The draw planner of glc_decode_crops_device_store (glc_kernels.h launch_store_plan_crops has the rules): what the
// host drivers of the pointer calls work out per crop - plan_encode, plan_crop, the directory entry, the hop
// descriptors, all from glc_common.h / glc_kernels.h, the same functions - for selections that are device data.
// One thread per (crop, hop slot): the kernel is a chain of three dependent loads (clip index -> length and entry)
// and some 64-bit integer arithmetic, so it is latency-bound whatever the split; with a thread per slot the
// descriptors of a crop go out as one store each from neighbouring lanes instead of max_hops stores one after the
// other from one lane, and the plan every thread of a crop repeats costs nothing that matters beside the loads
// (which the crop's threads share in cache).  Slot 0 of a crop also writes its directory entry and its verdict.
// Ordinary vector loads and stores, no atomics; nothing of the arena is dereferenced.
// Descriptors behind a crop's hops are null ({-1, -1, 0, 0, 0, 0, 0}): k_overlap_add_strided gives a span of cnt == 0
// at most one chunk whose four `keep` are all false - d2_store then stores element by element and keeps none, and
// d2_sample reads no block when both slots are absent - and k_overlap_add_planar returns at t_hi <= t_lo.  Neither
// writes anything.  An unusable crop gets descriptors with both slots absent over its whole span: +0.0.
// RAGGED (glc_decode_ragged_crops_device_store): the crop keeps v = min(wanted, len - start) samples and its descriptor
// slots are the hops of that valid part, then the padding [v * ch, length * ch) of the span a hop's worth per slot,
// both block slots absent, then null ones; slot 0 also writes v (0 for an unusable crop) where the caller asked.  A
// valid descriptor and the pad descriptor behind it meet at span position v * ch, which need not be a chunk
// boundary of the destination: DESIGN section 4, "a ragged crop's seam", has why neither writes the other's elements.
// ------------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_store_plan_crops(StoreDraw a) {
  const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * 256ull + threadIdx.x;
  if (t >= a.n_crops * a.max_hops) return;
  const unsigned long long i = t / a.max_hops;
  const unsigned s = static_cast<unsigned>(t - i * a.max_hops);
  const unsigned k = static_cast<unsigned>(i % a.per_round);  // the crop's place in its round
  const unsigned long long ch = a.ch, per_hop = static_cast<unsigned long long>(kHop) * ch;
  const long long clip = a.clips[i], start = a.starts[i];
  unsigned long long keep = a.length;  // samples per channel the crop takes from its clip
  unsigned verdict = 0;
  glc_plan plan{};
  glc_crop_plan win{};
  unsigned long long addr = a.arena, cap = 0;
  if (clip < 0 || static_cast<unsigned long long>(clip) >= a.n_entries) {
    verdict = kCompactBadCrop;  // and the entry is not read
  } else {
    const long long len = a.lengths[clip];
    // len <= max_length bounds len * ch (the host checked max_length), start <= len - length bounds start * ch
    if (len < 0 || static_cast<unsigned long long>(len) > a.max_length || start < 0) {
      verdict = kCompactBadCrop;
    } else if (RAGGED) {
      const long long want = a.want ? a.want[i] : static_cast<long long>(a.length);
      if (start >= len || want < 1 || static_cast<unsigned long long>(want) > a.length) {
        verdict = kCompactBadCrop;
      } else {  // start < len bounds start * ch, keep <= length bounds keep * ch (the host checked length)
        const unsigned long long left = static_cast<unsigned long long>(len - start);
        keep = static_cast<unsigned long long>(want) < left ? static_cast<unsigned long long>(want) : left;
      }
    }
    if (!verdict) {
      const unsigned long long n_samples = static_cast<unsigned long long>(len) * ch;
      plan = plan_encode(n_samples, static_cast<uint16_t>(a.ch));
      if (plan.n_frames == 0 ||
          !plan_crop(n_samples, static_cast<uint16_t>(a.ch), glc_crop{static_cast<unsigned long long>(start), keep}, &win))
        verdict = kCompactBadCrop;
    }
    if (!verdict) {
      const glc_store_entry e = a.entries[clip];
      // each term is bounded before the difference is formed: nothing wraps (compact_header_fault's way)
      if (e.stored == 0 || (e.offset & 63ull) || e.offset > a.arena_bytes || e.bytes > a.arena_bytes - e.offset)
        verdict = kCompactNoBlob;
      else
        addr = a.arena + e.offset, cap = e.bytes;
    }
  }
  const unsigned slot0 = k * a.max_frames;  // the crop's first block slot; its first table row is slot0 * ch
  if (s == 0) {
    a.dir[i] = verdict ? CompactBlob{a.arena, 0ull, slot0 * a.ch, 0u, {0u, 0u}}
                       : CompactBlob{addr, cap, slot0 * a.ch, static_cast<unsigned>(plan.n_frames * ch),
                                     {static_cast<unsigned>(win.first_frame * ch), static_cast<unsigned>(win.n_frames * ch)}};
    a.verdict[i] = verdict;
    if (RAGGED && a.valid) a.valid[i] = verdict ? 0ll : static_cast<long long>(keep);
  }
  const unsigned long long dst = i * a.clip_stride, span = a.length * ch;
  HopDescStrided d{-1, -1, 0u, 0u, 0ull, 0ull, 0ull};
  // silence a hop's worth per slot: over the whole span of an unusable crop, behind the valid part of a ragged one
  auto silence = [&](unsigned long long j0) {
    if (j0 >= span) return;
    const unsigned long long cnt = span - j0 < per_hop ? span - j0 : per_hop;
    d = HopDescStrided{-1, -1, 0u, static_cast<unsigned>(cnt), a.planes ? dst : dst + j0, a.planes ? a.channel_stride : 0ull, j0};
  };
  if (verdict) {
    silence(s * per_hop);
  } else if (s < win.n_hops) {
    const Trim whole = gapless_trim(plan.n_frames, a.ch, plan.encoder_delay, plan.per_channel * ch);
    const Trim trim{whole.start + static_cast<unsigned long long>(start) * ch, keep * ch};  // what the crop keeps of its un-trimmed stream
    hop_desc(&d, plan.n_frames, a.ch, trim, win.first_hop + s, static_cast<long long>(slot0) - static_cast<long long>(win.first_frame),
             dst, a.planes != 0, a.channel_stride);
  } else if (RAGGED) {
    silence(keep * ch + (s - win.n_hops) * per_hop);
  }
  a.desc[t] = d;
}

// ------------------------------------------------------------------------------------------
// The segment planner of glc_stream_dec_push_device (glc_kernels.h launch_stream_dec_plan has the rules): one thread
// per segment, one 32-byte entry in, one 32-byte directory entry and one verdict word out - k_store_plan_crops' rules
// for an entry, without a selection.  Latency-bound (one load per thread); ordinary vector loads and stores.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stream_dec_plan(unsigned long long arena, unsigned long long arena_bytes,
                                                          const glc_store_entry *__restrict__ entries,
                                                          const StreamDecSeg *__restrict__ segs, unsigned n_segs,
                                                          CompactBlob *__restrict__ dir, unsigned *__restrict__ verdict) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n_segs) return;
  const glc_store_entry e = entries[j];
  const StreamDecSeg sg = segs[j];
  // each term is bounded before the difference is formed: nothing wraps (k_store_plan_crops' way)
  const bool usable = e.stored != 0 && (e.offset & 63ull) == 0 && e.offset <= arena_bytes && e.bytes <= arena_bytes - e.offset;
  dir[j] = usable ? CompactBlob{arena + e.offset, e.bytes, sg.first_row, sg.rows, {0u, sg.rows}}
                  : CompactBlob{arena, 0ull, sg.first_row, 0u, {0u, 0u}};
  verdict[j] = usable ? 0u : kCompactNoBlob;
}

// ------------------------------------------------------------------------------------------
// The carry of a streaming decode (glc_kernels.h launch_stream_dec_carry has the two roles).  Workgroup (u, lane): unit
// u = half * ch + c is the 1024 floats of channel c of carry part `half` (0: the hop's sums, 1: the block's second
// half), one float4 per thread; the lane's descriptor is one block-uniform load.  The save role forms the sums with
// d2_sum on the operands and in the order D2 uses, so a carried sum has the bits D2 would have written.
// ------------------------------------------------------------------------------------------
template <bool SAVE>
__global__ __launch_bounds__(256) void k_stream_dec_carry(const StreamCarry *__restrict__ desc, unsigned ch,
                                                           float *__restrict__ blocks, float *__restrict__ carry) {
  const StreamCarry d = desc[blockIdx.y];
  const unsigned half = blockIdx.x / ch, c = blockIdx.x - half * ch;
  const unsigned i = threadIdx.x * 4u;
  float *held = carry + d.carry + (static_cast<size_t>(half) * ch + c) * kHopI + i;
  if constexpr (!SAVE) {
    float *dst = blocks + ((static_cast<size_t>(d.prev) + half) * ch + c) * kFrameI + kHopI + i;
    *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(held);
  } else {
    const float *cur = blocks + (static_cast<size_t>(d.cur) * ch + c) * kFrameI + i;
    float4 out;
    if (half) {
      out = *reinterpret_cast<const float4 *>(cur + kHopI);
    } else {
      const bool has_prev = d.prev >= 0;
      const float4 q = *reinterpret_cast<const float4 *>(cur);
      float4 p = float4{0.0f, 0.0f, 0.0f, 0.0f};
      if (has_prev) p = *reinterpret_cast<const float4 *>(blocks + (static_cast<size_t>(d.prev) * ch + c) * kFrameI + kHopI + i);
      const float pv[4] = {p.x, p.y, p.z, p.w}, cv[4] = {q.x, q.y, q.z, q.w};
      out = float4{d2_sum(pv, cv, has_prev, true, 0), d2_sum(pv, cv, has_prev, true, 1), d2_sum(pv, cv, has_prev, true, 2),
                   d2_sum(pv, cv, has_prev, true, 3)};
    }
    *reinterpret_cast<float4 *>(held) = out;
  }
}

// ------------------------------------------------------------------------------------------
// Eviction: glc_store_compact_device (glc_kernels.h StoreEvict has the plan, include/glc.h the rules).
// E1 is k_store_place's shape: one workgroup, chunks of 1024 entries, three Hillis-Steele scans per chunk (the
// maximum of the candidates' ends, the kept bytes, the kept count) with their carries in registers.  Every thread
// loads its entry, keep byte and length at the top of a chunk and stores behind the scans' barriers, and the number
// of a kept entry is at most its index: an output word is never written before the input word at the same place
// has been read, which is what lets the output arrays be the input arrays.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_store_evict_scan(StoreEvict a) {
  __shared__ unsigned long long s_max[1024], s_sum[1024];
  __shared__ unsigned s_cnt[1024];
  __shared__ unsigned long long s_limit, s_first;
  const unsigned t = threadIdx.x;
  if (t == 0) s_limit = 0ull, s_first = ~0ull;
  const unsigned long long n = a.n_entries;
  const unsigned long long *in = reinterpret_cast<const unsigned long long *>(a.entries);
  unsigned long long *out = reinterpret_cast<unsigned long long *>(a.entries_out);
  uint64_t *new_off = a.ws + 8, *src_off = a.ws + 8 + n + 1;
  unsigned long long carry_max = 0, carry_sum = 0, carry_cnt = 0;
  for (unsigned long long k0 = 0; k0 < n; k0 += 1024) {
    const unsigned long long i = k0 + t;
    unsigned long long offset = 0, bytes = 0, n_pairs = 0, word3 = 0;
    long long len = 0;
    bool keep = false;
    if (i < n) {
      offset = in[4 * i], bytes = in[4 * i + 1], n_pairs = in[4 * i + 2], word3 = in[4 * i + 3];
      keep = a.keep[i] != 0;
      if (a.lengths) len = a.lengths[i];
    }
    // each term is bounded before the difference is formed: nothing wraps (k_store_plan_crops' way)
    const bool usable = i < n && (word3 >> 32) != 0 && (offset & 63ull) == 0 && (bytes & 63ull) == 0 && bytes != 0 &&
                        offset <= a.arena_bytes && bytes <= a.arena_bytes - offset;
    const bool cand = keep && usable;
    s_max[t] = cand ? offset + bytes : 0ull;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const unsigned long long v = t >= static_cast<unsigned>(off) ? s_max[t - off] : 0ull;
      __syncthreads();
      if (v > s_max[t]) s_max[t] = v;
      __syncthreads();
    }
    const unsigned long long before = t ? s_max[t - 1] : 0ull;
    const unsigned long long ends_before = before > carry_max ? before : carry_max;  // E_i
    if (s_max[1023] > carry_max) carry_max = s_max[1023];
    const bool kept = cand && offset >= ends_before;
    s_sum[t] = kept ? bytes : 0ull;
    s_cnt[t] = kept ? 1u : 0u;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const unsigned long long v = t >= static_cast<unsigned>(off) ? s_sum[t - off] : 0ull;
      const unsigned c = t >= static_cast<unsigned>(off) ? s_cnt[t - off] : 0u;
      __syncthreads();
      s_sum[t] += v;
      s_cnt[t] += c;
      __syncthreads();
    }
    const unsigned long long place = carry_sum + s_sum[t] - (kept ? bytes : 0ull);  // exclusive: the kept sources are disjoint
    const unsigned long long k = carry_cnt + s_cnt[t] - (kept ? 1u : 0u);           // inside the arena, the sum cannot wrap
    carry_sum += s_sum[1023];
    carry_cnt += s_cnt[1023];
    if (i < n) a.new_index[i] = kept ? static_cast<long long>(k) : !keep ? kStoreDropped : !usable ? kStoreUnusable : kStoreOutOfOrder;
    if (kept) {
      const bool stored = place <= a.dst_bytes && bytes <= a.dst_bytes - place;  // the encoder's rule (k_store_place)
      out[4 * k] = place;
      out[4 * k + 1] = bytes;
      out[4 * k + 2] = n_pairs;
      out[4 * k + 3] = (word3 & 0xFFFFFFFFull) | (stored ? 1ull << 32 : 0ull);
      if (a.lengths_out) a.lengths_out[k] = len;
      new_off[k] = place;
      src_off[k] = offset;
      if (stored) atomicMax(&s_limit, place + bytes);
      if (offset != place) atomicMin(&s_first, place);
    }
    __syncthreads();  // the scan arrays are rewritten by the next chunk
  }
  if (t == 0) {
    new_off[carry_cnt] = carry_sum;
    a.ws[0] = carry_cnt;
    a.ws[1] = carry_sum;
    a.ws[2] = s_limit;
    a.ws[3] = s_first < carry_sum ? s_first : carry_sum;
    a.ws[4] = n + 1;  // words from new_off to src_off
    *a.n_out = carry_cnt;
    *a.cursor = carry_sum;
  }
}

// E2: behind E1 on the stream, so behind every read of the input arrays.
__global__ __launch_bounds__(256) void k_store_evict_tail(StoreEvict a) {
  const unsigned long long n_out = a.ws[0];
  unsigned long long *out = reinterpret_cast<unsigned long long *>(a.entries_out);
  const unsigned long long step = static_cast<unsigned long long>(gridDim.x) * 256ull;
  for (unsigned long long k = n_out + static_cast<unsigned long long>(blockIdx.x) * 256ull + threadIdx.x; k < a.n_entries; k += step) {
    out[4 * k] = out[4 * k + 1] = out[4 * k + 2] = out[4 * k + 3] = 0ull;
    if (a.lengths_out) a.lengths_out[k] = 0;
  }
}

// Packed bytes [lo, hi) - multiples of 64, hi - lo <= kStoreMoveTile, hi <= new_off[n_out] - from their sources to
// dst[p - origin].  The tile's first and last kept entry are found once (the same search in every lane: uniform),
// each 16-byte unit then searches between the two: no step for a blob that covers the tile, 8 for 64-byte blobs.
// A unit lies inside one blob (every offset and size is a multiple of 64), so no load leaves the blob: the arena.
__device__ __forceinline__ void store_evict_gather_tile(const unsigned long long *__restrict__ new_off,
                                                        const unsigned long long *__restrict__ src_off, unsigned long long n_out,
                                                        const unsigned char *arena, unsigned char *dst, unsigned long long origin,
                                                        unsigned long long lo, unsigned long long hi) {
  auto last_at_or_below = [&](unsigned long long p, unsigned long long a, unsigned long long b) {  // new_off[a] <= p, a <= b
    while (a < b) {
      const unsigned long long mid = a + (b - a + 1) / 2;
      if (new_off[mid] <= p) a = mid; else b = mid - 1;
    }
    return a;
  };
  const unsigned long long k_lo = last_at_or_below(lo, 0, n_out - 1), k_hi = last_at_or_below(hi - 16, k_lo, n_out - 1);
  // four units per thread, all loads in front of all stores.  Named scalars, not arrays: an array here is promoted to
  // LDS, and the index of that promotion reads the dispatch packet in every wave - measured: an empty round launch
  // took 16 us with the arrays and takes 2.5 us without them
  auto unit = [&](unsigned long long p) {
    uint4 v{};
    if (p < hi) {
      const unsigned long long k = last_at_or_below(p, k_lo, k_hi);
      v = *reinterpret_cast<const uint4 *>(arena + src_off[k] + (p - new_off[k]));
    }
    return v;
  };
  const unsigned long long p0 = lo + threadIdx.x * 16ull, p1 = p0 + 4096ull, p2 = p0 + 8192ull, p3 = p0 + 12288ull;
  const uint4 v0 = unit(p0), v1 = unit(p1), v2 = unit(p2), v3 = unit(p3);
  if (p0 < hi) *reinterpret_cast<uint4 *>(dst + (p0 - origin)) = v0;
  if (p1 < hi) *reinterpret_cast<uint4 *>(dst + (p1 - origin)) = v1;
  if (p2 < hi) *reinterpret_cast<uint4 *>(dst + (p2 - origin)) = v2;
  if (p3 < hi) *reinterpret_cast<uint4 *>(dst + (p3 - origin)) = v3;
}

__global__ __launch_bounds__(256) void k_store_evict_gather(const unsigned long long *__restrict__ ws, const unsigned char *arena,
                                                            unsigned char *dst) {
  const unsigned long long n_out = ws[0], limit = ws[2];
  const unsigned long long *new_off = ws + 8, *src_off = new_off + ws[4];
  for (unsigned long long lo = static_cast<unsigned long long>(blockIdx.x) * kStoreMoveTile; lo < limit;
       lo += static_cast<unsigned long long>(gridDim.x) * kStoreMoveTile) {
    const unsigned long long hi = lo + kStoreMoveTile < limit ? lo + kStoreMoveTile : limit;
    store_evict_gather_tile(new_off, src_off, n_out, arena, dst, 0ull, lo, hi);
  }
}

// One launch of the in-place rounds (glc_kernels.h launch_store_evict_round): job j < tiles is tile j of the write-back
// of round r - 1, job tiles + j tile j of the gather of round r.  A round at or behind the total returns at once.
__global__ __launch_bounds__(256) void k_store_evict_round(const unsigned long long *__restrict__ ws, unsigned char *arena,
                                                           unsigned char *stage, unsigned long long round, unsigned long long r,
                                                           unsigned tiles) {
  const unsigned long long n_out = ws[0], total = ws[1], first = ws[3];
  const unsigned long long *new_off = ws + 8, *src_off = new_off + ws[4];
  for (unsigned j = blockIdx.x; j < 2u * tiles; j += gridDim.x) {
    const bool back = j < tiles;
    if (back && r == 0) continue;
    const unsigned long long rr = back ? r - 1 : r, base = rr * round;
    if (base >= total) continue;
    const unsigned long long at = static_cast<unsigned long long>(back ? j : j - tiles) * kStoreMoveTile;
    const unsigned long long in_round = at + kStoreMoveTile < round ? at + kStoreMoveTile : round;
    unsigned long long lo = base + at, hi = base + in_round;
    if (lo < first) lo = first;
    if (hi > total) hi = total;
    if (lo >= hi) continue;
    unsigned char *buf = stage + (rr & 1ull) * round;
    if (back) {
      for (unsigned long long p = lo + threadIdx.x * 16ull; p < hi; p += 256ull * 16ull)
        *reinterpret_cast<uint4 *>(arena + p) = *reinterpret_cast<const uint4 *>(buf + (p - base));
    } else {
      store_evict_gather_tile(new_off, src_off, n_out, arena, buf, base, lo, hi);
    }
  }
}

// ------------------------------------------------------------------------------------------
// The segment join: glc_store_join_segments_device (glc_kernels.h StoreJoin has the plan, include/glc.h the rules).
// ------------------------------------------------------------------------------------------
struct StoreJoinWs {  // the workspace's arrays (glc_kernels.h)
  unsigned long long *head, *found, *ex_pairs, *ex_raw, *ex_bad, *clip_off, *clip_sum;
};
__device__ __forceinline__ StoreJoinWs store_join_ws(const StoreJoin &a) {
  StoreJoinWs w;
  w.head = reinterpret_cast<unsigned long long *>(a.ws);
  w.found = w.head + 8;
  w.ex_pairs = w.found + 4ull * a.n_segs;
  w.ex_raw = w.ex_pairs + a.n_segs + 1;
  w.ex_bad = w.ex_raw + a.n_segs + 1;
  w.clip_off = w.ex_bad + a.n_segs + 1;
  w.clip_sum = w.clip_off + a.n_clips + 1;
  return w;
}

// J1.  Thread 0 judges the entry and the header; nothing of a segment with an unusable entry is read, and nothing
// behind a failing header.  The two reductions run over whole 16-byte units of the sections, which end on multiples of
// 64 inside the blob (the header rule: `bytes` is exactly the sections and fits the entry), and mask what lies behind
// the rows: the padding is as untrusted as the rest.
__global__ __launch_bounds__(256) void k_store_join_plan(StoreJoin a) {
  __shared__ CompactHeader s_h;
  __shared__ unsigned s_bits;
  __shared__ unsigned long long s_part[2][4];
  const StoreJoinWs w = store_join_ws(a);
  const unsigned t = threadIdx.x;
  for (unsigned long long j = blockIdx.x; j < a.n_segs; j += gridDim.x) {
    const glc_store_entry e = a.entries[j];
    const StoreJoinSeg sg = a.segs[j];
    if (t == 0) {
      unsigned bits = 0;
      // each term is bounded before the difference is formed: nothing wraps (k_store_plan_crops' way)
      if (e.stored == 0 || (e.offset & 63ull) || e.offset > a.arena_bytes || e.bytes > a.arena_bytes - e.offset) {
        bits = kCompactNoBlob | kCompactBadHeader;
      } else if (e.bytes < sizeof(CompactHeader)) {
        bits = kCompactBadHeader;  // not even a header
      } else {
        const uint4 *hp = reinterpret_cast<const uint4 *>(a.arena + e.offset);
        uint4 *hs = reinterpret_cast<uint4 *>(&s_h);
        hs[0] = hp[0], hs[1] = hp[1], hs[2] = hp[2], hs[3] = hp[3];
        if (compact_header_fault(s_h, a.ch, sg.n_frames, 0, true, e.bytes) != HeaderFault::kNone) bits = kCompactBadHeader;
      }
      s_bits = bits;
    }
    __syncthreads();
    unsigned long long pairs = 0, raws = 0;
    if (s_bits == 0) {
      const unsigned long long F = sg.n_frames, M = F * a.ch;
      const CompactLayout l = compact_layout(a.ch, F);
      const unsigned char *blob = a.arena + e.offset;
      for (unsigned long long u = t; u * 4ull < M; u += 256ull) {
        const uint4 v = *reinterpret_cast<const uint4 *>(blob + l.o_cnt + 16ull * u);
        const unsigned long long m = 4ull * u;
        pairs += v.x;
        if (m + 1 < M) pairs += v.y;
        if (m + 2 < M) pairs += v.z;
        if (m + 3 < M) pairs += v.w;
      }
      for (unsigned long long u = t; u * 16ull < F; u += 256ull) {
        const uint4 v = *reinterpret_cast<const uint4 *>(blob + l.o_israw + 16ull * u);
        const unsigned words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (16ull * u + i < F && ((words[i >> 2] >> (8 * (i & 3))) & 0xFFu)) ++raws;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      pairs += __shfl_down(pairs, off, 64);
      raws += __shfl_down(raws, off, 64);
    }
    if ((t & 63u) == 0) s_part[0][t >> 6] = pairs, s_part[1][t >> 6] = raws;
    __syncthreads();
    if (t == 0) {
      unsigned bits = s_bits;
      const unsigned long long n_pairs = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
      const unsigned long long n_raw = (s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3]) * a.ch;
      if (bits == 0) {
        if (n_pairs != s_h.n_pairs) bits |= kCompactPairSum;
        if (n_raw != s_h.n_raw_rows) bits |= kCompactRawSum;
      }
      a.seg_status[j] = bits;
      w.found[4 * j] = e.offset;
      w.found[4 * j + 1] = bits ? 0ull : n_pairs;
      w.found[4 * j + 2] = bits ? 0ull : n_raw;
      w.found[4 * j + 3] = bits ? 1ull : 0ull;
    }
    __syncthreads();  // s_h, s_bits and s_part are rewritten by the next segment
  }
}

// J2.  The three scans over the segments first, their exclusive values in the workspace (the sums may wrap: only
// differences inside one clip are used, and those are bounded by the clip's rows); then the clips, k_store_place's
// placement rule word for word, a refused clip counting 0.
__global__ __launch_bounds__(1024) void k_store_join_scan(StoreJoin a) {
  __shared__ unsigned long long s[1024];
  __shared__ unsigned long long s_limit;
  const StoreJoinWs w = store_join_ws(a);
  const unsigned t = threadIdx.x;
  if (t == 0) s_limit = 0ull;
#pragma unroll 1
  for (int which = 0; which < 3; ++which) {
    unsigned long long *ex = which == 0 ? w.ex_pairs : which == 1 ? w.ex_raw : w.ex_bad;
    unsigned long long carry = 0;
    for (unsigned long long j0 = 0; j0 < a.n_segs; j0 += 1024) {
      const unsigned long long j = j0 + t;
      const unsigned long long mine = j < a.n_segs ? w.found[4 * j + 1 + which] : 0ull;
      scan_sum_1024(s, mine);
      if (j < a.n_segs) ex[j] = carry + s[t] - mine;
      const unsigned long long chunk_total = s[1023];
      __syncthreads();
      carry += chunk_total;
    }
    if (t == 0) ex[a.n_segs] = carry;
  }
  __threadfence_block();
  __syncthreads();  // the exclusive values are read below by other threads than wrote them
  const unsigned long long base = align64(*a.cursor);  // every thread reads it here; thread 0 writes it behind the last barrier
  unsigned long long carry = base;
  unsigned long long *out = reinterpret_cast<unsigned long long *>(a.entries_out);
  for (unsigned long long c0 = 0; c0 < a.n_clips; c0 += 1024) {
    const unsigned long long c = c0 + t;
    unsigned long long bytes = 0, n_pairs = 0, n_raw = 0, F = 0;
    long long len = 0;
    bool ok = false;
    if (c < a.n_clips) {
      const StoreJoinClip cl = a.clips[c];
      const unsigned long long j0 = cl.seg_first, j1 = cl.seg_first + cl.n_segs;
      F = cl.n_frames, len = cl.length;
      ok = w.ex_bad[j1] == w.ex_bad[j0];
      if (ok) {
        n_pairs = w.ex_pairs[j1] - w.ex_pairs[j0];
        n_raw = w.ex_raw[j1] - w.ex_raw[j0];
        bytes = compact_raw_offset(compact_layout(a.ch, F), n_pairs) + n_raw * (kFrameI * 2ull);
      }
    }
    scan_sum_1024(s, bytes);
    const unsigned long long offset = carry + s[t] - bytes;  // exclusive: every size is a multiple of 64
    const unsigned long long chunk_total = s[1023];
    __syncthreads();
    carry += chunk_total;
    if (c < a.n_clips) {
      const bool stored = ok && offset <= a.dst_bytes && bytes <= a.dst_bytes - offset;  // the encoder's rule (k_store_place)
      out[4 * c] = ok ? offset : 0ull;
      out[4 * c + 1] = bytes;
      out[4 * c + 2] = n_pairs;
      out[4 * c + 3] = n_raw | (stored ? 1ull << 32 : 0ull);
      if (a.lengths_out) a.lengths_out[c] = ok ? len : 0;
      w.clip_off[c] = offset - base;
      w.clip_sum[2 * c] = n_pairs;
      w.clip_sum[2 * c + 1] = n_raw;
      if (stored) {
        *reinterpret_cast<CompactHeader *>(a.dst + offset) = compact_header(a.ch, F, n_pairs, n_raw, bytes);
        atomicMax(&s_limit, offset + bytes - base);
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    w.clip_off[a.n_clips] = carry - base;
    w.head[0] = base;
    w.head[1] = carry - base;
    w.head[2] = s_limit;
    *a.cursor = carry;
  }
}

// M.  Where a byte of the packed destination space comes from.  A clip's blob is its header (J2 wrote it) and five
// runs - is_raw, scale, cnt, pairs, raw -, each the segments' runs back to back, each followed by zeros up to the next
// multiple of 64.  Segment j of a clip starts in a run at key(j): its first frame (is_raw), its first row's dword
// (scale, cnt), the pairs / raw rows of the clip's segments in front of it (pairs, raw).  Empty runs share a start:
// the search takes the LAST segment that starts at or below the byte, which is the one that holds it.
enum : unsigned { kJoinHeader = 0, kJoinIsRaw, kJoinScale, kJoinCnt, kJoinPairs, kJoinRaw };
struct JoinRun {  // one run of one clip
  unsigned long long clip, sec, at, len;  // at: the run's packed offset; len: its bytes without the padding
  unsigned long long j0, j1;              // the clip's segments
};
__device__ __forceinline__ unsigned long long join_key(const StoreJoin &a, const StoreJoinWs &w, const JoinRun &r, unsigned long long j) {
  if (j >= r.j1) return r.len;
  switch (r.sec) {
    case kJoinIsRaw: return a.segs[j].first_frame;
    case kJoinScale:
    case kJoinCnt: return a.segs[j].first_frame * a.ch * 4ull;
    case kJoinPairs: return (w.ex_pairs[j] - w.ex_pairs[r.j0]) * 4ull;
    default: return (w.ex_raw[j] - w.ex_raw[r.j0]) * (kFrameI * 2ull);
  }
}
// where segment j's part of the run lies in the arena
__device__ __forceinline__ unsigned long long join_source(const StoreJoin &a, const StoreJoinWs &w, const JoinRun &r, unsigned long long j) {
  const CompactLayout l = compact_layout(a.ch, a.segs[j].n_frames);
  const unsigned long long at = r.sec == kJoinIsRaw  ? l.o_israw
                                : r.sec == kJoinScale ? l.o_scale
                                : r.sec == kJoinCnt   ? l.o_cnt
                                : r.sec == kJoinPairs ? l.o_pairs
                                                      : compact_raw_offset(l, w.found[4 * j + 1]);
  return w.found[4 * j] + at;
}
// the run that holds packed byte p, the clip sought in [c_lo, c_hi]
__device__ __forceinline__ JoinRun join_run(const StoreJoin &a, const StoreJoinWs &w, unsigned long long p, unsigned long long c_lo,
                                            unsigned long long c_hi) {
  while (c_lo < c_hi) {
    const unsigned long long mid = c_lo + (c_hi - c_lo + 1) / 2;
    if (w.clip_off[mid] <= p) c_lo = mid; else c_hi = mid - 1;
  }
  const StoreJoinClip cl = a.clips[c_lo];
  const unsigned long long base = w.clip_off[c_lo], rel = p - base, n_pairs = w.clip_sum[2 * c_lo], n_raw = w.clip_sum[2 * c_lo + 1];
  const unsigned long long M = cl.n_frames * a.ch;
  const CompactLayout l = compact_layout(a.ch, cl.n_frames);
  const unsigned long long o_raw = compact_raw_offset(l, n_pairs);
  JoinRun r;
  r.clip = c_lo, r.j0 = cl.seg_first, r.j1 = cl.seg_first + cl.n_segs;
  if (rel < l.o_israw) r.sec = kJoinHeader, r.at = base, r.len = l.o_israw;
  else if (rel < l.o_scale) r.sec = kJoinIsRaw, r.at = base + l.o_israw, r.len = cl.n_frames;
  else if (rel < l.o_cnt) r.sec = kJoinScale, r.at = base + l.o_scale, r.len = 4ull * M;
  else if (rel < l.o_pairs) r.sec = kJoinCnt, r.at = base + l.o_cnt, r.len = 4ull * M;
  else if (rel < o_raw) r.sec = kJoinPairs, r.at = base + l.o_pairs, r.len = 4ull * n_pairs;
  else r.sec = kJoinRaw, r.at = base + o_raw, r.len = n_raw * (kFrameI * 2ull);
  return r;
}
// the segment of run r that holds byte u of the run (u < r.len), sought in [j_lo, j_hi]
__device__ __forceinline__ unsigned long long join_segment(const StoreJoin &a, const StoreJoinWs &w, const JoinRun &r, unsigned long long u,
                                                           unsigned long long j_lo, unsigned long long j_hi) {
  while (j_lo < j_hi) {
    const unsigned long long mid = j_lo + (j_hi - j_lo + 1) / 2;
    if (join_key(a, w, r, mid) <= u) j_lo = mid; else j_hi = mid - 1;
  }
  return j_lo;
}

// The 16 bytes at arena address `at` (any alignment) from the one or two aligned units that hold them: a dword select
// and a byte funnel, no byte loads.  Both units hold a byte of the run, so both lie inside the segment's blob, whose
// offset and size are multiples of 64.
__device__ __forceinline__ uint4 join_load16(const unsigned char *arena, unsigned long long at) {
  const unsigned sh = static_cast<unsigned>(at & 15ull);
  const unsigned char *p = arena + (at - sh);
  const uint4 lo = *reinterpret_cast<const uint4 *>(p);
  if (sh == 0) return lo;
  const uint4 hi = *reinterpret_cast<const uint4 *>(p + 16);
  const unsigned k = sh >> 2, b = (sh & 3u) * 8u;
  const unsigned w0 = k == 0 ? lo.x : k == 1 ? lo.y : k == 2 ? lo.z : lo.w;
  const unsigned w1 = k == 0 ? lo.y : k == 1 ? lo.z : k == 2 ? lo.w : hi.x;
  const unsigned w2 = k == 0 ? lo.z : k == 1 ? lo.w : k == 2 ? hi.x : hi.y;
  const unsigned w3 = k == 0 ? lo.w : k == 1 ? hi.x : k == 2 ? hi.y : hi.z;
  const unsigned w4 = k == 0 ? hi.x : k == 1 ? hi.y : k == 2 ? hi.z : hi.w;
  auto funnel = [b](unsigned l, unsigned h) { return static_cast<unsigned>(((static_cast<unsigned long long>(h) << 32) | l) >> b); };
  return uint4{funnel(w0, w1), funnel(w1, w2), funnel(w2, w3), funnel(w3, w4)};
}

// The slow path of a boundary unit: `n` elements of `width` bytes (1: is_raw, 4: the dword runs) from byte u of the
// run on, each from the segment that holds it, zero behind the run's end.  The segment only moves forward.
__device__ __forceinline__ unsigned join_gather4(const StoreJoin &a, const StoreJoinWs &w, const JoinRun &r, unsigned long long u,
                                                 unsigned long long &j) {
  unsigned word = 0;
  const unsigned width = r.sec == kJoinIsRaw ? 1u : 4u;
  for (unsigned i = 0; i < 4u; i += width) {
    const unsigned long long v = u + i;
    if (v >= r.len) break;
    j = join_segment(a, w, r, v, j, r.j1 - 1);
    const unsigned long long at = join_source(a, w, r, j) + (v - join_key(a, w, r, j));
    if (width == 4u) word = *reinterpret_cast<const unsigned *>(a.arena + at);
    else word |= static_cast<unsigned>(a.arena[at]) << (8u * i);
  }
  return word;
}

// Packed bytes [lo, hi) - multiples of 16, hi - lo <= kStoreMoveTile, hi <= limit - to dst + base.  The runs of the
// tile's first and last unit are found once (the same search in every lane: uniform); where they are one run, a unit
// that lies in it searches its segment between theirs.  Four units per thread, all loads in front of all stores, named
// scalars (the comment at store_evict_gather_tile).
__device__ __forceinline__ void store_join_move_tile(const StoreJoin &a, const StoreJoinWs &w, unsigned long long base,
                                                     unsigned long long lo, unsigned long long hi) {
  const JoinRun r_lo = join_run(a, w, lo, 0, a.n_clips - 1), r_hi = join_run(a, w, hi - 16, r_lo.clip, a.n_clips - 1);
  const bool one_run = r_lo.clip == r_hi.clip && r_lo.sec == r_hi.sec && r_lo.sec != kJoinHeader && lo - r_lo.at < r_lo.len;
  unsigned long long t_lo = 0, t_hi = 0;
  if (one_run) {
    const unsigned long long last = hi - 16 - r_lo.at < r_lo.len ? hi - 16 - r_lo.at : r_lo.len - 1;
    t_lo = join_segment(a, w, r_lo, lo - r_lo.at, r_lo.j0, r_lo.j1 - 1);
    t_hi = join_segment(a, w, r_lo, last, t_lo, r_lo.j1 - 1);
  }
  auto unit = [&](unsigned long long p, bool &live) {
    uint4 v{};
    live = false;
    if (p >= hi) return v;
    const JoinRun r = join_run(a, w, p, r_lo.clip, r_hi.clip);
    if (r.sec == kJoinHeader) return v;  // J2 wrote it
    live = true;
    const unsigned long long u = p - r.at;
    if (u >= r.len) return v;  // the zeros behind a run
    const bool narrow = one_run && r.clip == r_lo.clip && r.sec == r_lo.sec;
    unsigned long long j = join_segment(a, w, r, u, narrow ? t_lo : r.j0, narrow ? t_hi : r.j1 - 1);
    if (u + 16 <= join_key(a, w, r, j + 1)) return join_load16(a.arena, join_source(a, w, r, j) + (u - join_key(a, w, r, j)));
    v.x = join_gather4(a, w, r, u, j);
    v.y = join_gather4(a, w, r, u + 4, j);
    v.z = join_gather4(a, w, r, u + 8, j);
    v.w = join_gather4(a, w, r, u + 12, j);
    return v;
  };
  const unsigned long long p0 = lo + threadIdx.x * 16ull, p1 = p0 + 4096ull, p2 = p0 + 8192ull, p3 = p0 + 12288ull;
  bool s0, s1, s2, s3;
  const uint4 v0 = unit(p0, s0), v1 = unit(p1, s1), v2 = unit(p2, s2), v3 = unit(p3, s3);
  unsigned char *dst = a.dst + base;
  if (s0) *reinterpret_cast<uint4 *>(dst + p0) = v0;
  if (s1) *reinterpret_cast<uint4 *>(dst + p1) = v1;
  if (s2) *reinterpret_cast<uint4 *>(dst + p2) = v2;
  if (s3) *reinterpret_cast<uint4 *>(dst + p3) = v3;
}

__global__ __launch_bounds__(256) void k_store_join_move(StoreJoin a) {
  const StoreJoinWs w = store_join_ws(a);
  const unsigned long long base = w.head[0], limit = w.head[2];
  for (unsigned long long lo = static_cast<unsigned long long>(blockIdx.x) * kStoreMoveTile; lo < limit;
       lo += static_cast<unsigned long long>(gridDim.x) * kStoreMoveTile) {
    const unsigned long long hi = lo + kStoreMoveTile < limit ? lo + kStoreMoveTile : limit;
    store_join_move_tile(a, w, base, lo, hi);
  }
}

// ------------------------------------------------------------------------------------------
// The cut: glc_store_cut_device (glc_kernels.h StoreCut has the plan, include/glc.h the rules).
// ------------------------------------------------------------------------------------------
struct StoreCutWs {  // the workspace's arrays (glc_kernels.h)
  unsigned long long *head, *found, *cut_off, *runs;
};
__device__ __forceinline__ StoreCutWs store_cut_ws(const StoreCut &a) {
  StoreCutWs w;
  w.head = reinterpret_cast<unsigned long long *>(a.ws);
  w.found = w.head + 8;
  w.cut_off = w.found + 8ull * a.n_cuts;
  w.runs = w.cut_off + a.n_cuts + 1;
  return w;
}

// C1.  Thread 0 judges the selection, the entry, the header and the window, in that order: the entry of a clip index
// outside the index is not read, nothing of a blob with an unusable entry, nothing behind a failing header.  The
// header's own frame count is bounded as glc_compact_join bounds it before a size is formed from it.  The reductions
// run over whole 16-byte units of the cnt and is_raw sections from their starts to the window's end and mask what lies
// behind it inside the last unit; a unit that holds a row of the window lies inside the section, which ends on a
// multiple of 64 inside the blob (the header rule), and no unit behind the window's last one is loaded.
__global__ __launch_bounds__(256) void k_store_cut_plan(StoreCut a) {
  __shared__ CompactHeader s_h;
  __shared__ unsigned s_bits;
  __shared__ unsigned long long s_off;
  __shared__ unsigned long long s_part[5][4];
  const StoreCutWs w = store_cut_ws(a);
  const unsigned t = threadIdx.x;
  for (unsigned long long i = blockIdx.x; i < a.n_cuts; i += gridDim.x) {
    const StoreCutItem c = a.cuts[i];
    if (t == 0) {
      unsigned bits = 0;
      unsigned long long off = 0;
      if (c.clip >= a.n_entries) {
        bits = kCompactBadCrop;  // and the entry is not read
      } else {
        const glc_store_entry e = a.entries[c.clip];
        // each term is bounded before the difference is formed: nothing wraps (k_store_plan_crops' way)
        if (e.stored == 0 || (e.offset & 63ull) || e.offset > a.arena_bytes || e.bytes > a.arena_bytes - e.offset) {
          bits = kCompactNoBlob | kCompactBadHeader;
        } else if (e.bytes < sizeof(CompactHeader)) {
          bits = kCompactBadHeader;  // not even a header
        } else {
          const uint4 *hp = reinterpret_cast<const uint4 *>(a.arena + e.offset);
          uint4 *hs = reinterpret_cast<uint4 *>(&s_h);
          hs[0] = hp[0], hs[1] = hp[1], hs[2] = hp[2], hs[3] = hp[3];
          off = e.offset;
          const unsigned long long F = s_h.n_frames;
          // the 32-bit row limit of every clip, and a frame is at least its is_raw byte (glc_compact_join's bound)
          if (F == 0 || F > 0xFFFFFFFFull / a.ch || F > e.bytes - sizeof(CompactHeader) ||
              compact_header_fault(s_h, a.ch, F, 0, true, e.bytes) != HeaderFault::kNone)
            bits = kCompactBadHeader;
          else if (c.first_frame > F || c.n_frames > F - c.first_frame)
            bits = kCompactBadCrop;
        }
      }
      s_bits = bits;
      s_off = off;
    }
    __syncthreads();
    unsigned long long p0 = 0, p = 0, r0 = 0, r = 0, over = 0;
    if (s_bits == 0) {
      const unsigned long long f0 = c.first_frame, f1 = f0 + c.n_frames, m0 = f0 * a.ch, m1 = f1 * a.ch;
      const CompactLayout l = compact_layout(a.ch, s_h.n_frames);
      const unsigned char *blob = a.arena + s_off;
      auto row = [&](unsigned long long m, unsigned n) {
        if (m >= m1) return;
        if (n > static_cast<unsigned>(kHop)) over = 1;
        if (m < m0) p0 += n; else p += n;
      };
      for (unsigned long long u = t; u * 4ull < m1; u += 256ull) {
        const uint4 v = *reinterpret_cast<const uint4 *>(blob + l.o_cnt + 16ull * u);
        const unsigned long long m = 4ull * u;
        row(m, v.x), row(m + 1, v.y), row(m + 2, v.z), row(m + 3, v.w);
      }
      auto flags = [&](unsigned long long f, unsigned word) {
#pragma unroll
        for (unsigned k = 0; k < 4u; ++k)
          if (f + k < f1 && ((word >> (8u * k)) & 0xFFu)) {
            if (f + k < f0) ++r0; else ++r;
          }
      };
      for (unsigned long long u = t; u * 16ull < f1; u += 256ull) {
        const uint4 v = *reinterpret_cast<const uint4 *>(blob + l.o_israw + 16ull * u);
        const unsigned long long f = 16ull * u;
        flags(f, v.x), flags(f + 4, v.y), flags(f + 8, v.z), flags(f + 12, v.w);
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      p0 += __shfl_down(p0, off, 64);
      p += __shfl_down(p, off, 64);
      r0 += __shfl_down(r0, off, 64);
      r += __shfl_down(r, off, 64);
      over += __shfl_down(over, off, 64);
    }
    if ((t & 63u) == 0) s_part[0][t >> 6] = p0, s_part[1][t >> 6] = p, s_part[2][t >> 6] = r0, s_part[3][t >> 6] = r, s_part[4][t >> 6] = over;
    __syncthreads();
    if (t == 0) {
      unsigned bits = s_bits;
      auto sum = [&](int k) { return s_part[k][0] + s_part[k][1] + s_part[k][2] + s_part[k][3]; };
      const unsigned long long P0 = sum(0), P = sum(1), R0 = sum(2) * a.ch, R = sum(3) * a.ch;
      if (bits == 0) {
        if (sum(4) != 0 || P0 + P > s_h.n_pairs) bits |= kCompactRowBounds;
        if (R0 + R > s_h.n_raw_rows) bits |= kCompactRawRange;
      }
      a.cut_status[i] = bits;
      unsigned long long *f = w.found + 8ull * i;
      f[0] = bits ? 0ull : s_off;
      f[1] = bits ? 0ull : P0;
      f[2] = bits ? 0ull : P;
      f[3] = bits ? 0ull : R0;
      f[4] = bits ? 0ull : R;
      f[5] = bits ? 1ull : 0ull;
      f[6] = bits ? 0ull : s_h.n_frames;
      f[7] = bits ? 0ull : s_h.n_pairs;
    }
    __syncthreads();  // s_h, s_bits, s_off and s_part are rewritten by the next cut
  }
}

// C2.  k_store_place's placement rule word for word, a refused cut counting 0; then, per cut, where its five runs lie
// in the arena: the window's slice of each of the source's sections (the source's layout from ITS frame and pair
// counts, the pairs behind the P0 in front, the planes behind the R0 in front).
__global__ __launch_bounds__(1024) void k_store_cut_scan(StoreCut a) {
  __shared__ unsigned long long s[1024];
  __shared__ unsigned long long s_limit;
  const StoreCutWs w = store_cut_ws(a);
  const unsigned t = threadIdx.x;
  if (t == 0) s_limit = 0ull;
  const unsigned long long base = align64(*a.cursor);  // every thread reads it here; thread 0 writes it behind the last barrier
  unsigned long long carry = base;
  unsigned long long *out = reinterpret_cast<unsigned long long *>(a.entries_out);
  for (unsigned long long c0 = 0; c0 < a.n_cuts; c0 += 1024) {
    const unsigned long long i = c0 + t;
    unsigned long long bytes = 0, P = 0, R = 0;
    StoreCutItem c{};
    bool ok = false;
    if (i < a.n_cuts) {
      c = a.cuts[i];
      ok = w.found[8 * i + 5] == 0;
      if (ok) {
        P = w.found[8 * i + 2], R = w.found[8 * i + 4];
        bytes = compact_raw_offset(compact_layout(a.ch, c.n_frames), P) + R * (kFrameI * 2ull);
      }
    }
    scan_sum_1024(s, bytes);
    const unsigned long long offset = carry + s[t] - bytes;  // exclusive: every size is a multiple of 64
    const unsigned long long chunk_total = s[1023];
    __syncthreads();
    carry += chunk_total;
    if (i < a.n_cuts) {
      const bool stored = ok && offset <= a.dst_bytes && bytes <= a.dst_bytes - offset;  // the encoder's rule (k_store_place)
      out[4 * i] = ok ? offset : 0ull;
      out[4 * i + 1] = bytes;
      out[4 * i + 2] = P;
      out[4 * i + 3] = R | (stored ? 1ull << 32 : 0ull);
      a.lengths_out[i] = ok ? c.length : 0;
      w.cut_off[i] = offset - base;
      unsigned long long *run = w.runs + 10ull * i;
      const unsigned long long *f = w.found + 8ull * i;
      const CompactLayout ls = compact_layout(a.ch, f[6]);
      const unsigned long long rows0 = c.first_frame * a.ch, rows = c.n_frames * a.ch;
      run[0] = ok ? f[0] + ls.o_israw + c.first_frame : 0ull, run[1] = ok ? c.n_frames : 0ull;
      run[2] = ok ? f[0] + ls.o_scale + 4ull * rows0 : 0ull, run[3] = ok ? 4ull * rows : 0ull;
      run[4] = ok ? f[0] + ls.o_cnt + 4ull * rows0 : 0ull, run[5] = ok ? 4ull * rows : 0ull;
      run[6] = ok ? f[0] + ls.o_pairs + 4ull * f[1] : 0ull, run[7] = ok ? 4ull * P : 0ull;
      run[8] = ok ? f[0] + compact_raw_offset(ls, f[7]) + f[3] * (kFrameI * 2ull) : 0ull, run[9] = ok ? R * (kFrameI * 2ull) : 0ull;
      if (stored) {
        *reinterpret_cast<CompactHeader *>(a.dst + offset) = compact_header(a.ch, c.n_frames, P, R, bytes);
        atomicMax(&s_limit, offset + bytes - base);
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    w.cut_off[a.n_cuts] = carry - base;
    w.head[0] = base;
    w.head[1] = carry - base;
    w.head[2] = s_limit;
    *a.cursor = carry;
  }
}

// M.  Where a byte of the packed destination space comes from.  A piece's blob is its header (C2 wrote it) and five
// runs - is_raw, scale, cnt, pairs, raw -, each ONE contiguous range of the arena (C2's table), each followed by zeros
// up to the next multiple of 64.  A refused cut has no bytes and shares its start with the next one: the search takes
// the LAST cut that starts at or below the byte, which is the one that holds it (below `limit` that is a stored one).
enum : unsigned { kCutHeader = 0, kCutIsRaw, kCutScale, kCutCnt, kCutPairs, kCutRaw };
struct CutRun {  // one run of one cut
  unsigned long long cut, at, len, src;  // at: the run's packed offset; len: its bytes without the padding; src: in the arena
  unsigned sec;
};
// the run that holds packed byte p, the cut sought in [c_lo, c_hi]
__device__ __forceinline__ CutRun cut_run(const StoreCut &a, const StoreCutWs &w, unsigned long long p, unsigned long long c_lo,
                                          unsigned long long c_hi) {
  while (c_lo < c_hi) {
    const unsigned long long mid = c_lo + (c_hi - c_lo + 1) / 2;
    if (w.cut_off[mid] <= p) c_lo = mid; else c_hi = mid - 1;
  }
  const unsigned long long base = w.cut_off[c_lo], rel = p - base;
  const CompactLayout l = compact_layout(a.ch, a.cuts[c_lo].n_frames);
  const unsigned long long *run = w.runs + 10ull * c_lo;
  const unsigned long long o_raw = align64(l.o_pairs + run[7]);
  CutRun r;
  r.cut = c_lo;
  if (rel < l.o_israw) {
    r.sec = kCutHeader, r.at = base, r.len = l.o_israw, r.src = 0ull;
    return r;
  }
  if (rel < l.o_scale) r.sec = kCutIsRaw, r.at = base + l.o_israw;
  else if (rel < l.o_cnt) r.sec = kCutScale, r.at = base + l.o_scale;
  else if (rel < l.o_pairs) r.sec = kCutCnt, r.at = base + l.o_cnt;
  else if (rel < o_raw) r.sec = kCutPairs, r.at = base + l.o_pairs;
  else r.sec = kCutRaw, r.at = base + o_raw;
  r.src = run[2u * (r.sec - 1u)], r.len = run[2u * (r.sec - 1u) + 1u];
  return r;
}

// The 16 bytes of run r from its byte u on.  A unit inside the run is join_load16 of src + u: both aligned units it
// loads hold a byte of the run, so both lie inside the source blob, whose offset and size are multiples of 64.  The
// run's last unit where the run does not end on 16 takes dword loads (byte loads in is_raw; the dword runs start and
// end on dwords) of what the run holds and is zero behind it, as is every unit of the padding.
__device__ __forceinline__ uint4 cut_unit(const unsigned char *arena, const CutRun &r, unsigned long long u) {
  uint4 v{};
  if (u >= r.len) return v;
  const unsigned long long at = r.src + u;
  if (u + 16ull <= r.len) return join_load16(arena, at);
  const unsigned left = static_cast<unsigned>(r.len - u);  // 1 .. 15
  if (r.sec == kCutIsRaw) {
    auto word = [&](unsigned k) {
      unsigned x = 0;
#pragma unroll
      for (unsigned b = 0; b < 4u; ++b)
        if (k + b < left) x |= static_cast<unsigned>(arena[at + k + b]) << (8u * b);
      return x;
    };
    v.x = word(0), v.y = word(4), v.z = word(8), v.w = word(12);
  } else {
    auto word = [&](unsigned k) { return k < left ? *reinterpret_cast<const unsigned *>(arena + at + k) : 0u; };
    v.x = word(0), v.y = word(4), v.z = word(8), v.w = word(12);
  }
  return v;
}

// Packed bytes [lo, hi) - multiples of 16, hi - lo <= kStoreMoveTile, hi <= limit - to dst + base.  The runs of the
// tile's first and last unit are found once (the same search in every lane: uniform).  Where they are one run of one
// cut every unit of the tile lies in it or in its padding, and its source is the tile's one base plus p: no search and
// no table load per unit.  Otherwise a unit finds its cut between the two and its run from that cut's layout.  Four
// units per thread, all loads in front of all stores, named scalars (the comment at store_evict_gather_tile).
__device__ __forceinline__ void store_cut_move_tile(const StoreCut &a, const StoreCutWs &w, unsigned long long base,
                                                    unsigned long long lo, unsigned long long hi) {
  const CutRun r_lo = cut_run(a, w, lo, 0, a.n_cuts - 1), r_hi = cut_run(a, w, hi - 16, r_lo.cut, a.n_cuts - 1);
  const bool one_run = r_lo.cut == r_hi.cut && r_lo.sec == r_hi.sec && r_lo.sec != kCutHeader;
  auto unit = [&](unsigned long long p, bool &live) {
    uint4 v{};
    live = false;
    if (p >= hi) return v;
    if (one_run) {
      live = true;
      return cut_unit(a.arena, r_lo, p - r_lo.at);
    }
    const CutRun r = cut_run(a, w, p, r_lo.cut, r_hi.cut);
    if (r.sec == kCutHeader) return v;  // C2 wrote it
    live = true;
    return cut_unit(a.arena, r, p - r.at);
  };
  const unsigned long long p0 = lo + threadIdx.x * 16ull, p1 = p0 + 4096ull, p2 = p0 + 8192ull, p3 = p0 + 12288ull;
  bool s0, s1, s2, s3;
  const uint4 v0 = unit(p0, s0), v1 = unit(p1, s1), v2 = unit(p2, s2), v3 = unit(p3, s3);
  unsigned char *dst = a.dst + base;
  if (s0) *reinterpret_cast<uint4 *>(dst + p0) = v0;
  if (s1) *reinterpret_cast<uint4 *>(dst + p1) = v1;
  if (s2) *reinterpret_cast<uint4 *>(dst + p2) = v2;
  if (s3) *reinterpret_cast<uint4 *>(dst + p3) = v3;
}

__global__ __launch_bounds__(256) void k_store_cut_move(StoreCut a) {
  const StoreCutWs w = store_cut_ws(a);
  const unsigned long long base = w.head[0], limit = w.head[2];
  for (unsigned long long lo = static_cast<unsigned long long>(blockIdx.x) * kStoreMoveTile; lo < limit;
       lo += static_cast<unsigned long long>(gridDim.x) * kStoreMoveTile) {
    const unsigned long long hi = lo + kStoreMoveTile < limit ? lo + kStoreMoveTile : limit;
    store_cut_move_tile(a, w, base, lo, hi);
  }
}

// ------------------------------------------------------------------------------------------
// S1: the virtual stream of a round of glc_roundtrip_batch_device, gathered from clips that lie strided
// (and, `planar`, one plane per channel) in the caller's memory.  Workgroup row blockIdx.x is virtual frame
// slot v: the 1024 * ch interleaved samples [1024 v, 1024 v + 1024) of the stream.  Its clip is the last one
// whose `slot` is <= v - a binary search per WORKGROUP (block-uniform, scalar loads), not per element.
// Everything at or behind the clip's `len` samples is written as +0.0 in the same pass: the zeros behind
// a clip and its junk frame need no memset.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ StageClip stage_find_clip(const StageClip *__restrict__ clips, unsigned n_clips, unsigned v) {
  unsigned lo = 0, hi = n_clips;  // clips[lo].slot <= v < clips[hi].slot
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (clips[mid].slot <= v) lo = mid;
    else hi = mid;
  }
  return clips[lo];
}

// Elements [t, t + 4) of a run of `len` samples of S (float, or int16_t / int32_t widened by pcm_widen1 with
// `inv`; +0.0 past the run's end - the reference's padding, never a widened integer zero).  A run that starts off
// the boundary of a vector of four S (16 bytes of float4 / int4, 8 of short4) is read as the two aligned
// vectors around the four - both inside the run, so nothing outside the caller's samples is touched; only where
// one of them would cross the run's first or last element (its edges) do the four come one by one.  `mis`
// counts ELEMENTS from the vector boundary: an int16 run may start at any 2-byte address.  t advances by 4 per
// thread, so the case is wave-uniform.
template <typename S>
struct StageVec4;
template <>
struct StageVec4<float> { using type = float4; };
template <>
struct StageVec4<short> { using type = short4; };
template <>
struct StageVec4<int> { using type = int4; };

template <typename S>
__device__ __forceinline__ float stage_widen(S s, float inv) {
  if constexpr (std::is_same<S, float>::value) return s;
  else return pcm_widen1(s, inv);
}

template <typename S>
__device__ __forceinline__ float4 stage_load4(const S *__restrict__ run, unsigned long long t, unsigned long long len, float inv) {
  using S4 = typename StageVec4<S>::type;
  const S *p = run + t;
  const unsigned mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) / sizeof(S)) & 3u;
  if (mis == 0 && t + 4 <= len) {
    const S4 a = *reinterpret_cast<const S4 *>(p);
    return float4{stage_widen(a.x, inv), stage_widen(a.y, inv), stage_widen(a.z, inv), stage_widen(a.w, inv)};
  }
  if (mis != 0 && t >= mis && t - mis + 8 <= len) {
    const S4 a = *reinterpret_cast<const S4 *>(p - mis), b = *reinterpret_cast<const S4 *>(p - mis + 4);
    if (mis == 1) return float4{stage_widen(a.y, inv), stage_widen(a.z, inv), stage_widen(a.w, inv), stage_widen(b.x, inv)};
    if (mis == 2) return float4{stage_widen(a.z, inv), stage_widen(a.w, inv), stage_widen(b.x, inv), stage_widen(b.y, inv)};
    return float4{stage_widen(a.w, inv), stage_widen(b.x, inv), stage_widen(b.y, inv), stage_widen(b.z, inv)};
  }
  float4 r;
  r.x = t < len ? stage_widen(p[0], inv) : 0.0f;
  r.y = t + 1 < len ? stage_widen(p[1], inv) : 0.0f;
  r.z = t + 2 < len ? stage_widen(p[2], inv) : 0.0f;
  r.w = t + 3 < len ? stage_widen(p[3], inv) : 0.0f;
  return r;
}

// Interleaved clips (and mono planar ones, which are the same thing): a clip is ONE run of len * ch samples,
// a thread converts four of them into a float4.  grid (V, ch).
template <typename S>
__global__ __launch_bounds__(256) void k_stage_clips(const S *__restrict__ src, const StageClip *__restrict__ clips,
                                                      unsigned n_clips, unsigned ch, float inv, float *__restrict__ vs) {
  const unsigned v = blockIdx.x;
  const StageClip cl = stage_find_clip(clips, n_clips, v);
  const unsigned per_hop = static_cast<unsigned>(kHopI) * ch;
  const unsigned o = (blockIdx.y * 256u + threadIdx.x) * 4u;
  if (o >= per_hop) return;
  const unsigned long long t = static_cast<unsigned long long>(v - cl.slot) * per_hop + o;
  *reinterpret_cast<float4 *>(vs + static_cast<size_t>(v) * per_hop + o) = stage_load4(src + cl.src, t, cl.len * ch, inv);
}

// Planar clips of 2 / 4 / 8 channels: a thread takes the same four samples of every plane (CH coalesced
// vector loads, one plane each) and stores them interleaved as CH float4.  grid (V).
template <int CH, typename S>
__global__ __launch_bounds__(256) void k_stage_clips_planar(const S *__restrict__ src, const StageClip *__restrict__ clips,
                                                             unsigned n_clips, unsigned long long cstride, float inv,
                                                             float *__restrict__ vs) {
  const unsigned v = blockIdx.x;
  const StageClip cl = stage_find_clip(clips, n_clips, v);
  const unsigned i0 = threadIdx.x * 4u;
  const unsigned long long t = static_cast<unsigned long long>(v - cl.slot) * kHopI + i0;
  float q[4 * CH];  // [sample][channel]
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float4 p = stage_load4(src + cl.src + c * cstride, t, cl.len, inv);
    q[c] = p.x, q[CH + c] = p.y, q[2 * CH + c] = p.z, q[3 * CH + c] = p.w;
  }
  float4 *dst = reinterpret_cast<float4 *>(vs + (static_cast<size_t>(v) * kHopI + i0) * CH);
#pragma unroll
  for (int j = 0; j < CH; ++j) dst[j] = float4{q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]};
}

// Planar clips of any other channel count: a thread owns a float4 of the interleaved OUTPUT and fetches its
// four samples one by one (a division each).  grid (V, ch).
template <typename S>
__global__ __launch_bounds__(256) void k_stage_clips_planar_any(const S *__restrict__ src,
                                                                 const StageClip *__restrict__ clips, unsigned n_clips,
                                                                 unsigned ch, unsigned long long cstride, float inv,
                                                                 float *__restrict__ vs) {
  const unsigned v = blockIdx.x;
  const StageClip cl = stage_find_clip(clips, n_clips, v);
  const unsigned per_hop = static_cast<unsigned>(kHopI) * ch;
  const unsigned o = (blockIdx.y * 256u + threadIdx.x) * 4u;
  if (o >= per_hop) return;
  const unsigned long long t0 = static_cast<unsigned long long>(v - cl.slot) * kHopI;
  float q[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned i = (o + e) / ch, c = (o + e) - i * ch;
    q[e] = t0 + i < cl.len ? stage_widen(src[cl.src + c * cstride + t0 + i], inv) : 0.0f;
  }
  *reinterpret_cast<float4 *>(vs + static_cast<size_t>(v) * per_hop + o) = float4{q[0], q[1], q[2], q[3]};
}

// ------------------------------------------------------------------------------------------
// S2: the segment stager of a streaming push (glc_kernels.h StreamSpan).  Workgroup row blockIdx.x is a UNIT of 512
// samples per channel: units [0, vs_units) are the half hops of the round's virtual stream, the ones behind them the
// quarters of the lanes' new held-back buffers.  A unit's span is the last one whose `unit` is <= it (a binary search
// per workgroup, as S1); unit 0 and unit vs_units - 1 belong to no lane and are +0.0.  Sample x of a lane comes from
// what it held back (x < received), from the new chunk (x < received + n_new), and is +0.0 in front of sample 0 and
// behind the chunk.  A thread owns a float4 of the interleaved destination and fetches its four samples one by one.
// The held-back samples are read from one buffer and written to the other, so no order among the workgroups matters.
// grid (units, ch).
// ------------------------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(256) void k_stage_segments(const S *__restrict__ src, const StreamSpan *__restrict__ spans,
                                                         unsigned n_spans, unsigned vs_units, unsigned ch, unsigned planar,
                                                         unsigned long long cstride, float inv, float *__restrict__ held,
                                                         float *__restrict__ vs) {
  const unsigned u = blockIdx.x;
  const unsigned per_unit = 512u * ch;
  const unsigned o = (blockIdx.y * 256u + threadIdx.x) * 4u;
  if (o >= per_unit) return;
  if (u < vs_units && (u == 0 || u + 1 == vs_units)) {
    *reinterpret_cast<float4 *>(vs + static_cast<size_t>(u) * per_unit + o) = float4{0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  unsigned lo = 0, hi = n_spans;  // spans[lo].unit <= u < spans[hi].unit
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (spans[mid].unit <= u) lo = mid;
    else hi = mid;
  }
  const StreamSpan sp = spans[lo];
  const long long x_unit = sp.x0 + 512ll * static_cast<long long>(u - sp.unit);
  const long long received = static_cast<long long>(sp.received), end = static_cast<long long>(sp.received + sp.n_new);
  const long long held_x = static_cast<long long>(sp.held_x);
  float q[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned i = (o + e) / ch, c = (o + e) - i * ch;
    const long long x = x_unit + i;
    float v = 0.0f;
    if (x >= held_x && x < received) {
      v = held[sp.held_old + static_cast<unsigned long long>(x - held_x) * ch + c];
    } else if (x >= received && x < end) {
      const unsigned long long t = static_cast<unsigned long long>(x - received);
      v = stage_widen(src[sp.src + (planar ? c * cstride + t : t * ch + c)], inv);
    }
    q[e] = v;
  }
  float *dst = u < vs_units ? vs + static_cast<size_t>(u) * per_unit : held + sp.held_new + static_cast<size_t>(u - sp.unit) * per_unit;
  *reinterpret_cast<float4 *>(dst + o) = float4{q[0], q[1], q[2], q[3]};
}

// ------------------------------------------------------------------------------------------
// Clock probe (include/glc_debug.h, measurement only): ONE wave that sleeps beside whatever else runs
// on the device and reads the shader-clock counter (s_memtime) against the constant 100 MHz counter
// (s_memrealtime) over `ticks_100mhz`: shader cycles / reference ticks x 100 MHz = the clock the chip
// held over that window (MI355X_MICROARCH.md, DVFS give-back item 6).  It executes a handful of scalar
// instructions per microsecond; nothing of the product reads what it writes.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_clock_probe(unsigned long long ticks_100mhz, unsigned long long *__restrict__ out) {
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = r0;
  while (r1 - r0 < ticks_100mhz) {
    __builtin_amdgcn_s_sleep(32);
    r1 = __builtin_amdgcn_s_memrealtime();
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) {
    out[0] = t1 - t0;
    out[1] = r1 - r0;
  }
}

}  // namespace

hipError_t launch_clock_probe(uint64_t ticks_100mhz, uint64_t *out, hipStream_t s) {
  hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, static_cast<unsigned long long>(ticks_100mhz),
                     reinterpret_cast<unsigned long long *>(out));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- launchers

// Which kernel takes a launch of 3584 / 4096 rows or more (the rest of the dispatch is by row count alone):
//   st 16 waves  256 x 128 tiles, one 1024-thread workgroup per CU: a launch runs in rounds of 256 tiles;
//   st 8 waves   256 x 64 tiles, two 512-thread workgroups per CU: rounds of 512, and a CU with one
//                workgroup left finishes it in about 0.6 of a round.
// The 16-wave form is 2 % faster on full rounds (its staging and barrier cost nothing: k1_tune [abl]) and
// worse on a last round that is half empty - so it takes the launches whose last round of 32 row tiles is
// full or more than half full, the 8-wave form the rest (profiles/r03_k1_tune_st_*.txt).
bool mdct_forward_has_segment_loader(uint32_t ch) { return ch == 1 || ch == 2 || ch == 4 || ch == 8; }

namespace {
template <int NW>
hipError_t launch_st_ch(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                        hipStream_t s) {
  // PCM by one dwordx4 per lane and piece when the channel count divides the tile height, else one
  // dword per (row, sample).  PRIO: 8 waves - by quarter of the i loop (between a CU's two workgroups);
  // 16 waves - by distance from the last barrier (inside the workgroup).
  constexpr int P = NW == 8 ? 1 : 2;
  return by_channels(pcm.ch, [&](auto CH) {
    return k1::launch_st<4, decltype(CH)::value, P, 4, NW>(t, pcm, frame_begin, M, coef, s);
  });
}
hipError_t launch_dma_ch(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin, uint32_t M, float *coef,
                         hipStream_t s) {
  return by_channels(pcm.ch, [&](auto CH) {
    return k1::launch_dma<4, decltype(CH)::value, 1>(t, pcm, frame_begin, M, coef, s);
  });
}
}  // namespace

hipError_t launch_mdct_forward(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin,
                               uint32_t M, float *coef, hipStream_t s, int variant, bool beside) {
  // Shapes measured with tools/k1_tune.hip.  The f32 VALU needs >= 4 waves per SIMD to approach its
  // issue rate, so every kernel for 4096 rows or more keeps 4 x 8 outputs per lane (32 accumulators) and
  // 16 waves per CU.
  // A clip of a few seconds is latency-bound by one wave's chain of 2048 dependent i-steps, not by
  // throughput, and the length of a step is the lane tile: cut it until every SIMD has a wave of its own
  // (glc_mdct_fwd.hpp k_mdct_fwd_small: 2 x 2 outputs per lane, then 2 x 4).  Measured against the 4 x 8
  // kernels (profiles/r03_k1_tune_short_clips.txt, r03_k1_tune_mid_sizes.txt): 172 rows 0.053-0.058 ms (4 x 8
  // tile: 0.19), 600 rows 0.10, 1024 rows 0.11, 2048 rows 0.20, 3072 rows 0.28; a launch of 256-row tiles costs
  // 0.28-0.34 ms however few rows it has (one workgroup's chain) and draws level at about 3500 rows - when
  // the channel count has a segment loader; with one dword per (row, sample) only at 4096.  (Rounds 1-3 used a
  // 64 x 128 kernel for 1793..4095 rows: 0.22 ms at 2048 rows, 0.34 at 3072 - slower than both neighbours when
  // a launch has the chip to itself; it keeps one job, below.)
  const bool seg = mdct_forward_has_segment_loader(pcm.ch);
  if (M <= 640) return k1::launch_small<2>(t, pcm, frame_begin, M, coef, s);
  // beside: an opening round of glc_encode (2048 rows), which runs beside its neighbours' kernels on a second
  // stream.  Alone the 2 x 4 kernel is faster there (0.198 against 0.221 ms), but its 1024 workgroups fill every
  // CU four deep and two such launches get in each other's way; the 64 x 128 kernel of rounds 1-3 puts ONE
  // workgroup on each CU: glc_encode at config 2 1.00-1.02 ms against 1.05-1.08 (profiles/r03_encode_rounds_kernel.txt).
  if ((beside || variant == 4) && M > 1792 && M <= 2048) return k1::launch_sched<64, 128, 16, 4>(t, pcm, frame_begin, M, coef, s);
  if (M < (seg ? 3584u : 4096u)) return k1::launch_small<4>(t, pcm, frame_begin, M, coef, s);
  // variant (include/glc_debug.h glc_debug_set_mdct_variant): 0 = shipped, 1 = round 3's kernel, 2 / 3 = one form for every launch
  if (variant == 1) return launch_dma_ch(t, pcm, frame_begin, M, coef, s);
  if (variant == 2) return launch_st_ch<8>(t, pcm, frame_begin, M, coef, s);
  if (variant == 3) return launch_st_ch<16>(t, pcm, frame_begin, M, coef, s);
  if (mdct_forward_is_st16(M, pcm.ch, variant)) return launch_st_ch<16>(t, pcm, frame_begin, M, coef, s);
  return launch_st_ch<8>(t, pcm, frame_begin, M, coef, s);
}

bool mdct_forward_is_st16(uint32_t M, uint32_t ch, int variant) {
  if (M < (mdct_forward_has_segment_loader(ch) ? 3584u : 4096u) || variant == 1 || variant == 2) return false;
  if (variant == 3) return true;
  const unsigned last_round = ((M + 255) / 256) % 32;  // row tiles in the last round of 32
  return last_round == 0 || last_round > 16;
}

bool encode_screen_shape(const uint32_t *edges, uint32_t n_bands, ScreenShape *sh) {
  if (!edges || n_bands == 0 || n_bands > 64) return false;
  sh->l0 = edges[n_bands - 1];
  sh->c0 = (sh->l0 + 63u) / 64u * 64u;
  sh->ne = sh->c0 / 64u;
  if (sh->ne < 1 || sh->ne > 15) return false;
  // The balanced wave layout of k_mdct_mix_st (glc_mdct_fwd.hpp mix_wave) wherever it exists.  The plane count
  // follows from the choice, and the workspace size, its carving and the quantiser's loop read it from here alone.
  sh->hp = static_cast<uint32_t>(k1::mix_hybrid_pairs(static_cast<int>(sh->ne)));
  sh->n_planes = static_cast<uint32_t>(k1::mix_planes(static_cast<int>(sh->ne), static_cast<int>(sh->hp)));
  return true;
}

namespace {
__global__ __launch_bounds__(64) void k_debug_mfma_bf16(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b,
                                                        const float *__restrict__ c, float *__restrict__ d) {
  const int lane = threadIdx.x;
  const k1::bf16x8 av = __builtin_bit_cast(k1::bf16x8, reinterpret_cast<const uint4 *>(a)[lane]);
  const k1::bf16x8 bv = __builtin_bit_cast(k1::bf16x8, reinterpret_cast<const uint4 *>(b)[lane]);
  k1::f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = c[lane * 16 + e];
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
#pragma unroll
  for (int e = 0; e < 16; ++e) d[lane * 16 + e] = acc[e];
}
}  // namespace

hipError_t launch_debug_mfma_bf16(const uint16_t *a, const uint16_t *b, const float *c, float *d, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_mfma_bf16, dim3(1), dim3(64), 0, s, a, b, c, d);
  return hipGetLastError();
}

bool encode_matrix_bound_built(const DeviceTables &t, const ScreenShape &sh, uint32_t ch) {
  return t.cos_bf && sh.ne == static_cast<uint32_t>(MatrixBound::kNe) && (ch == 1 || ch == 2 || ch == 4 || ch == 8);
}

namespace {
inline uint64_t screen_stride(uint32_t M) { return (static_cast<uint64_t>(M) + 255ull) / 256ull * 256ull; }
}  // namespace

uint64_t encode_screen_bytes(uint32_t M, const ScreenShape &sh) {
  // hf planes | row flags | failed rows per quantiser wave (a quarter of a plane is more than it needs)
  return ((sh.n_planes + 1ull) * screen_stride(M) + screen_stride(M) + screen_stride(M) / 4) * 4ull;
}

hipError_t launch_encode_screened(const DeviceTables &t, const ScreenShape &sh, const PcmView &pcm, uint64_t frame_begin,
                                  uint32_t M, float *coef, const ScreenLaunch &launch, bool *decided) {
  void *const workspace = launch.workspace;
  uint32_t *const host_stat = launch.host_stat;
  const uint32_t seq = launch.seq;
  uint8_t *const records = launch.records;
  const hipStream_t s = launch.s;
  const bool latency_repair = launch.latency_repair, matrix_bound = launch.matrix_bound;
  const EdgeLaunch *const edge = launch.edge;
  *decided = pcm.ch == 1 || pcm.ch == 2 || pcm.ch == 4;
  if (M == 0) return hipSuccess;
  // the edge rows the side stream takes: none without `edge`, and then every kernel below is what it always was
  const unsigned long long edge_a = edge ? edge->a : 0ull, edge_b = edge ? edge->b : kNoEdge;
  const EdgeRows er = edge_rows(edge_a, edge_b, frame_begin, M, pcm.ch);
  if (edge && (er.n == 0 || er.n > kEdgeRowsMax || !edge->side || edge->side == s || !edge->coef || !edge->failed_total))
    return hipErrorInvalidValue;
  const uint64_t stride = screen_stride(M);
  float *hf = static_cast<float *>(workspace);
  // the workspace is carved for the FMA form, the larger of the two: the matrix form's 4 planes and its A plane lie
  // at the front of the FMA form's, the flags and counts where they always are
  unsigned *row_flag = reinterpret_cast<unsigned *>(hf + (sh.n_planes + 1ull) * stride);
  unsigned *wave_fail = row_flag + stride;
  static_assert(MatrixBound::kGroups <= 8, "the matrix form's planes fit in those of any FMA form (8 at the least)");
  if (matrix_bound && !encode_matrix_bound_built(t, sh, pcm.ch)) return hipErrorInvalidValue;
  const unsigned n_planes = matrix_bound ? static_cast<unsigned>(MatrixBound::kGroups) : sh.n_planes;
  hipError_t e;
  if (edge && (e = hipEventRecord(edge->ev_fork, s)) != hipSuccess) return e;
  if (matrix_bound)  // (encode_matrix_bound_built has refused every count but 1 / 2 / 4 / 8: no form for any count is built)
    e = by_channels<8>(pcm.ch, [&](auto CH) {
      return k1::launch_mx_st<decltype(CH)::value>(t, pcm, frame_begin, M, coef, hf, stride, s);
    });
  else
    e = by_channels(pcm.ch, [&](auto CH) {
      return k1::launch_mix_st<decltype(CH)::value>(t, pcm, frame_begin, M, coef, sh.ne, sh.hp, hf, stride, s);
    });
  if (e != hipSuccess) return e;
  const ScreenArgs sa{hf, row_flag, wave_fail, host_stat, stride, sh.c0, sh.l0, n_planes, seq, edge_a, edge_b,
                      edge ? edge->failed_total : nullptr};
  const unsigned long long hdr = record_header_bytes(pcm.ch), rec = record_bytes(pcm.ch);
  const dim3 grid((M + 4 * kQRows - 1) / (4 * kQRows));
  const long long fb = static_cast<long long>(frame_begin);
  // from the side stream's first command on, every way out joins it: the caller's stream never goes on beside it
  bool forked = false;
  auto leave = [&](hipError_t err) -> hipError_t {
    if (!forked) return err;
    hipError_t j = hipEventRecord(edge->ev_edge, edge->side);
    if (j == hipSuccess) j = hipStreamWaitEvent(s, edge->ev_edge, 0);
    return err != hipSuccess ? err : j;
  };
  if (edge) {
    // The side stream needs only what was on the stream before K1 (the PCM): the edge transform forms all 1024
    // columns of its rows in a buffer of their own, so neither it nor the edge quantiser waits for a kernel of this
    // launch, and no event stands between K1 and K2.  It is queued behind K1 so that K1's single round of workgroups
    // is on the chip first; its waves take the CUs K1 leaves.
    if ((e = hipStreamWaitEvent(edge->side, edge->ev_fork, 0)) != hipSuccess) return e;
    forked = true;
    e = edge->capped ? k1::launch_edge_rows<GLC_SMALL_ROWS_R, true>(t, pcm, frame_begin, M, edge->coef, er, 0u, edge->side)
                     : k1::launch_edge_rows<GLC_SMALL_ROWS_R, false>(t, pcm, frame_begin, M, edge->coef, er, 0u, edge->side);
    if (e != hipSuccess) return leave(e);
    const unsigned g_pre = (er.n_pre + 15u) / 16u, g_suf = std::max(er.suf0 / 16u, g_pre), g_end = (M + 15u) / 16u;
    const dim3 egrid(g_pre + (er.suf0 < M && g_suf < g_end ? g_end - g_suf : 0u));
    if (*decided)
      hipLaunchKernelGGL((k_quantize_screen<true, 3>), egrid, dim3(256), 0, edge->side, t, edge->coef, M, pcm.ch, rec, hdr, pcm, fb, records, sa);
    else
      hipLaunchKernelGGL((k_quantize_screen<false, 3>), egrid, dim3(256), 0, edge->side, t, edge->coef, M, pcm.ch, rec, hdr, pcm, fb, records, sa);
    if ((e = hipGetLastError()) != hipSuccess) return leave(e);
  }
  if (*decided)
    hipLaunchKernelGGL((k_quantize_screen<true, 1>), grid, dim3(256), 0, s, t, coef, M, pcm.ch, rec, hdr, pcm, fb, records, sa);
  else
    hipLaunchKernelGGL((k_quantize_screen<false, 1>), grid, dim3(256), 0, s, t, coef, M, pcm.ch, rec, hdr, pcm, fb, records, sa);
  if ((e = hipGetLastError()) != hipSuccess) return leave(e);
  // the repair: exact columns C0.. of the failed rows - one wave per (two failed rows, 64 columns) found through the
  // fail counts where few rows fail, the row tiles that hold a failed row where many do - then those rows' records
  // from all 1024 exact coefficients.  Every launch leaves at once where nothing failed.
  e = latency_repair ? k1::launch_small_rows<GLC_SMALL_ROWS_R>(t, pcm, frame_begin, M, coef, row_flag, wave_fail, sh.c0, s)
                     : k1::launch_small_cols<2>(t, pcm, frame_begin, M, coef, row_flag, sh.c0, s);
  if (e != hipSuccess) return leave(e);
  if (*decided)
    hipLaunchKernelGGL((k_quantize_screen<true, 2>), grid, dim3(256), 0, s, t, coef, M, pcm.ch, rec, hdr, pcm, fb, records, sa);
  else
    hipLaunchKernelGGL((k_quantize_screen<false, 2>), grid, dim3(256), 0, s, t, coef, M, pcm.ch, rec, hdr, pcm, fb, records, sa);
  // the join: the stream goes on (K3, the caller's own work) only behind the edge rows' records
  return leave(hipGetLastError());
}

hipError_t launch_quantize(const DeviceTables &t, const float *coef, uint32_t M, uint32_t ch, const PcmView &pcm,
                           uint64_t frame_begin, uint8_t *records, hipStream_t s, bool *decided) {
  *decided = ch == 1 || ch == 2 || ch == 4;  // a frame's rows sit in one wave: K2 decides raw-vs-compressed itself
  if (M == 0) return hipSuccess;
  const unsigned long long hdr = record_header_bytes(ch), rec = record_bytes(ch);
  const dim3 grid((M + 4 * kQRows - 1) / (4 * kQRows));
  if (*decided)
    hipLaunchKernelGGL(k_quantize<true>, grid, dim3(256), 0, s, t, coef, M, ch, rec, hdr, pcm,
                       static_cast<long long>(frame_begin), records);
  else
    hipLaunchKernelGGL(k_quantize<false>, grid, dim3(256), 0, s, t, coef, M, ch, rec, hdr, pcm,
                       static_cast<long long>(frame_begin), records);
  return hipGetLastError();
}

hipError_t launch_decide_raw(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin,
                             uint32_t n_frames, uint8_t *records, hipStream_t s) {
  if (n_frames == 0) return hipSuccess;
  const unsigned long long hdr = record_header_bytes(pcm.ch), rec = record_bytes(pcm.ch);
  hipLaunchKernelGGL(k_decide_raw, dim3(n_frames), dim3(256), 0, s, t, pcm,
                     static_cast<long long>(frame_begin), n_frames, rec, hdr, records);
  return hipGetLastError();
}

namespace {
inline uint64_t align256(uint64_t v) { return (v + 255ull) & ~255ull; }
// Consecutive 256-byte aligned arrays of a workspace.  Each workspace has ONE function that takes its arrays
// from a base: the launcher calls it with the workspace, the *_bytes() function with base 0 and reads `used`.
struct Carve {
  uintptr_t base;
  uint64_t used = 0;
  template <typename T>
  T *take(uint64_t n) {
    T *p = reinterpret_cast<T *>(base + used);
    used += align256(n * sizeof(T));
    return p;
  }
};

struct CompactScratch {  // of P1-P3 over M rows
  unsigned *loc;
  unsigned long long *blk, *blk_raw, *totals;
  uint64_t bytes;
};
CompactScratch compact_scratch(const void *base, uint64_t M) {
  const uint64_t nblk = (M + 1023) / 1024;
  Carve c{reinterpret_cast<uintptr_t>(base)};
  CompactScratch w;
  w.loc = c.take<unsigned>(M);
  w.blk = c.take<unsigned long long>(nblk);
  w.blk_raw = c.take<unsigned long long>(nblk);
  w.totals = c.take<unsigned long long>(2);
  w.bytes = c.used;
  return w;
}
}  // namespace

uint64_t compact_scratch_bytes(uint64_t M) { return compact_scratch(nullptr, M).bytes; }

hipError_t launch_compact(const uint8_t *records, uint32_t M, uint32_t ch, uint64_t n_frames, void *scratch, uint8_t *blob,
                          const CompactLayout &l, const FrameMap *frame_map, uint64_t *clip_dir, hipStream_t s) {
  static_assert(sizeof(FrameMap) == sizeof(uint2), "FrameMap is read as a uint2");
  if (!scratch || !blob || (frame_map == nullptr) != (clip_dir == nullptr)) return hipErrorInvalidValue;
  const CompactScratch w = compact_scratch(scratch, M);
  const uint2 *fmap = reinterpret_cast<const uint2 *>(frame_map);
  auto *dir = reinterpret_cast<unsigned long long *>(clip_dir);
  if (M == 0) {  // an empty range: the scans are over nothing, the header says so
    hipLaunchKernelGGL(k_pack_scan_blocks, dim3(1), dim3(1024), 0, s, w.blk, w.blk_raw, 0u, w.totals, ch, 0ull, l, blob);
    return hipGetLastError();
  }
  const unsigned long long hdr = record_header_bytes(ch), rec = record_bytes(ch);
  const unsigned nblk = (M + 1023) / 1024;
  if (fmap)
    hipLaunchKernelGGL(k_pack_scan_rows<true>, dim3(nblk), dim3(256), 0, s, records, M, ch, rec, w.loc, w.blk, w.blk_raw, l, blob, fmap);
  else
    hipLaunchKernelGGL(k_pack_scan_rows<false>, dim3(nblk), dim3(256), 0, s, records, M, ch, rec, w.loc, w.blk, w.blk_raw, l, blob, fmap);
  hipLaunchKernelGGL(k_pack_scan_blocks, dim3(1), dim3(1024), 0, s, w.blk, w.blk_raw, nblk, w.totals, ch,
                     static_cast<unsigned long long>(n_frames), l, blob);
  if (fmap)
    hipLaunchKernelGGL(k_pack_rows<true>, dim3((M + 3) / 4), dim3(256), 0, s, records, M, ch, rec, hdr, w.loc, w.blk, w.blk_raw,
                       w.totals, l, blob, fmap, dir);
  else
    hipLaunchKernelGGL(k_pack_rows<false>, dim3((M + 3) / 4), dim3(256), 0, s, records, M, ch, rec, hdr, w.loc, w.blk, w.blk_raw,
                       w.totals, l, blob, fmap, dir);
  return hipGetLastError();
}

namespace {
struct StoreScratch {  // of A1-A3 over M rows of n_clips clips
  unsigned *loc;
  unsigned long long *blk, *blk_raw, *clip_base;
  uint64_t bytes;
};
StoreScratch store_scratch(const void *base, uint64_t M, uint64_t n_clips) {
  const uint64_t nblk = (M + 1023) / 1024;
  Carve c{reinterpret_cast<uintptr_t>(base)};
  StoreScratch w;
  w.loc = c.take<unsigned>(M);
  w.blk = c.take<unsigned long long>(nblk);
  w.blk_raw = c.take<unsigned long long>(nblk);
  w.clip_base = c.take<unsigned long long>(2 * n_clips);
  w.bytes = c.used;
  return w;
}
}  // namespace

uint64_t compact_store_scratch_bytes(uint64_t M, uint64_t n_clips) { return store_scratch(nullptr, M, n_clips).bytes; }

hipError_t launch_compact_store(const uint8_t *records, uint32_t M, uint32_t ch, const FrameMap *frame_map, const ClipSpan *clips,
                                uint32_t n_clips, void *scratch, uint8_t *arena, uint64_t arena_bytes, uint64_t *cursor,
                                glc_store_entry *entries, hipStream_t s) {
  static_assert(sizeof(ClipSpan) == sizeof(uint2) && sizeof(glc_store_entry) == 32, "read and written by the kernels as laid out here");
  if (!records || !frame_map || !clips || !scratch || !arena || !cursor || !entries || ch == 0 || M == 0 || n_clips == 0 || M % ch)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(arena) & 63u) || ((reinterpret_cast<uintptr_t>(cursor) | reinterpret_cast<uintptr_t>(entries)) & 7u))
    return hipErrorInvalidValue;
  const StoreScratch w = store_scratch(scratch, M, n_clips);
  const uint2 *fmap = reinterpret_cast<const uint2 *>(frame_map), *cl = reinterpret_cast<const uint2 *>(clips);
  auto *e = reinterpret_cast<unsigned long long *>(entries);
  const unsigned long long hdr = record_header_bytes(ch), rec = record_bytes(ch);
  const unsigned nblk = (M + 1023) / 1024;
  hipLaunchKernelGGL(k_store_scan_rows, dim3(nblk), dim3(256), 0, s, records, M, ch, rec, w.loc, w.blk, w.blk_raw, fmap);
  hipLaunchKernelGGL(k_store_place, dim3(1), dim3(1024), 0, s, w.blk, w.blk_raw, nblk, w.loc, M, ch, cl, n_clips, w.clip_base, arena,
                     static_cast<unsigned long long>(arena_bytes), reinterpret_cast<unsigned long long *>(cursor), e);
  hipLaunchKernelGGL(k_store_rows, dim3((M + 3) / 4), dim3(256), 0, s, records, M, ch, rec, hdr, w.loc, w.blk, w.blk_raw, w.clip_base,
                     fmap, cl, e, arena);
  return hipGetLastError();
}

namespace {
struct RowArrays {  // what DecodeRows points at, per row
  unsigned long long *row_begin;
  unsigned *row_cnt;
  float *row_scale;
  long long *row_raw;
  unsigned long long *row_raw_len;
  void take(Carve &c, uint64_t m) {
    row_begin = c.take<unsigned long long>(m);
    row_cnt = c.take<unsigned>(m);
    row_scale = c.take<float>(m);
    row_raw = c.take<long long>(m);
    row_raw_len = c.take<unsigned long long>(m);
  }
  DecodeRows rows(const void *pairs, const void *raw_pool) const {
    // any_raw: the host does not know, so the raw-row kernel is always launched (it returns at once for
    // the rows of compressed frames)
    return DecodeRows{static_cast<const uint32_t *>(pairs), reinterpret_cast<const uint64_t *>(row_begin), row_cnt, row_scale,
                      reinterpret_cast<const int64_t *>(row_raw), reinterpret_cast<const uint64_t *>(row_raw_len),
                      static_cast<const int16_t *>(raw_pool), 1u};
  }
};
struct R1Tables : RowArrays {  // the fixed-stride lists in front of the row arrays
  unsigned *pairs;
  uint64_t bytes;
};
R1Tables r1_tables(const void *base, uint32_t M) {
  const uint64_t m = M ? M : 1;
  Carve c{reinterpret_cast<uintptr_t>(base)};
  R1Tables t;
  t.pairs = c.take<unsigned>(m * kHopI);
  t.take(c, m);
  t.bytes = c.used;
  return t;
}
struct R2Tables : RowArrays {  // the row arrays (32 B per row), the block sums behind them
  unsigned long long *blk, *blk_raw;
  uint64_t bytes;
};
R2Tables r2_tables(const void *base, uint32_t M) {
  const uint64_t m = M ? M : 1, nblk = (m + 1023) / 1024;
  Carve c{reinterpret_cast<uintptr_t>(base)};
  R2Tables t;
  t.take(c, m);
  t.blk = c.take<unsigned long long>(nblk);
  t.blk_raw = c.take<unsigned long long>(nblk);
  t.bytes = c.used;
  return t;
}
}  // namespace

uint64_t rows_from_records_bytes(uint32_t M) { return r1_tables(nullptr, M).bytes; }

namespace {
hipError_t rows_from_records(const uint8_t *records, uint32_t M, uint32_t ch, const FrameMap *fmap, void *workspace,
                             uint64_t *stats, hipStream_t s, DecodeRows *rows) {
  if (!records || !workspace || !rows || ch == 0 || (reinterpret_cast<uintptr_t>(records) & 15u)) return hipErrorInvalidValue;
  const R1Tables t = r1_tables(workspace, M);
  *rows = t.rows(t.pairs, records);
  if (M == 0) return hipSuccess;
  const unsigned long long rec = record_bytes(ch), hdr = record_header_bytes(ch);
  auto *st = reinterpret_cast<unsigned long long *>(stats);
  if (fmap)
    hipLaunchKernelGGL(k_rows_from_records<true>, dim3((M + 3) / 4), dim3(256), 0, s, records, M, ch, rec, hdr, t.pairs, t.row_begin,
                       t.row_cnt, t.row_scale, t.row_raw, t.row_raw_len, st, reinterpret_cast<const uint2 *>(fmap));
  else
    hipLaunchKernelGGL(k_rows_from_records<false>, dim3((M + 3) / 4), dim3(256), 0, s, records, M, ch, rec, hdr, t.pairs, t.row_begin,
                       t.row_cnt, t.row_scale, t.row_raw, t.row_raw_len, st, static_cast<const uint2 *>(nullptr));
  return hipGetLastError();
}
}  // namespace

hipError_t launch_rows_from_records(const uint8_t *records, uint32_t M, uint32_t ch, void *workspace, uint64_t *stats,
                                    hipStream_t s, DecodeRows *rows) {
  return rows_from_records(records, M, ch, nullptr, workspace, stats, s, rows);
}

hipError_t launch_rows_from_records_batch(const uint8_t *records, uint32_t M, uint32_t ch, const FrameMap *fmap, void *workspace,
                                          uint64_t *clip_stats, hipStream_t s, DecodeRows *rows) {
  if (!fmap || !clip_stats) return hipErrorInvalidValue;
  return rows_from_records(records, M, ch, fmap, workspace, clip_stats, s, rows);
}

uint64_t rows_from_compact_bytes(uint32_t M) { return r2_tables(nullptr, M).bytes; }

hipError_t launch_rows_from_compact(const CompactBlob *dir, const CompactBlob &one, uint32_t n_entries, uint32_t M, uint32_t ch,
                                    const R2Mode &mode, const void *base, void *workspace, CompactStatus *status, hipStream_t s,
                                    DecodeRows *rows) {
  static_assert(sizeof(CompactBlob) == 32 && sizeof(CompactStatus) == 64, "read and written by the kernels as laid out here");
  if (!workspace || !status || !rows || !base || ch == 0 || n_entries == 0 || (!dir && n_entries != 1)) return hipErrorInvalidValue;
  // whole frames; every window has some; whole blobs have nothing in front (a directory's entries: the caller's word)
  if (M % ch || (M == 0 && !mode.totals) || (mode.totals && mode.max_front)) return hipErrorInvalidValue;
  if (!dir && ((one.addr & 63u) || one.first_row != 0 || one.win[1] != M || one.rows % ch || one.win[0] % ch ||
               one.win[0] > one.rows || M > one.rows - one.win[0] || one.win[0] > mode.max_front ||
               (mode.totals && one.rows != M) || one.addr < reinterpret_cast<uintptr_t>(base)))
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(base) & 63u) return hipErrorInvalidValue;
  const R2Tables t = r2_tables(workspace, M);
  const unsigned nblk = static_cast<unsigned>((static_cast<uint64_t>(M) + 1023) / 1024);
  *rows = t.rows(base, base);
  hipLaunchKernelGGL(k_r2_headers, dim3((n_entries + 255) / 256), dim3(256), 0, s, dir, one, n_entries, ch, status, mode.verdict);
  if (M == 0) return hipGetLastError();
  if (mode.max_front) {
    const unsigned chunks = static_cast<unsigned>((static_cast<uint64_t>(mode.max_front) + kR2wPrefixRows - 1) / kR2wPrefixRows);
    for (uint32_t b0 = 0; b0 < n_entries; b0 += 65535u)  // blockIdx.y is 16 bits wide
      hipLaunchKernelGGL(k_r2w_prefix, dim3(chunks, std::min(n_entries - b0, 65535u)), dim3(256), 0, s, dir, one, b0, ch, status);
  }
  const auto scan_rows = mode.totals ? k_r2_scan_rows<false> : k_r2_scan_rows<true>;
  const auto scan_blocks = mode.totals ? k_r2_scan_blocks<true> : k_r2_scan_blocks<false>;
  const auto table_rows = mode.totals ? k_r2_rows<false> : k_r2_rows<true>;
  hipLaunchKernelGGL(scan_rows, dim3(nblk), dim3(256), 0, s, dir, one, n_entries, M, ch, status, t.row_raw_len, t.blk, t.blk_raw);
  hipLaunchKernelGGL(scan_blocks, dim3(1), dim3(1024), 0, s, dir, one, n_entries, M, t.blk, t.blk_raw, nblk, t.row_raw_len, status);
  hipLaunchKernelGGL(table_rows, dim3(static_cast<unsigned>((static_cast<uint64_t>(M) + 3) / 4)), dim3(256), 0, s, dir, one, n_entries,
                     M, ch, static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(base)), t.blk, t.blk_raw, status, t.row_begin,
                     t.row_cnt, t.row_scale, t.row_raw, t.row_raw_len);
  return hipGetLastError();
}

hipError_t launch_store_plan_crops(const StoreDraw &a, hipStream_t s) {
  static_assert(sizeof(glc_store_entry) == 32 && sizeof(HopDescStrided) == 40, "read and written by the planner as laid out here");
  if (a.n_crops == 0) return hipSuccess;
  if (!a.entries || !a.lengths || !a.clips || !a.starts || !a.dir || !a.desc || !a.verdict || a.ch == 0 || a.ch > 65535u ||
      a.max_hops == 0 || a.per_round == 0 || a.length == 0 || a.n_entries == 0)
    return hipErrorInvalidValue;
  // descriptors per crop: the fixed draw's are its hops, one fewer than its frames; a ragged crop may need one more
  if (a.max_frames != a.max_hops + 1 && !(a.ragged && a.max_frames == a.max_hops)) return hipErrorInvalidValue;
  const uint64_t threads = a.n_crops * a.max_hops, blocks = (threads + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const auto planner = a.ragged ? k_store_plan_crops<true> : k_store_plan_crops<false>;
  hipLaunchKernelGGL(planner, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_dec_plan(uint64_t arena, uint64_t arena_bytes, const glc_store_entry *entries, const StreamDecSeg *segs,
                                  uint32_t n_segs, CompactBlob *dir, uint32_t *verdict, hipStream_t s) {
  if (n_segs == 0) return hipSuccess;
  if (!entries || !segs || !dir || !verdict || (arena & 63u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_stream_dec_plan, dim3((n_segs + 255u) / 256u), dim3(256), 0, s, arena, arena_bytes, entries, segs, n_segs, dir,
                     verdict);
  return hipGetLastError();
}

hipError_t launch_stream_dec_carry(bool save, const StreamCarry *desc, uint32_t n_desc, uint32_t ch, float *blocks, float *carry,
                                   hipStream_t s) {
  if (n_desc == 0) return hipSuccess;
  if (!desc || !blocks || !carry || ch == 0 || ch > 32767u) return hipErrorInvalidValue;
  for (uint32_t d0 = 0; d0 < n_desc; d0 += 65535u) {  // blockIdx.y is 16 bits wide
    const dim3 grid(2u * ch, std::min(n_desc - d0, 65535u));
    if (save) hipLaunchKernelGGL(k_stream_dec_carry<true>, grid, dim3(256), 0, s, desc + d0, ch, blocks, carry);
    else hipLaunchKernelGGL(k_stream_dec_carry<false>, grid, dim3(256), 0, s, desc + d0, ch, blocks, carry);
  }
  return hipGetLastError();
}

hipError_t launch_store_evict_scan(const StoreEvict &a, hipStream_t s) {
  if (!a.entries || !a.keep || !a.entries_out || !a.new_index || !a.n_out || !a.cursor || !a.ws || a.n_entries == 0 ||
      (a.lengths == nullptr) != (a.lengths_out == nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_store_evict_scan, dim3(1), dim3(1024), 0, s, a);
  const uint64_t blocks = (a.n_entries + 255) / 256;
  hipLaunchKernelGGL(k_store_evict_tail, dim3(static_cast<unsigned>(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_store_evict_gather(const uint64_t *ws, const void *arena, uint64_t arena_bytes, void *dst, hipStream_t s) {
  if (!ws || !arena || !dst) return hipErrorInvalidValue;
  if (arena_bytes == 0) return hipSuccess;  // nothing is usable in an empty arena
  const uint64_t tiles = (arena_bytes + kStoreMoveTile - 1) / kStoreMoveTile;
  hipLaunchKernelGGL(k_store_evict_gather, dim3(static_cast<unsigned>(tiles < kStoreMoveGrid ? tiles : kStoreMoveGrid)), dim3(256), 0, s,
                     reinterpret_cast<const unsigned long long *>(ws), static_cast<const unsigned char *>(arena),
                     static_cast<unsigned char *>(dst));
  return hipGetLastError();
}

hipError_t launch_store_join_plan(const StoreJoin &a, hipStream_t s) {
  if (a.n_segs == 0 || a.n_clips == 0) return hipSuccess;
  (void)hipGetLastError();
  constexpr uint64_t kMaxGrid = 1ull << 20;  // segments behind it are taken by the grid stride
  hipLaunchKernelGGL(k_store_join_plan, dim3(static_cast<unsigned>(a.n_segs < kMaxGrid ? a.n_segs : kMaxGrid)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_store_join_scan, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_store_join_move(const StoreJoin &a, uint64_t max_bytes, hipStream_t s) {
  const uint64_t tiles = (max_bytes + kStoreMoveTile - 1) / kStoreMoveTile;
  if (a.n_segs == 0 || a.n_clips == 0 || tiles == 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_store_join_move, dim3(static_cast<unsigned>(tiles < kStoreMoveGrid ? tiles : kStoreMoveGrid)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_store_cut_plan(const StoreCut &a, hipStream_t s) {
  if (a.n_cuts == 0) return hipSuccess;
  (void)hipGetLastError();
  constexpr uint64_t kMaxGrid = 1ull << 20;  // cuts behind it are taken by the grid stride
  hipLaunchKernelGGL(k_store_cut_plan, dim3(static_cast<unsigned>(a.n_cuts < kMaxGrid ? a.n_cuts : kMaxGrid)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_store_cut_scan, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_store_cut_move(const StoreCut &a, uint64_t max_bytes, hipStream_t s) {
  const uint64_t tiles = (max_bytes + kStoreMoveTile - 1) / kStoreMoveTile;
  if (a.n_cuts == 0 || tiles == 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_store_cut_move, dim3(static_cast<unsigned>(tiles < kStoreMoveGrid ? tiles : kStoreMoveGrid)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_store_evict_round(const uint64_t *ws, void *arena, void *stage, uint64_t round, uint64_t r, hipStream_t s) {
  if (!ws || !arena || !stage || round == 0 || (round & 63ull) || round > (1ull << 40)) return hipErrorInvalidValue;
  const uint64_t tiles = (round + kStoreMoveTile - 1) / kStoreMoveTile;
  hipLaunchKernelGGL(k_store_evict_round, dim3(static_cast<unsigned>(2 * tiles < kStoreMoveGrid ? 2 * tiles : kStoreMoveGrid)), dim3(256),
                     0, s, reinterpret_cast<const unsigned long long *>(ws), static_cast<unsigned char *>(arena),
                     static_cast<unsigned char *>(stage), static_cast<unsigned long long>(round), static_cast<unsigned long long>(r),
                     static_cast<unsigned>(tiles));
  return hipGetLastError();
}

uint64_t imdct_plan_bytes(uint32_t groups) {
  // headers | records | work keys | unit order
  return static_cast<uint64_t>(groups) * (4ull * kPlanHdrDwords + static_cast<uint64_t>(kPlanRecCap) * kPlanRecDwords * 4ull + 8ull);
}

hipError_t launch_imdct_rows(const DeviceTables &t, const DecodeRows &rows, uint32_t row_begin,
                             uint32_t M, uint32_t ch, float *blocks, hipStream_t s, int variant, void *plan,
                             uint32_t plan_groups, bool reuse_plan) {
  if (M == 0) return hipSuccess;
  // every caller decodes whole frames; the one-row kernel is the cross-check variant (glc_debug.h)
  if (variant == 1 || ch == 0 || M % ch != 0) {
    hipLaunchKernelGGL(k_imdct_rows, dim3(M), dim3(256), 0, s, t, rows, row_begin, M, ch, blocks);
    return hipGetLastError();
  }
  if (!plan || plan_groups < ch) return hipErrorInvalidValue;
  const uint32_t n_frames = M / ch;
  const uint32_t groups = (n_frames + 7) / 8;
  // plan + apply, in batches of whole frame groups (x all channels) through one workspace of
  // plan_groups (frame group, channel) units
  unsigned *hdr = static_cast<unsigned *>(plan);
  unsigned *rec = hdr + static_cast<size_t>(plan_groups) * kPlanHdrDwords;
  unsigned *work = rec + static_cast<size_t>(plan_groups) * kPlanRecCap * kPlanRecDwords;
  unsigned *order = work + plan_groups;
  const uint32_t fg_per_batch = plan_groups / ch;
  if (reuse_plan && groups > fg_per_batch) return hipErrorInvalidValue;  // only a one-batch launch leaves its plan behind
  if (rows.any_raw) hipLaunchKernelGGL(k_imdct_raw_rows, dim3(M), dim3(256), 0, s, rows, row_begin, M, ch, blocks);
  for (uint32_t fg0 = 0; fg0 < groups; fg0 += fg_per_batch) {
    const uint32_t n_fg = groups - fg0 < fg_per_batch ? groups - fg0 : fg_per_batch;
    const uint32_t n_units = n_fg * ch;
    const dim3 grid(n_units);
    // more units than CUs: rank them by work (fewer land one per CU whatever the order)
    const bool ranked = n_units > 256 && n_units <= kOrderMaxUnits;
    if (!reuse_plan) {
      hipLaunchKernelGGL(k_imdct_plan, grid, dim3(256), 0, s, rows, row_begin, n_frames, ch, fg0, 2u, hdr, rec, work);
      const unsigned neighbours = variant == 5 && n_units % 256 == 0 && n_units % ch == 0 ? 1u : 0u;
      if (ranked && variant != 6)
        hipLaunchKernelGGL(k_imdct_order, dim3((n_units + 3) / 4), dim3(256), 0, s, work, n_units, order, ch, neighbours);
    }
    const unsigned *ord = ranked && variant != 6 ? order : nullptr;
    if (variant == 2)
      hipLaunchKernelGGL(k_imdct_apply<false>, grid, dim3(256), 0, s, t, hdr, rec, ord, n_frames, ch, fg0, n_units, blocks);
    else if (variant == 4)
      hipLaunchKernelGGL((k_imdct_apply<true, true, false>), grid, dim3(256), 0, s, t, hdr, rec, ord, n_frames, ch, fg0, n_units, blocks);
    else if (variant == 3)
      hipLaunchKernelGGL((k_imdct_apply<true, false>), grid, dim3(256), 0, s, t, hdr, rec, ord, n_frames, ch, fg0, n_units, blocks);
    else
      hipLaunchKernelGGL(k_imdct_apply<true>, grid, dim3(256), 0, s, t, hdr, rec, ord, n_frames, ch, fg0, n_units, blocks);
  }
  return hipGetLastError();
}

namespace {
// What the D2 launchers share.  blockIdx.y is 16 bits wide: rows (hops or descriptors) [0, n) go out in slabs
// of 32768, launch(first row, rows).  (Every decode driver stays far below: rounds of <= 4097 hops.)
template <typename F>
void d2_slabs(uint64_t n, F &&launch) {
  for (uint64_t r0 = 0; r0 < n; r0 += 32768) launch(r0, static_cast<unsigned>(std::min<uint64_t>(n - r0, 32768)));
}
// (... and by_channels, at the top of the file, for the instantiation by channel count)
inline unsigned d2_blocks_x(uint32_t ch) { return (1024u * ch / 4u + 255u) / 256u; }  // 4-sample chunks of a hop over 256 threads

template <typename T>
hipError_t overlap_add_typed(const float *blocks, int64_t blk_frame0, uint64_t n_frames, uint32_t ch, uint64_t hop_begin,
                             uint64_t hop_end, T *out, hipStream_t s) {
  if (hop_end <= hop_begin) return hipSuccess;
  const unsigned per_hop = 1024u * ch;
  d2_slabs(hop_end - hop_begin, [&](uint64_t r0, unsigned nh) {
    const dim3 grid(d2_blocks_x(ch), nh);
    T *o = out + r0 * per_hop;
    const long long f0 = static_cast<long long>(blk_frame0);
    const unsigned long long nf = n_frames, hb = hop_begin + r0;
    if (reinterpret_cast<uintptr_t>(o) & (4u * sizeof(T) - 1u)) {  // not aligned to a float4 / short4
      hipLaunchKernelGGL((k_overlap_add<0, false, T>), grid, dim3(256), 0, s, blocks, f0, nf, ch, hb, o);
      return;
    }
    by_channels(ch, [&](auto CH) {
      hipLaunchKernelGGL((k_overlap_add<decltype(CH)::value, true, T>), grid, dim3(256), 0, s, blocks, f0, nf, ch, hb, o);
    });
  });
  return hipGetLastError();
}
}  // namespace

hipError_t launch_overlap_add(const float *blocks, int64_t blk_frame0, uint64_t n_frames, uint32_t ch,
                              uint64_t hop_begin, uint64_t hop_end, float *out, hipStream_t s) {
  return overlap_add_typed(blocks, blk_frame0, n_frames, ch, hop_begin, hop_end, out, s);
}

hipError_t launch_overlap_add(const float *blocks, int64_t blk_frame0, uint64_t n_frames, uint32_t ch,
                              uint64_t hop_begin, uint64_t hop_end, int16_t *out, hipStream_t s) {
  return overlap_add_typed(blocks, blk_frame0, n_frames, ch, hop_begin, hop_end, reinterpret_cast<short *>(out), s);
}

namespace {
template <typename S>
hipError_t stage_clips_typed(const S *src, const StageClip *clips, uint32_t n_clips, uint32_t ch, bool planar, uint64_t channel_stride,
                             uint32_t n_virtual_frames, float inv, float *vstream, hipStream_t s) {
  if (!src || !clips || !vstream || n_clips == 0 || ch == 0 || (reinterpret_cast<uintptr_t>(vstream) & 15u) ||
      (reinterpret_cast<uintptr_t>(src) & (sizeof(S) - 1u)))
    return hipErrorInvalidValue;
  if (n_virtual_frames == 0) return hipSuccess;
  const unsigned long long cs = channel_stride;
  const dim3 wide(n_virtual_frames, ch), one(n_virtual_frames);  // 1024 * ch / 4 float4 over 256 threads: ch workgroups per slot
  if (ch > 65535u) return hipErrorInvalidValue;
  if (!planar || ch == 1) {
    hipLaunchKernelGGL(k_stage_clips<S>, wide, dim3(256), 0, s, src, clips, n_clips, ch, inv, vstream);
  } else {
    switch (ch) {
      case 2: hipLaunchKernelGGL((k_stage_clips_planar<2, S>), one, dim3(256), 0, s, src, clips, n_clips, cs, inv, vstream); break;
      case 4: hipLaunchKernelGGL((k_stage_clips_planar<4, S>), one, dim3(256), 0, s, src, clips, n_clips, cs, inv, vstream); break;
      case 8: hipLaunchKernelGGL((k_stage_clips_planar<8, S>), one, dim3(256), 0, s, src, clips, n_clips, cs, inv, vstream); break;
      default: hipLaunchKernelGGL(k_stage_clips_planar_any<S>, wide, dim3(256), 0, s, src, clips, n_clips, ch, cs, inv, vstream); break;
    }
  }
  return hipGetLastError();
}

// `(1 << (bits - 1)) as f32` on an i32 literal: 32 bits shift into the sign (quirk Q11, glc_wav.cpp).  A power of
// two, so its reciprocal is exact.
float pcm_widen_inv(uint32_t bits) {
  const float max = bits == 32 ? -2147483648.0f : static_cast<float>(1u << (bits - 1));
  return 1.0f / max;
}
}  // namespace

hipError_t launch_stage_clips(const float *src, const StageClip *clips, uint32_t n_clips, uint32_t ch, bool planar,
                              uint64_t channel_stride, uint32_t n_virtual_frames, float *vstream, hipStream_t s) {
  return stage_clips_typed(src, clips, n_clips, ch, planar, channel_stride, n_virtual_frames, 1.0f, vstream, s);
}

hipError_t launch_stage_clips_int(const void *src, bool wide, uint32_t bits, const StageClip *clips, uint32_t n_clips, uint32_t ch,
                                  bool planar, uint64_t channel_stride, uint32_t n_virtual_frames, float *vstream, hipStream_t s) {
  if (bits == 0 || bits > (wide ? 32u : 16u)) return hipErrorInvalidValue;
  const float inv = pcm_widen_inv(bits);
  return wide ? stage_clips_typed(static_cast<const int *>(src), clips, n_clips, ch, planar, channel_stride, n_virtual_frames, inv, vstream, s)
              : stage_clips_typed(static_cast<const short *>(src), clips, n_clips, ch, planar, channel_stride, n_virtual_frames, inv, vstream, s);
}

namespace {
template <typename S>
hipError_t stage_segments_typed(const S *src, const StreamSpan *spans, uint32_t n_spans, uint32_t vs_units, uint32_t held_units,
                                uint32_t ch, bool planar, uint64_t channel_stride, float inv, float *held, float *vstream, hipStream_t s) {
  if (!spans || !held || n_spans == 0 || ch == 0 || ch > 65535u || (vs_units && !vstream) || vs_units == 1 ||
      ((reinterpret_cast<uintptr_t>(vstream) | reinterpret_cast<uintptr_t>(held)) & 15u) ||
      (reinterpret_cast<uintptr_t>(src) & (sizeof(S) - 1u)))
    return hipErrorInvalidValue;
  if (vs_units + held_units == 0) return hipSuccess;
  // 512 * ch / 4 float4 over 256 threads: ceil(ch / 2) workgroups per unit
  hipLaunchKernelGGL(k_stage_segments<S>, dim3(vs_units + held_units, (ch + 1u) / 2u), dim3(256), 0, s, src, spans, n_spans, vs_units,
                     ch, planar && ch > 1 ? 1u : 0u, static_cast<unsigned long long>(channel_stride), inv, held, vstream);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_stage_segments(const void *src, glc_pcm_format fmt, uint32_t bits, const StreamSpan *spans, uint32_t n_spans,
                                 uint32_t vs_units, uint32_t held_units, uint32_t ch, bool planar, uint64_t channel_stride,
                                 float *held, float *vstream, hipStream_t s) {
  if (fmt == GLC_PCM_F32)
    return stage_segments_typed(static_cast<const float *>(src), spans, n_spans, vs_units, held_units, ch, planar, channel_stride, 1.0f,
                                held, vstream, s);
  const bool wide = fmt == GLC_PCM_S32;
  if ((!wide && fmt != GLC_PCM_S16) || bits == 0 || bits > (wide ? 32u : 16u)) return hipErrorInvalidValue;
  const float inv = pcm_widen_inv(bits);
  return wide ? stage_segments_typed(static_cast<const int *>(src), spans, n_spans, vs_units, held_units, ch, planar, channel_stride, inv,
                                     held, vstream, s)
              : stage_segments_typed(static_cast<const short *>(src), spans, n_spans, vs_units, held_units, ch, planar, channel_stride, inv,
                                     held, vstream, s);
}

namespace {
template <typename T, typename D>
hipError_t overlap_add_strided_typed(const float *blocks, const D *desc, uint32_t n_desc, uint32_t ch, bool planar, T *out,
                                     hipStream_t s) {
  if (n_desc == 0) return hipSuccess;
  if (!blocks || !desc || !out || ch == 0 || (reinterpret_cast<uintptr_t>(out) & (sizeof(T) - 1u))) return hipErrorInvalidValue;
  d2_slabs(n_desc, [&](uint64_t d0, unsigned nd) {
    const D *d = desc + d0;
    if constexpr (std::is_same<D, HopDescStrided>::value) {  // (a HopDesc has no planes)
      if (planar && ch > 1) {
        hipLaunchKernelGGL(k_overlap_add_planar<T>, dim3(ch, nd), dim3(256), 0, s, blocks, d, ch, out);
        return;
      }
    }
    // (a span that starts off a chunk boundary has one chunk more: the kernel's stride loop takes it)
    const dim3 grid(d2_blocks_x(ch), nd);
    by_channels(ch, [&](auto CH) {
      hipLaunchKernelGGL((k_overlap_add_strided<decltype(CH)::value, T, D>), grid, dim3(256), 0, s, blocks, d, ch, out);
    });
  });
  return hipGetLastError();
}
}  // namespace

hipError_t launch_overlap_add_strided(const float *blocks, const HopDescStrided *desc, uint32_t n_desc, uint32_t ch, bool planar,
                                      float *out, hipStream_t s) {
  return overlap_add_strided_typed(blocks, desc, n_desc, ch, planar, out, s);
}

hipError_t launch_overlap_add_strided(const float *blocks, const HopDescStrided *desc, uint32_t n_desc, uint32_t ch, bool planar,
                                      int16_t *out, hipStream_t s) {
  return overlap_add_strided_typed(blocks, desc, n_desc, ch, planar, reinterpret_cast<short *>(out), s);
}

hipError_t launch_overlap_add_strided(const float *blocks, const HopDesc *desc, uint32_t n_desc, uint32_t ch, float *out,
                                      hipStream_t s) {
  return overlap_add_strided_typed(blocks, desc, n_desc, ch, false, out, s);
}

hipError_t launch_overlap_add_strided(const float *blocks, const HopDesc *desc, uint32_t n_desc, uint32_t ch, int16_t *out,
                                      hipStream_t s) {
  return overlap_add_strided_typed(blocks, desc, n_desc, ch, false, reinterpret_cast<short *>(out), s);
}

namespace {
template <typename S>
hipError_t widen_typed(const S *in, uint64_t n, float inv, float *out, hipStream_t s) {
  // body from the first 16-byte aligned destination element; the source is vector-loaded if it is
  // aligned to four of its samples there
  const unsigned long long head = std::min<uint64_t>(n, (16u - (reinterpret_cast<uintptr_t>(out) & 15u)) / 4u % 4u);
  const bool vec = (reinterpret_cast<uintptr_t>(in + head) & (4u * sizeof(S) - 1u)) == 0;
  const uint64_t threads = (n - head) / 4u + head + (n - head) % 4u;  // n <= 2^30 (launch_pcm_widen)
  const dim3 grid(static_cast<unsigned>((threads + 255u) / 256u));
  if (vec) hipLaunchKernelGGL((k_pcm_widen<S, true>), grid, dim3(256), 0, s, in, out, n, static_cast<unsigned>(head), inv);
  else hipLaunchKernelGGL((k_pcm_widen<S, false>), grid, dim3(256), 0, s, in, out, n, static_cast<unsigned>(head), inv);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_pcm_widen(const void *in, bool wide, uint32_t bits, uint64_t n, float *out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const float inv = pcm_widen_inv(bits);
  constexpr uint64_t kPiece = uint64_t{1} << 30;  // samples per launch: the grid stays far below its limit
  for (uint64_t at = 0; at < n; at += kPiece) {
    const uint64_t m = std::min(kPiece, n - at);
    const hipError_t e = wide ? widen_typed(static_cast<const int32_t *>(in) + at, m, inv, out + at, s)
                              : widen_typed(static_cast<const int16_t *>(in) + at, m, inv, out + at, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace glc
