// glc_kernels.h — launch interface of the gfx950 kernels (implemented in glc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glc_common.h"

namespace glc {

// Device-resident constant tables of one context.
struct DeviceTables {
  const float *cos_t;      // [2048][1024]  T transposed (row i): forward MDCT operand
  const float *cos;        // [1024][2048]  T (row k): inverse MDCT operand
  const float *window;     // [2048]
  const float *indiv;      // [1024] 1/weights[k].max(0.1)
  const float *band_pf;    // [n_bands]
  const float *band_len;   // [n_bands]
  const uint16_t *band_of; // [1024]
  const uint32_t *edges;   // [n_bands+1]
  uint32_t n_bands;
  float norm, cf, noise_floor;
  const uint16_t *cos_bf;  // bf16 pieces of T[k][i], k >= C0, in fragment order (MatrixBound below); null where not built
};

// The matrix form of the screened transform (glc_mdct_fwd.hpp k_mdct_mx_st): the bound sums e_k of
// the columns k >= C0 on the bf16 matrix pipe.  Each f32 operand is split a = a1 + a2 + r, a1 = bf16_rn(a), a2 =
// bf16_rn(a - a1); e_k sums the kProducts piece products a1 t1 + a1 t2 + a2 t1 with one v_mfma_f32_32x32x16_bf16 per
// product and K-block of kKBlock i-steps.  A chain of accumulating instructions is cut every kSegBlocks K-blocks: the
// segment's accumulator is added to a per-output f32 total and cleared.  The error budget, per unit of A = sum |xw|:
//   split         kSplitEps = 3 * 2^-16 (+ O(2^-24)): the dropped a2 t2 + r_a t + a r_t, |T| <= 1
//   accumulation  kSegBlocks * kProducts instructions per chain, each within kKappa (|C| + sum |p|), kKappa = 17 * 2^-23
//                 (any f32 summation of 16 products and C, rounding or truncating, in any order)
//   totals        kSegments f32 adds, 2^-24 each
// and the sum must stay within gamma_2048 = 2048 u / (1 - 2048 u), the half of kScreenCErr that belongs to e_k.
struct MatrixBound {
  static constexpr int kNe = 6;                    // the form is built for C0 = 384 (44.1 and 48 kHz)
  static constexpr int kPieces = 2;                // bf16 pieces kept per operand
  static constexpr int kProducts = 3;              // piece products summed
  static constexpr int kKBlock = 16;               // i-steps per instruction
  static constexpr int kSegBlocks = 8;             // K-blocks per accumulation segment
  static constexpr int kSegments = 2048 / (kKBlock * kSegBlocks);
  static constexpr int kRows = 128;                // rows per workgroup
  static constexpr int kGroups = 4;                // workgroups per row tile = hf planes of a launch
  static constexpr int kTile = 32;                 // bound columns per fragment
  static constexpr double kKappa = 17.0 / 8388608.0;
  static constexpr double kSplitEps = 3.0 / 65536.0;
  static constexpr double kGamma = 2048.0 / 16777216.0 / (1.0 - 2048.0 / 16777216.0);
  static constexpr double kBudget = kSplitEps + kSegBlocks * kProducts * kKappa + kSegments / 16777216.0;
  static_assert(kBudget <= kGamma, "the matrix form's e_k must stay within gamma_2048 A of the real sum");
};
// bytes of the fragment-ordered table image for a last band that starts at column c0 (a multiple of 64)
inline uint64_t matrix_bound_table_bytes(uint32_t c0) { return 128ull * ((1024u - c0) / 32u) * 2ull * 64ull * 16ull; }

// View of interleaved PCM on the device (whole stream or a shard with halo).
struct PcmView {
  const float *p;      // element (t0*ch) of the stream
  uint64_t t0;         // first per-channel sample index present
  uint64_t t_count;    // per-channel samples present
  uint64_t n_samples;  // interleaved length of the WHOLE stream
  uint32_t ch;
};

// K1: windowed forward MDCT of rows [0, M) (row = (frame - frame_begin)*ch + c) -> coef[M][1024].
hipError_t launch_mdct_forward(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin,
                               uint32_t M, float *coef, hipStream_t s, int variant = 0, bool beside = false);
// K2: scale, masking thresholds, quantiser -> record header {scale,nnz} + dense i16 row.  For 1 / 2 /
// 4 channels the kernel also takes the raw-vs-compressed decision and writes the raw plane of raw
// frames (*decided = true: do not launch K3); `pcm` / `frame_begin` are what that needs.
hipError_t launch_quantize(const DeviceTables &t, const float *coef, uint32_t M, uint32_t ch, const PcmView &pcm,
                           uint64_t frame_begin, uint8_t *records, hipStream_t s, bool *decided);
// K1 + K2 of a launch whose records, row by row, provably do not depend on the last band (the screen, DESIGN
// section 2): the mixed-role transform (exact below C0, a fused-multiply-add bound above), the quantiser on the
// rows that pass, then the repair - exact columns C0.. and today's quantiser for the rows that failed.  Same
// record bytes as launch_mdct_forward + launch_quantize for every input; *decided as launch_quantize.
// The repair's transform is one of two kernels, chosen by the caller per launch (`latency_repair`); both write the
// same coefficients for every input, so the records never depend on the choice:
//   false  k_mdct_fwd_small_cols: the 2 x 2 short-clip kernel over the columns C0.., one workgroup per (tile of 32
//          rows, 32 columns) that leaves unless the tile holds a failed row - a throughput kernel: many failed rows
//          share its table tiles, and a launch costs its LDS-staged chain (55 us) however few rows failed
//   true   k_mdct_fwd_small_rows: one wave per (two failed rows, 64 columns), found from the quantiser's per-wave fail
//          counts on a fixed grid; the rows in LDS, the table streamed 112 i-steps ahead - a latency kernel: a
//          handful of failed rows cost one wave's chain of 2048 dependent adds, a long list costs a chain per
//          kRowsGrid items
struct ScreenShape {
  uint32_t l0, c0, ne;  // start of the last band, l0 rounded up to 64, c0 / 64
  uint32_t hp;          // exact column pairs of the transform's hybrid waves (0: none - waves [0, ne) are exact)
  uint32_t n_planes;    // hf planes of a launch: one per wave that carries bound columns (the A plane follows them)
};
bool encode_screen_shape(const uint32_t *edges, uint32_t n_bands, ScreenShape *sh);  // false: c0 / 64 outside 1..15
// true where launch_mdct_forward gives the launch to the 16-wave k_mdct_fwd_st, the form the mixed-role kernel has
bool mdct_forward_is_st16(uint32_t M, uint32_t ch, int variant);
bool mdct_forward_has_segment_loader(uint32_t ch);
uint64_t encode_screen_bytes(uint32_t M, const ScreenShape &sh);
// workspace: encode_screen_bytes(M) bytes, 16-byte aligned, nothing in it needs initialising.  host_stat: 8
// device-visible host words {failed rows, rows, seq, -, u64 failed rows so far, ...} the last launch writes; they count
// the serial repair's rows, the edge rows that failed go to EdgeLaunch::failed_total alone.
// The edge path: the frames whose window reaches into the stream's zero padding (edge_frames below) fail the screen
// on any content that is not silent there, and which they are is known before anything is launched.  With `edge`
// given, their exact coefficients (k_mdct_edge_rows, the repair's chain with the row list taken from the kernel
// arguments, all 1024 columns into edge->coef) and their records (k_quantize_screen<*, 3>) are queued on edge->side
// beside K1 and K2, depending on nothing either writes; K2 evaluates their screen but neither writes nor lists them,
// the serial repair is left the rows nobody could predict, and the caller's stream continues only behind the side
// stream's last launch.  Same record bytes with or without it.
struct EdgeLaunch {
  uint64_t a, b;                // edge_frames of the stream, absolute frame numbers
  hipStream_t side;             // not the launch's stream
  hipEvent_t ev_fork, ev_edge;  // this launch's own until its stream has passed the join
  float *coef;                  // [kEdgeRowsMax][1024], this launch's own for as long
  bool capped;                  // the transform with the short table ring and a register cap (k_mdct_edge_rows_capped: fits beside
                                // two resident workgroups of K2 on a CU) instead of the latency form; same bytes
  unsigned long long *failed_total;  // device: the edge rows that failed the screen so far; the repair quantiser adds this launch's
};
// What a screened launch is given besides its rows (the comments above say what each is).
struct ScreenLaunch {
  void *workspace;
  uint32_t *host_stat;
  uint32_t seq;
  uint8_t *records;
  hipStream_t s;
  bool latency_repair, matrix_bound;
  const EdgeLaunch *edge;  // null: no edge path
};
hipError_t launch_encode_screened(const DeviceTables &t, const ScreenShape &sh, const PcmView &pcm, uint64_t frame_begin,
                                  uint32_t M, float *coef, const ScreenLaunch &launch, bool *decided);

// The ONE definition of an edge frame: frame f reads per-channel samples [hop f - hop/2, hop f - hop/2 + frame); it
// is an edge frame if that window is not wholly inside the stream [0, per_channel) of plan_encode.  Edge frames are
// the prefix [0, a) and the suffix [b, n_frames) of the stream's frames (a <= b; a shard's halo is not padding).
struct EdgeFrames {
  uint64_t a, b;
};
GLC_HD inline EdgeFrames edge_frames(uint64_t per_channel, uint64_t n_frames) {
  const uint64_t tail = kFrame - kHop / 2;  // a frame's window ends at hop f + tail
  uint64_t a = n_frames < 1 ? n_frames : 1;  // frame 0 starts hop / 2 before the stream, frame 1 inside it
  uint64_t b = per_channel >= tail ? (per_channel - tail) / kHop + 1 : 0;  // the first f with hop f + tail > per_channel
  if (b > n_frames) b = n_frames;
  if (b < a) b = a;
  return {a, b};
}
// The edge rows of a launch of M rows (row = (frame - frame_begin) * ch + c) of a stream whose edge frames are
// f < a || f >= b: rows [0, n_pre) and [suf0, M), n of them (suf0 >= n_pre).
struct EdgeRows {
  unsigned n_pre, suf0, n;
};
GLC_HD inline EdgeRows edge_rows(unsigned long long a, unsigned long long b, unsigned long long frame_begin, unsigned M,
                                 unsigned ch) {
  const unsigned long long nf = M / ch, fe = frame_begin + nf;
  const unsigned long long pre = a > frame_begin ? (a < fe ? a : fe) - frame_begin : 0;
  const unsigned long long s = b > frame_begin ? (b < fe ? b : fe) - frame_begin : 0;  // first suffix frame of the launch
  const unsigned n_pre = static_cast<unsigned>(pre) * ch;
  unsigned suf0 = static_cast<unsigned>(s) * ch;
  if (suf0 < n_pre) suf0 = n_pre;
  if (suf0 > M) suf0 = M;
  return {n_pre, suf0, n_pre + (M - suf0)};
}
constexpr unsigned kEdgeRowsMax = 32;  // edge rows a launch may hand to the side stream: 4 frames x 8 channels
constexpr unsigned long long kNoEdge = ~0ull;  // b of a launch that takes no edge path (with a = 0): no frame is an edge frame
// true where the matrix form (MatrixBound) exists for a launch: the rate's ne, a channel count with a segment
// loader, and the table image uploaded
bool encode_matrix_bound_built(const DeviceTables &t, const ScreenShape &sh, uint32_t ch);
// One v_mfma_f32_32x32x16_bf16 of one wave on given operands (the instruction the matrix form accumulates with):
// a, b = 64 lanes x 8 bf16 (lane l: index l % 32, K slots 8 (l / 32) .. + 7), c, d = 64 lanes x 16 f32.  Device pointers.
hipError_t launch_debug_mfma_bf16(const uint16_t *a, const uint16_t *b, const float *c, float *d, hipStream_t s);
// K3: per-frame raw-vs-compressed decision and raw fallback plane (channel counts K2 does not decide).
hipError_t launch_decide_raw(const DeviceTables &t, const PcmView &pcm, uint64_t frame_begin,
                             uint32_t n_frames, uint8_t *records, hipStream_t s);

// P1-P3: compact blob of M = n_frames*ch rows of records, written to `blob` on the device at the sections of
// `l` (glc_common.h compact_layout): header, per-frame raw flags, per-row scale and pair count, the ascending
// (u16 idx | i16 q << 16) pairs of every compressed row back to back, then the 2048-sample planes of
// raw-frame rows.  `scratch`: compact_scratch_bytes(M) bytes, 256-byte aligned, nothing in it needs
// initialising.  The alignment padding of the fixed sections is NOT written here (the caller zeroes
// [0, l.o_pairs) first).
// frame_map / clip_dir (both or neither; a round of glc_encode_batch): row m is channel m % ch of real frame
// m / ch, whose record is number frame_map[m / ch].slot among `records` (the virtual stream's frames, junk
// ones included - those are in no map and nothing of them reaches the blob).  clip_dir[2 * i],
// clip_dir[2 * i + 1]: pairs and raw rows the blob holds in front of clip i, for every clip named in a
// FrameMap::clip.
struct FrameMap {
  uint32_t slot;  // record index of this real frame
  uint32_t clip;  // the clip whose first frame this is, or 0xFFFFFFFF
};
uint64_t compact_scratch_bytes(uint64_t M);
hipError_t launch_compact(const uint8_t *records, uint32_t M, uint32_t ch, uint64_t n_frames, void *scratch, uint8_t *blob,
                          const CompactLayout &l, const FrameMap *frame_map, uint64_t *clip_dir, hipStream_t s);

// A1-A3: the pack of a round of glc_encode_batch_device_compact.  The M real rows of `records` (frame_map as in
// launch_rows_from_records_batch: EVERY real frame names its record slot and its clip of the round) become one
// blob per clip - the CompactLayout of the clip's own frames, padding zeroed, no directory - placed back to back
// in `arena` (64-byte aligned) from *cursor rounded up to 64.  clips[k]: first real frame and frames of clip k;
// they tile [0, M / ch) in order.  entries[k] (include/glc.h glc_store_entry) is written for every clip; a clip
// with offset + bytes > arena_bytes is not stored and nothing of it is written; *cursor ends behind the last
// clip, stored or not.  scratch: compact_store_scratch_bytes(M, n_clips) bytes, 256-byte aligned, nothing in it
// needs initialising.  Three launches whatever n_clips, no synchronisation, ordinary stores only.
struct ClipSpan {
  uint32_t first, frames;
};
uint64_t compact_store_scratch_bytes(uint64_t M, uint64_t n_clips);
hipError_t launch_compact_store(const uint8_t *records, uint32_t M, uint32_t ch, const FrameMap *frame_map, const ClipSpan *clips,
                                uint32_t n_clips, void *scratch, uint8_t *arena, uint64_t arena_bytes, uint64_t *cursor,
                                glc_store_entry *entries, hipStream_t s);

// D1: sparse dequant + inverse MDCT + window -> blocks[row][2048].
//   pairs: packed (u16 idx | i16 q << 16), canonical (ascending, unique, idx < 1024)
//   row_begin[M] / row_cnt[M]: pair range of a row; row_scale[M]; row_raw[M]: -1 or offset (in
//   i16) of the frame's raw_pcm vec in raw_pool, row_raw_len[M] its length.
struct DecodeRows {
  const uint32_t *pairs;
  const uint64_t *row_begin;
  const uint32_t *row_cnt;
  const float *row_scale;
  const int64_t *row_raw;
  const uint64_t *row_raw_len;
  const int16_t *raw_pool;
  uint32_t any_raw;  // the stream has rows of raw frames (their blocks are written by a kernel of their own)
};
// R1: the DecodeRows of M = n_frames * ch rows of frame records that are on the device, built there:
// the ascending (k | q << 16) lists of the rows of compressed frames at a fixed stride (row_begin[m] =
// 1024 m), row_scale from the record, rows of raw frames pointing at their frame's planar i16 block
// inside `records` (raw_pool = records, 16-byte aligned), row_raw = -1 for the others.  `workspace`:
// rows_from_records_bytes(M) bytes that stay untouched for as long as *rows is in use.  `stats`: null,
// or kRowStatSlots pairs of device counters, kRowStatStride uint64_t apart, that are ADDED to: the sums over
// the slots of [0] and of [1] are {list entries, raw frames}.  One launch, no synchronisation:
// *rows may be handed to launch_imdct_rows on the same stream at once (any_raw is set: the host does
// not know).
constexpr uint32_t kRowStatSlots = 64, kRowStatStride = 16;  // a 128-byte line per slot
uint64_t rows_from_records_bytes(uint32_t M);
hipError_t launch_rows_from_records(const uint8_t *records, uint32_t M, uint32_t ch, void *workspace, uint64_t *stats,
                                    hipStream_t s, DecodeRows *rows);
// R1 over the real frames of a round of glc_roundtrip_batch_device: row m is channel m % ch of real frame
// m / ch, whose record is number fmap[m / ch].slot among `records` (the virtual stream's frames; the junk ones
// are in no map and get no row).  Here fmap[r].clip names the clip of EVERY real frame.  clip_stats:
// per clip kClipStatSlots pairs of counters, kRowStatStride uint64_t apart (clip i's first at clip_stats +
// i * kClipStatSlots * kRowStatStride), ADDED to as launch_rows_from_records adds to its one set.
constexpr uint32_t kClipStatSlots = 4;
hipError_t launch_rows_from_records_batch(const uint8_t *records, uint32_t M, uint32_t ch, const FrameMap *fmap, void *workspace,
                                          uint64_t *clip_stats, hipStream_t s, DecodeRows *rows);
// R2: the DecodeRows of WINDOWS of COMPACT BLOBS (glc_common.h CompactLayout) that are on the device, built there.
// Nothing of the payload is copied: rows->pairs and rows->raw_pool are ONE common `base` (at or below every blob
// address, 64-byte aligned like every blob) from which row_begin counts in u32 and row_raw in i16, so the lists and
// raw planes are read where they lie inside the blobs.  Entry i of `n_entries` names a blob - address, capacity in
// bytes the caller vouches for, `rows` = ALL rows of the blob the host expects (frames * ch) - and the window [win[0],
// win[0] + win[1]) of its rows (whole frames, inside the blob; win[1] >= 1) whose tables are rows [first_row,
// first_row + win[1]) of this launch; first_row ascends from 0 and the windows' rows sum to M (whole frames: an M that
// is no multiple of ch is refused).  A WHOLE BLOB is the window {0, rows}.  The same blob may be named by any number
// of entries, in any address order.  `dir` is the table of entries on the device, or null with n_entries == 1, when
// `one` travels as a kernel argument.  status[n_entries] (device, kept by the caller for as long as it wants to read
// it; written here, no need to zero it): what the checks found, per ENTRY.
//   header (k_r2_headers, one thread per entry): glc_common.h compact_header_fault - magic, ch, exactly rows / ch frames,
//   n_pairs <= 1024 rows, n_raw_rows <= rows and a multiple of ch, bytes == the sum of the sections <= capacity.
//   A blob that fails is read no further: its window's rows are empty lists of scale 0.0f with no raw plane, and
//   all rejected (n_bad_rows = win[1], first_bad_row = win[0]).
//   prefix (k_r2w_prefix): the pairs and the rows of raw frames IN FRONT of the window, a reduction over the is_raw
//   and cnt sections of rows [0, win[0]) - 4096 rows per workgroup, one vector atomic add per workgroup and sum into
//   the entry's status.  No row in front of a window gets a table entry, none has its list read or is validated.
//   Not launched when every window starts at its blob's row 0 (mode.max_front == 0).
//   scans (k_r2_scan_rows, k_r2_scan_blocks): row_begin = exclusive 64-bit sum of cnt over the blob's rows in
//   front (rows of raw frames count 0 whatever their cnt says), raw plane = rows of raw frames in front: sums
//   inside blocks of 1024 table rows, one workgroup scans the block sums in chunks of 1024 and takes each entry's
//   own origin - the running sums at its first row minus its window's prefix - out of them.
//   rows (k_r2_rows, one wave per row): a compressed row is kept when cnt <= 1024, row_begin + cnt <= n_pairs and
//   its bins ascend strictly below 1024; the rows of a raw frame when the frame's planes lie below n_raw_rows
//   and inside `bytes`.  A row that is not kept becomes the empty list with its stored scale and no raw plane.
//   first_bad_row / n_bad_rows count the window's rows in the blob's row numbering.
//   No load leaves [address, address + capacity), and nothing behind a window is read.
// mode {totals, max_front, verdict}.  totals: a launch of WHOLE blobs, every win = {0, rows} and max_front 0.  Each
// entry's two sums are compared with the totals its header promised (kCompactPairSum / kCompactRawSum: reported, they
// reject nothing), and M == 0 queues the header kernel alone.  Without it - a launch of windows - the sums say nothing
// about the totals, so the two flags are never set, also where a window covers its blob; M == 0 is refused.
// max_front: the largest win[0] of the entries, or a bound of it (it sizes the prefix launch).  verdict (null, or
// n_entries device words): bits that
// join kCompactBadHeader in the status of an entry whose header check fails - the draw planner's word about an entry
// it emptied (cap 0: the capacity pre-check fails it and nothing is read).
// Fixed slots (glc_decode_crops_device_store): an entry of a window launch may own MORE table rows than its window
// has - first_row of the next entry lies further on, and M counts the slots.  The rows of a slot behind the window
// are empty rows (count 0, scale 0.0f, no raw plane) that report nothing; win[1] may then be 0.
// workspace: rows_from_compact_bytes(M) = 5 row arrays of align256(8 M), align256(4 M), align256(4 M), align256(8 M),
// align256(8 M) bytes (32 B per TABLE row) + 2 x align256(8 ceil(M / 1024)) bytes of block sums, M counted as 1 when
// 0, align256 = rounding up to 256: nothing in it is per row of a blob.  It stays untouched while *rows is in use.
// Four launches, five with the prefix, whatever n_entries (up to 65535; one more prefix launch per 65535 beyond), no
// synchronisation, no workgroup waits for another; any_raw is set (the host does not know).
struct CompactBlob {
  uint64_t addr, cap;
  uint32_t first_row, rows;
  uint32_t win[2];  // first row and row count of the window inside the blob; a whole blob: {0, rows}
};
constexpr uint32_t kCompactBadHeader = 1u, kCompactRowBounds = 2u, kCompactNotCanonical = 4u, kCompactRawRange = 8u,
                   kCompactPairSum = 16u, kCompactRawSum = 32u;
struct CompactStatus {  // 64 bytes per entry
  uint32_t flags, header_ok;
  uint64_t n_bad_rows, first_bad_row;  // first_bad_row: ~0 while no row has been rejected
  uint64_t n_pairs, n_raw_rows, bytes;  // of a header that passed
  uint64_t pairs_before, raw_before;    // running sums of the launch at the entry's first row minus its window's prefix, mod 2^64
};
struct R2Mode {
  bool totals;
  uint32_t max_front;
  const uint32_t *verdict;
};
uint64_t rows_from_compact_bytes(uint32_t M);
hipError_t launch_rows_from_compact(const CompactBlob *dir, const CompactBlob &one, uint32_t n_entries, uint32_t M, uint32_t ch,
                                    const R2Mode &mode, const void *base, void *workspace, CompactStatus *status, hipStream_t s,
                                    DecodeRows *rows);
// variant (include/glc_debug.h): 0 = shipped (k_imdct_plan + k_imdct_apply, absent row pairs skipped
// by scalar branches); 1 = one row per workgroup (the cross-check kernel); 2 = plan + apply without
// the skip; 3 = without the issue-priority schedule; 4 = skipping in row pairs only.  All but 1 need a workspace `plan` of imdct_plan_bytes(plan_groups) bytes,
// plan_groups >= ch (launches with more (frame group, channel) units go through it in batches).
// reuse_plan: the workspace still holds the plan records of exactly this launch (same rows, same
// row_begin and M, one batch) - only the apply kernel runs.
uint64_t imdct_plan_bytes(uint32_t groups);
hipError_t launch_imdct_rows(const DeviceTables &t, const DecodeRows &rows, uint32_t row_begin,
                             uint32_t M, uint32_t ch, float *blocks, hipStream_t s, int variant = 0,
                             void *plan = nullptr, uint32_t plan_groups = 0, bool reuse_plan = false);
// D2: overlap-add + interleave of hops [hop_begin, hop_end) into out (hop h = second half of
// frame h-1 + first half of frame h; hop n_frames is the bare overlap tail).  `blocks` holds
// frames blk_frame0, blk_frame0+1, ... (blk_frame0 may be -1: a zero "frame before the first").
hipError_t launch_overlap_add(const float *blocks, int64_t blk_frame0, uint64_t n_frames,
                              uint32_t ch, uint64_t hop_begin, uint64_t hop_end, float *out,
                              hipStream_t s);
// ... with the narrowing of the reference's 16-bit writers on the way out: the same sums, then
// `(v * 32767.0).clamp(-32768.0, 32767.0) as i16` (NaN -> 0, truncation) - `out` is any 2-byte aligned pointer.
hipError_t launch_overlap_add(const float *blocks, int64_t blk_frame0, uint64_t n_frames,
                              uint32_t ch, uint64_t hop_begin, uint64_t hop_end, int16_t *out,
                              hipStream_t s);

// S1: the interleaved virtual stream of a round of glc_roundtrip_batch_device, gathered from strided device
// audio.  clips[k] (ascending `slot`, clips[0].slot == 0): the clip's first sample is element `src` of the
// source, it has `len` samples per channel and owns the virtual frame slots [slot, clips[k + 1].slot).
// Interleaved source: sample t of channel c at src + t * ch + c; planar: at src + c * channel_stride + t.
// vstream[(1024 v + i) * ch + c] for v < n_virtual_frames: the clip's sample 1024 (v - slot) + i, +0.0 from
// `len` on - EVERY element of the stream is written.  vstream is 16-byte aligned, the source 4-byte.
struct StageClip {
  uint64_t src, len;
  uint32_t slot, pad[3];
};
hipError_t launch_stage_clips(const float *src, const StageClip *clips, uint32_t n_clips, uint32_t ch, bool planar,
                              uint64_t channel_stride, uint32_t n_virtual_frames, float *vstream, hipStream_t s);
// ... from integer clips (`wide`: int32_t samples of 1..32 bits, else int16_t of 1..16), widened in the SAME pass
// by W1's rule (launch_pcm_widen below: one device function serves both): `src`, StageClip::src and channel_stride
// count elements of the sample type, the source is aligned to its sample and to nothing more.  The zeros behind
// a clip are +0.0, not widened integer zeros.
hipError_t launch_stage_clips_int(const void *src, bool wide, uint32_t bits, const StageClip *clips, uint32_t n_clips, uint32_t ch,
                                  bool planar, uint64_t channel_stride, uint32_t n_virtual_frames, float *vstream, hipStream_t s);

// S2: the segment stager of a streaming push (glc_stream_enc_push_device; DESIGN section 3, "a round of segments").
// A lane's stream is numbered in samples per channel from 0; of the `received` samples it has had so far the session
// holds back [held_x, received) as floats, interleaved, at element held_old of `held`; the push brings n_new more at
// element `src` of the source (laid out as S1's clips are).  A span is a run of 512-sample UNITS whose first one shows
// the lane's sample x0 (negative in front of the stream: +0.0) and which lasts until the next span's `unit`:
//   units [0, vs_units)   half hops of the round's virtual stream, vstream[unit * 512 * ch ..): the span of a segment
//                         of frames [F, F + n) starts at unit 2 slot - 1 with x0 = 1024 F - 512 and owns 2 n + 2 units,
//                         so that the frame in virtual slot `slot` + k is the lane's frame F + k.  Units 0 and
//                         vs_units - 1 belong to no span and are written +0.0.
//   units from vs_units   the new held-back samples of a lane, 4 units from element held_new of `held`, x0 = the new
//                         held_x; what lies at or behind received + n_new is written +0.0.
// Spans ascend in `unit`; spans[0].unit is 1 (0 when vs_units == 0).  Every element of the virtual stream and of the
// named held-back buffers is written; held_old and held_new of a lane are different buffers.  Samples at or behind
// received + n_new are +0.0: the padding behind a finished stream.  Integer sources are widened by W1's rule.
struct StreamSpan {
  uint64_t src;       // element of the lane's new chunk in the source
  uint64_t received;  // samples per channel the lane had before this push
  uint64_t n_new;     // ... and what the push adds
  uint64_t held_x;    // the lane's sample at held_old
  uint64_t held_old, held_new;  // elements of `held`, multiples of 4
  int64_t x0;
  uint32_t unit, pad;
};
hipError_t launch_stage_segments(const void *src, glc_pcm_format fmt, uint32_t bits, const StreamSpan *spans, uint32_t n_spans,
                                 uint32_t vs_units, uint32_t held_units, uint32_t ch, bool planar, uint64_t channel_stride,
                                 float *held, float *vstream, hipStream_t s);

// D2 by descriptor, one per kept output hop (the batch drivers): the hop is made of the second half of block slot
// `prev` (-1: +0.0, a stream's first hop) and the first half of slot `cur` (-1: none, the bare tail).  The
// destination is a 64-bit element index bound to no alignment beyond that of `out`, which is aligned to its
// element.  Interleaved (cstride == 0 in every descriptor): out[dst .. dst + cnt) = samples [first,
// first + cnt) of the hop.  `planar`: the span is the clip's interleaved samples [j0, j0 + cnt), sample j going
// to out[dst + (j % ch) * cstride + j / ch] - dst is the clip's first element.
struct HopDescStrided {
  int32_t prev, cur;
  uint32_t first, cnt;
  uint64_t dst, cstride, j0;
};
hipError_t launch_overlap_add_strided(const float *blocks, const HopDescStrided *desc, uint32_t n_desc, uint32_t ch, bool planar,
                                      float *out, hipStream_t s);
// ... narrowed to 16-bit PCM as launch_overlap_add narrows: dst and cstride count 2-byte elements, `out` is any
// 2-byte aligned pointer, chunks are short4 at 8-byte boundaries.  A null descriptor writes nothing here either.
hipError_t launch_overlap_add_strided(const float *blocks, const HopDescStrided *desc, uint32_t n_desc, uint32_t ch, bool planar,
                                      int16_t *out, hipStream_t s);
// The descriptor of hop h of a clip of `nf` frames whose frame f is block slot base + f, the ONE statement of it for
// the host drivers (write_hop_descs) and the draw planner: the span of the hop that `trim` keeps lands from element
// `dst` on, interleaved, or (planes) in planes `cstride` apart.  false: the trim keeps nothing of the hop.
GLC_HD inline bool hop_desc(HopDescStrided *d, uint64_t nf, uint32_t ch, const Trim &trim, uint64_t h, int64_t base, uint64_t dst,
                            bool planes, uint64_t cstride) {
  const uint64_t per_hop = uint64_t(kHop) * ch, lo_all = trim.start, hi_all = trim.start + trim.n;
  const uint64_t lo = lo_all > h * per_hop ? lo_all : h * per_hop, hi = hi_all < (h + 1) * per_hop ? hi_all : (h + 1) * per_hop;
  if (hi <= lo) return false;
  const uint64_t j0 = lo - trim.start;
  *d = HopDescStrided{h >= 1 ? static_cast<int32_t>(base + static_cast<int64_t>(h) - 1) : -1,
                      h < nf ? static_cast<int32_t>(base + static_cast<int64_t>(h)) : -1,
                      static_cast<uint32_t>(lo - h * per_hop),
                      static_cast<uint32_t>(hi - lo),
                      planes ? dst : dst + j0,
                      planes ? cstride : 0ull,
                      j0};
  return true;
}

// The draw planner (glc_decode_crops_device_store; DESIGN section 3, "drawing from the store"): crop i of n_crops is
// samples [starts[i], starts[i] + length) per channel of stored clip clips[i] - device data, as are the store's index
// entries[n_entries] and the clips' lengths[n_entries] (samples per channel).  Crop i is number k = i % per_round of
// round i / per_round and owns there table rows [k * max_frames * ch, (k + 1) * max_frames * ch), block slots
// [k * max_frames, (k + 1) * max_frames) and descriptors [k * max_hops, (k + 1) * max_hops) (glc_common.h
// store_crop_slots).  Written, one launch for all rounds:
//   dir[i]      usable: {arena + offset, bytes, k * max_frames * ch, frames(len) * ch, {first_frame * ch, n_frames * ch}}
//               (glc_common.h plan_crop); unusable: {arena, 0, k * max_frames * ch, 0, {0, 0}}
//   desc[i * max_hops + s]   usable: hop_desc of hop first_hop + s with base = k * max_frames - first_frame and the
//               destination of clip i of the output layout, null ({-1, -1, 0, 0, 0, 0, 0}) from n_hops on; unusable:
//               both slots absent over interleaved samples [s * 1024 ch, (s + 1) * 1024 ch) of the span (+0.0)
//   verdict[i]  0, kCompactBadCrop (clip index outside [0, n_entries), a length below 0, above max_length or one the
//               encoder refuses, start < 0, start + length beyond the clip: the entry is then not read) or
//               kCompactNoBlob (stored == 0, offset no multiple of 64, [offset, offset + bytes) not inside the arena)
// max_length * ch must not wrap and frames(max_length) * ch must fit 32 bits (the caller's check).  No load leaves
// the four index arrays; `arena` is a number here, nothing of the arena is read.
// The RAGGED form (glc_decode_ragged_crops_device_store; `ragged` set, max_hops = store_ragged_slots' max_descs): crop
// i wants w = want ? want[i] : length samples from starts[i] on and gets v = min(w, len - start) of them, the rest of
// its `length` is +0.0.  The selection is usable when the index is in range, the length is the encoder's and at most
// max_length, 0 <= start < len and 1 <= w <= length - start + length may lie beyond the clip, and max_length below
// length.  Of a usable crop:
//   dir[i]      as above, with the window plan_crop gives for {start, v}
//   desc[i * max_hops + s]   s < n_hops: hop_desc of hop first_hop + s with the trim {whole.start + start * ch, v * ch};
//               then the padding, a hop's worth per slot, both slots absent over interleaved samples [v * ch + k * 1024
//               ch, min(v * ch + (k + 1) * 1024 ch, length * ch)) of the span, k = s - n_hops; null behind that
//   valid[i]    v (where `valid` is not null); 0 for an unusable crop, which is otherwise as above
// No load leaves the four index arrays and `want`.
constexpr uint32_t kCompactNoBlob = 64u, kCompactBadCrop = 128u;
struct StoreDraw {
  uint64_t arena, arena_bytes;
  const glc_store_entry *entries;
  const int64_t *lengths;
  uint64_t n_entries, max_length;
  const int64_t *clips, *starts;
  uint64_t length, n_crops;
  uint32_t ch, max_hops, max_frames, per_round;
  uint64_t clip_stride, channel_stride;  // of the output layout, in elements
  uint32_t planes, ragged;               // planes: planar output of more than one channel
  CompactBlob *dir;
  HopDescStrided *desc;
  uint32_t *verdict;
  const int64_t *want;  // the ragged form's two: either may be null
  int64_t *valid;
};
hipError_t launch_store_plan_crops(const StoreDraw &a, hipStream_t s);

// The segment planner of a streaming decode push (glc_stream_dec_push_device; DESIGN section 3, "a lane's carry"):
// segment j of n_segs is the blob entries[j] names - device data - and owns table rows [segs[j].first_row,
// segs[j].first_row + segs[j].rows) of its round (the host's word, from the table image).  Written, one launch per push:
//   dir[j]      usable: {arena + offset, bytes, first_row, rows, {0, rows}}: the whole blob is the window, and its header
//               must carry exactly rows / ch frames; unusable: {arena, 0, first_row, 0, {0, 0}} - the slot's rows are
//               empty rows and nothing is read
//   verdict[j]  0, or kCompactNoBlob (stored == 0, offset no multiple of 64, [offset, offset + bytes) not inside the arena)
// No load leaves entries[0 .. n_segs); `arena` is a number here, nothing of the arena is read.
struct StreamDecSeg {
  uint32_t first_row, rows;
};
hipError_t launch_stream_dec_plan(uint64_t arena, uint64_t arena_bytes, const glc_store_entry *entries, const StreamDecSeg *segs,
                                  uint32_t n_segs, CompactBlob *dir, uint32_t *verdict, hipStream_t s);

// The carry of a streaming decode ("a lane's carry"): per lane 2 x [ch][1024] floats at element
// `carry` of the session's buffer (a multiple of 4) - (a) the finished sums of the lane's last hop, (b) the second half
// of its last frame's windowed block.  Two roles, one descriptor per lane of the round that takes part:
//   load (in front of D2)  (a) -> the second half of block slot `prev`, (b) -> the second half of slot prev + 1: the
//                          pseudo-slots of the lane, behind the round's real frames.  `cur` is not used.  The sums
//                          re-enter D2 as the second half of a slot whose hop has no `cur`, so D2 adds nothing to them.
//   save (behind D1)       (a) <- d2_sum(second half of slot `prev` (-1: absent, +0.0), first half of slot `cur`) - the
//                          sum D2 would form, by D2's own function and in its order; (b) <- the second half of slot `cur`.
// blocks: [slot][ch][2048] floats, 16-byte aligned.  Memory-bound: 16-byte loads and stores, a grid of (units of 256
// float4, lanes), the lane's descriptor read once per workgroup; ordinary vector stores, no flags, no atomics.
struct StreamCarry {
  int32_t prev, cur;
  uint64_t carry;
};
hipError_t launch_stream_dec_carry(bool save, const StreamCarry *desc, uint32_t n_desc, uint32_t ch, float *blocks, float *carry,
                                   hipStream_t s);

// Eviction (glc_store_compact_device; DESIGN section 3, "evicting from the store").  include/glc.h states the rules;
// the two launchers below are all of the call.
//   E1  k_store_evict_scan, ONE workgroup of 1024 threads over chunks of 1024 entries with a carry (k_store_place's
//       form): usability, the exclusive prefix maximum of the candidates' ends, the kept flag, the exclusive scans of
//       the kept sizes and counts; new_index for every entry, entries_out / lengths_out for the kept ones, the move
//       table in the workspace, *n_out and *cursor.  A chunk is read whole before anything of it is written and a
//       kept entry's number never exceeds its index, so entries_out may be entries (and lengths_out lengths).
//   E2  k_store_evict_tail: the all-zero words of entries_out / lengths_out [n_out, n_entries).
//   M   k_store_evict_gather (out of place) / k_store_evict_round (in place): tiles of kStoreMoveTile packed bytes; the
//       kept entries a tile meets by binary search over the ascending new offsets of the move table, 16-byte loads
//       and stores.
// The workspace (store_evict_ws_bytes(n_entries), 8-byte aligned): u64 head[8] = {n_out, total, limit, first_moved, n_entries + 1},
// u64 new_off[n_entries + 1] (new_off[n_out] = total), u64 src_off[n_entries].  limit: the end of the last stored
// kept blob - the stored ones are a prefix, every size being positive -; first_moved: the new offset of the first
// kept blob that is not where it was (total when none moves): in place nothing below it is touched.
constexpr uint32_t kStoreMoveTile = 16384;   // packed bytes per workgroup pass: 256 threads x 4 x 16 bytes
constexpr uint32_t kStoreMoveGrid = 2048;    // workgroups of a move launch at most (grid-stride behind them)
constexpr int64_t kStoreDropped = -1, kStoreUnusable = -2, kStoreOutOfOrder = -3;
struct StoreEvict {
  uint64_t arena_bytes, dst_bytes;
  const glc_store_entry *entries;
  const int64_t *lengths;        // or null (then lengths_out is null too)
  const uint8_t *keep;
  uint64_t n_entries;
  glc_store_entry *entries_out;
  int64_t *lengths_out;
  int64_t *new_index;
  uint64_t *n_out, *cursor;
  uint64_t *ws;
};
inline uint64_t store_evict_ws_bytes(uint64_t n_entries) { return (8ull + 2ull * n_entries + 1ull) * 8ull; }
hipError_t launch_store_evict_scan(const StoreEvict &a, hipStream_t s);
// Out of place: packed bytes [0, limit) from their sources in `arena` to `dst`, one launch whose shape depends on
// arena_bytes alone.
hipError_t launch_store_evict_gather(const uint64_t *ws, const void *arena, uint64_t arena_bytes, void *dst, hipStream_t s);
// In place, launch r of ceil(arena_bytes / round) + 1: staging[(r - 1) & 1] goes back to packed bytes
// [(r - 1) round, r round) of the arena and packed bytes [r round, (r + 1) round) are gathered into staging[r & 1]
// (stage: two buffers of `round` bytes, the second at stage + round; round a multiple of 64).  The two halves
// touch disjoint bytes: every source of round r lies at or behind r * round.  Bytes below first_moved and at or
// above total are neither staged nor written.
hipError_t launch_store_evict_round(const uint64_t *ws, void *arena, void *stage, uint64_t round, uint64_t r, hipStream_t s);

// The segment join (glc_store_join_segments_device; DESIGN section 3, "joining a clip's segments").  include/glc.h
// states the rules; the two launchers below are all of the call.
//   J1  k_store_join_plan, one workgroup of 256 threads per segment: the entry rule of the draw, the header rule with
//       the segment's frames exact and the entry's bytes available, then - only behind a header that passed - the sum of
//       the cnt section and the count of set is_raw bytes, 16-byte loads over the 64-byte aligned sections, the words
//       behind the rows masked.  seg_status[j] and found[j] = {arena offset, n_pairs, n_raw_rows, bad}; a bad segment
//       counts no pairs and no raw rows.
//   J2  k_store_join_scan, ONE workgroup of 1024 threads (k_store_evict_scan's form, chunks of 1024 with a carry): the
//       exclusive scans of found[].n_pairs / n_raw_rows / bad over ALL segments - a clip's totals and a segment's place
//       in its clip are differences of them -, then over the clips the sizes, the exclusive scan of the sizes from the
//       rounded-up cursor, entries_out, lengths_out, the headers of the stored clips, the cursor and the move table.
//   M   k_store_join_move: tiles of kStoreMoveTile bytes of the packed destination space [0, limit); a 16-byte unit
//       finds its clip by search over clip_off, its section from the clip's layout and its segment by search over the
//       segments' starts in that section's run.
// The workspace (store_join_ws_bytes(n_segs, n_clips), 8-byte aligned), in uint64_t words: head[8] = {base, total,
// limit} (base: the rounded-up cursor; total, limit: packed - relative to base - ends of all and of the stored clips),
// found[n_segs] of 4 words, ex_pairs / ex_raw / ex_bad of n_segs + 1 words each, clip_off[n_clips + 1] (packed),
// clip_sum[n_clips] of 2 words {n_pairs, n_raw_rows}.
struct StoreJoinSeg {   // host, in the table image
  uint32_t clip, pad;
  uint64_t first_frame, n_frames;
};
struct StoreJoinClip {  // host, in the table image
  uint64_t seg_first, n_segs, n_frames;
  int64_t length;
};
struct StoreJoin {
  const unsigned char *arena;
  uint64_t arena_bytes;
  const glc_store_entry *entries;
  const StoreJoinSeg *segs;
  uint64_t n_segs;
  const StoreJoinClip *clips;
  uint64_t n_clips;
  uint32_t ch, has_lengths;
  unsigned char *dst;
  uint64_t dst_bytes;
  uint64_t *cursor;
  glc_store_entry *entries_out;
  int64_t *lengths_out;  // or null
  uint32_t *seg_status;
  uint64_t *ws;
};
inline uint64_t store_join_ws_bytes(uint64_t n_segs, uint64_t n_clips) {
  return (8ull + 4ull * n_segs + 3ull * (n_segs + 1ull) + (n_clips + 1ull) + 2ull * n_clips) * 8ull;
}
hipError_t launch_store_join_plan(const StoreJoin &a, hipStream_t s);
// max_bytes: a host bound on the packed bytes of the stored clips; the launch's shape depends on it alone.
hipError_t launch_store_join_move(const StoreJoin &a, uint64_t max_bytes, hipStream_t s);

// The cut (glc_store_cut_device; DESIGN section 3, "cutting a stored clip").  include/glc.h states the rules; the two
// launchers below are all of the call.
//   C1  k_store_cut_plan, one workgroup of 256 threads per cut: thread 0 judges the selection (clip < n_entries), the
//       entry (the draw's rule), the header (its own frame count, bounded as glc_compact_join bounds it before any size
//       is formed, entry.bytes available) and the window (inside the header's frames).  Behind a header and a window
//       that passed, all threads reduce the cnt words of the rows in front of the window (P0) and in it (P), every
//       word held to 1024, and the non-zero is_raw bytes in front (R0 / ch) and in it (R / ch): 16-byte loads over
//       the 64-byte aligned sections, the edges masked.  Nothing behind the window's last row / frame is read.
//       cut_status[i] and found[i] = {arena offset, P0, P, R0, R, bad, the source's n_frames, the source's n_pairs}.
//   C2  k_store_cut_scan, ONE workgroup of 1024 threads (k_store_join_scan's form, chunks of 1024 with a carry): the
//       sizes, their exclusive scan from the rounded-up cursor, entries_out, lengths_out, the headers of the stored
//       pieces, the cursor and the move table.
//   M   k_store_cut_move: tiles of kStoreMoveTile bytes of the packed destination space [0, limit).  Every run of a
//       piece - is_raw, scale, cnt, pairs, raw - is ONE contiguous range of the source blob, so a tile whose first and
//       last unit lie in one run of one cut has one source base for all its units; a tile that spans runs or pieces
//       finds each unit's cut by search over cut_off and its run from the piece's layout.
// The workspace (store_cut_ws_bytes(n_cuts), 8-byte aligned), in uint64_t words: head[8] = {base, total, limit} (as
// the join's), found[n_cuts] of 8 words, cut_off[n_cuts + 1] (packed), runs[n_cuts] of 10 words: per run the arena
// offset of its first byte and its bytes without the padding.
struct StoreCutItem {  // host, in the table image
  uint64_t clip, first_frame, n_frames;
  int64_t length;      // what lengths_out receives for a piece that is cut
};
struct StoreCut {
  const unsigned char *arena;
  uint64_t arena_bytes;
  const glc_store_entry *entries;
  uint64_t n_entries;
  const StoreCutItem *cuts;
  uint64_t n_cuts;
  uint32_t ch, pad;
  unsigned char *dst;
  uint64_t dst_bytes;
  uint64_t *cursor;
  glc_store_entry *entries_out;
  int64_t *lengths_out;
  uint32_t *cut_status;
  uint64_t *ws;
};
inline uint64_t store_cut_ws_bytes(uint64_t n_cuts) { return (8ull + 8ull * n_cuts + (n_cuts + 1ull) + 10ull * n_cuts) * 8ull; }
hipError_t launch_store_cut_plan(const StoreCut &a, hipStream_t s);
// max_bytes: a host bound on the packed bytes of the stored pieces; the launch's shape depends on it alone.
hipError_t launch_store_cut_move(const StoreCut &a, uint64_t max_bytes, hipStream_t s);

// The interleaved descriptor with a 32-bit destination, 24 bytes instead of 40: what glc_decode_batch uploads per
// kept hop (its rounds address their output in 31 bits).  Same kernel, same chunks; kept beside HopDescStrided
// because that driver measured slower, per launch and per call, with the wide form.
struct HopDesc {
  int32_t prev, cur;
  uint32_t dst, first, cnt, pad;
};
hipError_t launch_overlap_add_strided(const float *blocks, const HopDesc *desc, uint32_t n_desc, uint32_t ch, float *out,
                                      hipStream_t s);
// ... narrowed to 16-bit PCM as launch_overlap_add narrows (glc_decode_batch_i16): dst an index of 2-byte elements.
hipError_t launch_overlap_add_strided(const float *blocks, const HopDesc *desc, uint32_t n_desc, uint32_t ch, int16_t *out,
                                      hipStream_t s);

// W1: interleaved integer PCM -> f32 as the reference's loaders widen it: out[i] = (float)in[i] / max,
// max = 2^(bits-1), -2^31 for bits == 32.  `wide`: int32_t samples (bits 1..32), else int16_t
// (bits 1..16); `in` aligned to its sample size, `out` to 4 bytes.
hipError_t launch_pcm_widen(const void *in, bool wide, uint32_t bits, uint64_t n, float *out, hipStream_t s);

// Measurement only (include/glc_debug.h): one sleeping wave that reports {shader cycles, 100 MHz ticks}
// over a window of `ticks_100mhz` reference ticks, beside whatever runs on the device meanwhile.
hipError_t launch_clock_probe(uint64_t ticks_100mhz, uint64_t *out, hipStream_t s);

}  // namespace glc
