/*
 * glc_debug.h - cross-check hooks of libglc_hip.so.  NOT part of the drop-in boundary (that is
 * include/glc.h): these entry points exist so that soak tools and tests can run one stream through
 * two independent implementations of the same arithmetic and demand identical bits, or drive one kernel
 * stage on inputs built for the purpose (tests/test_quantizer_edges.py, tests/test_decode_edges.py,
 * tests/test_compact_edges.py).  tests/test_channel_axis.py drives the store pack, the windowed R2 and the draw
 * planner through their hooks at 4, 5, 7, 9, 16, 17, 257 and 513 channels.  tests/test_encode_screen_drivers.py holds
 * the screened encode under the store encode (glc_encode_batch_device_compact and _int), the stream push (device and
 * host) and glc_roundtrip_batch_device_pcm to the oracle with glc_debug_set_encode_screen / _bound / _repair / _edge
 * and their stats: forced on under the FMA and the matrix form with either repair, and, for a clip longer than a round,
 * in the automatic mode; tests/test_encode_screen_edges.py does for glc_encode, glc_encode_batch and the float round
 * trips, under the automatic bound kind and the forced matrix form.
 */
#ifndef GLC_DEBUG_H
#define GLC_DEBUG_H

#include "glc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which inverse-transform kernel the decode entry points of `ctx` launch (imdct_block,
 * src/codec.rs:377-390):
 *   0  shipped: k_imdct_plan + k_imdct_apply - 8 frames of one channel per unit over the union of
 *      their indices; union records in global memory, coefficients fed from SGPRs, absent rows
 *      skipped one by one by scalar branches
 *   1  k_imdct_rows: one row per workgroup, no grouping (the simplest restatement)
 *   2  plan + apply without the skip (every row takes every union entry)
 *   3  plan + apply without the issue-priority schedule (waves of a SIMD finish one after the other)
 *   4  plan + apply skipping absent rows only in pairs (both rows of a pair lack the entry)
 *   5  the shipped kernels, units dealt so that the four which share a CU are consecutive frame groups of
 *      one channel (L1 reuse of table rows) instead of being ranked by work   (placement: speed only)
 *   6  the shipped kernels in the natural unit order with the channel rotated per round (round 2's placement)
 * All of them produce the same bits; tools/soak_decode.py checks that on random streams. */
int glc_debug_set_imdct_variant(glc_ctx *ctx, int variant);

/* Which forward-transform kernel takes the launches of 4096 rows or more of `ctx` (mdct_block,
 * src/codec.rs:359-375; shorter launches are dispatched by row count alone and are not affected):
 *   0  shipped: k_mdct_fwd_st - table values from SGPRs, a wave's lanes hold 256 rows -, 16 waves per
 *      workgroup when the launch's last round of 32 row tiles is full or more than half full, else 8
 *   1  k_mdct_fwd_dma: round 3's kernel (128 x 128 tile, both operands from LDS)
 *   2  k_mdct_fwd_st, 8 waves per workgroup for every launch
 *   3  k_mdct_fwd_st, 16 waves per workgroup for every launch
 *   4  shipped, and launches of 1793..2048 rows take k_mdct_fwd_sched (64 x 128 tile) - the kernel glc_encode gives
 *      its opening rounds, which run beside each other; a launch that has the chip to itself takes the 2 x 4 kernel
 * All of them produce the same bits (tests/test_gpu_parity.py). */
int glc_debug_set_mdct_variant(glc_ctx *ctx, int variant);

/* Whether the encode launches of `ctx` take the screened path (exact transform only for the
 * columns below the last band; the last band by a fused-multiply-add upper bound, and exactly - the repair - for
 * the rows whose bound does not stay under the noise floor):
 *   0  automatic: the launches glc_debug_set_mdct_variant's variant 0 gives to the 16-wave k_mdct_fwd_st, at rates
 *      whose last band starts at 64..960 (rounded up to 64), unless the guard holds the path off: after a launch in
 *      which more than one row in eight failed the screen, 32 launches take today's kernels, then one probes, and
 *      no other is screened until the probe's count is back; a context's first screened launch counts as a probe
 *   1  off: today's kernels for every launch
 *   2  on for every launch of 256 rows or more, guard ignored (tests reach the path with a few hundred rows)
 * A launch with a coefficient tap (d_coeffs) and glc_mdct_forward_device never take it.  All modes produce the
 * same record bytes (tests/test_encode_screen.py). */
int glc_debug_set_encode_screen(glc_ctx *ctx, int mode);
/* Rows the screened path has transformed since the context was created, and how many of them failed the screen
 * and were repaired.  Waits for the context's encode streams. */
int glc_debug_encode_screen_stats(glc_ctx *ctx, uint64_t *rows_screened, uint64_t *rows_repaired);
/* The layout a screened launch has at a rate whose last band starts in (64 (ne - 1), 64 ne], ne in 1..15: the exact
 * column pairs of the transform's hybrid waves (0: none, waves [0, ne) are exact - csrc/glc_mdct_fwd.hpp mix_wave), the
 * hf planes the transform writes and the quantiser reads (the A plane follows them), and the bytes of the workspace
 * of a launch of `rows` rows: (planes + 1) planes of rows rounded up to 256 floats, one of row flags, a quarter of
 * one of fail counts.  Host arithmetic only: no context, no device. */
int glc_debug_encode_screen_layout(uint32_t ne, uint32_t rows, uint32_t *hybrid_pairs, uint32_t *planes,
                                   uint64_t *workspace_bytes);

/* Which transform repairs the rows of a screened launch that failed the screen (csrc/glc_kernels.h
 * launch_encode_screened):
 *   0  automatic: k_mdct_fwd_small_rows (one wave per two failed rows and 64 columns: a handful of failed rows cost
 *      one wave's chain) when the last failed-row count the device reported is small, k_mdct_fwd_small_cols (the
 *      row tiles that hold a failed row) when it is large or none has been read yet
 *   1  k_mdct_fwd_small_cols for every screened launch
 *   2  k_mdct_fwd_small_rows for every screened launch
 * The setting survives glc_debug_set_encode_screen.  All kinds produce the same record bytes
 * (tests/test_encode_repair.py). */
int glc_debug_set_encode_repair(glc_ctx *ctx, int kind);
/* Screened launches of `ctx` so far whose repair took k_mdct_fwd_small_cols / k_mdct_fwd_small_rows.  Host counters:
 * nothing is waited for. */
int glc_debug_encode_repair_stats(glc_ctx *ctx, uint64_t *launches_tiles, uint64_t *launches_latency);

/* Whether a screened launch of glc_encode_range_device hands its edge frames - the frames whose 2048-sample window
 * reaches into the stream's zero padding: frame 0 and, unless the stream ends exactly where its window does, the last
 * frame - to a side stream of the
 * context (csrc/glc_kernels.h EdgeLaunch): all their exact coefficients, in a buffer of their own, and their records
 * are then produced beside K1 and K2 instead of by the serial repair behind them, and the caller's stream continues
 * behind both.
 *   0  automatic: every screened launch that holds 1..32 edge rows takes it, with the transform of kind 3
 *   1  off: bit for bit the launches of a library without the path
 *   2  on, with k_mdct_edge_rows: the latency repair's chain as it is, 28 table loads in flight (211 VGPRs: its waves
 *      do not fit beside two resident workgroups of K2 on a CU, and K2 then needs a second round)
 *   3  on, with k_mdct_edge_rows_capped: the same chain with 12 table loads in flight, at most 192 VGPRs and 16 KiB of
 *      LDS, which fits beside them.  (Neither fits beside a resident K1 workgroup, which leaves 32 VGPRs per SIMD.)
 * The setting survives glc_debug_set_encode_screen.  All kinds produce the same record bytes, and
 * glc_debug_encode_screen_stats' rows_repaired counts the edge rows that failed the screen whichever path took them
 * (tests/test_encode_edge.py). */
int glc_debug_set_encode_edge(glc_ctx *ctx, int kind);
/* Screened launches of `ctx` so far that took the edge path, and the edge rows they handed to the side stream.  Host
 * counters: nothing is waited for. */
int glc_debug_encode_edge_stats(glc_ctx *ctx, uint64_t *launches, uint64_t *rows);

/* Which form of the mixed-role transform a screened launch takes (csrc/glc_kernels.h MatrixBound):
 *   0  automatic: the matrix form (k_mdct_mx_st: the bound sums on the bf16 matrix pipe) where it is built - 44.1 and
 *      48 kHz, 1 / 2 / 4 / 8 channels - for launches of 3584 rows and up, the FMA form (k_mdct_mix_st) everywhere else
 *   1  the FMA form for every screened launch
 *   2  the matrix form wherever it is built, whatever the row count (and with the screen forced on as well, mode 2 of
 *      glc_debug_set_encode_screen, from 128 rows - one row tile of the form - instead of 256)
 * The setting survives glc_debug_set_encode_screen.  All kinds produce the same record bytes
 * (tests/test_encode_matrix.py). */
int glc_debug_set_encode_bound(glc_ctx *ctx, int kind);
/* H and A of the last screened launch of `ctx` on its own coefficient workspace, which must have had `rows` rows: per
 * row the maximum over the launch's hf planes and the A plane, as the quantiser reads them.  Waits for the stream. */
int glc_debug_encode_bound_tap(glc_ctx *ctx, uint32_t rows, float *h, float *a);
/* One v_mfma_f32_32x32x16_bf16 of one wave on host operands: a, b = 64 lanes x 8 bf16 (lane l: row / column l % 32, K
 * slots 8 (l / 32) .. + 7), c, d = 64 lanes x 16 f32 (lane l, element e: row 8 (e / 4) + 4 (l / 32) + e % 4, column
 * l % 32).  The instruction the matrix form accumulates with, for checking its error model on the device. */
int glc_debug_mfma_bf16(glc_ctx *ctx, const uint16_t *a, const uint16_t *b, const float *c, float *d);
/* The constants of the matrix form (host only; no context, no device): the ne it is built for, bf16 pieces kept per
 * operand, piece products summed, i-steps per instruction, K-blocks per accumulation segment, hf planes of a launch,
 * the per-instruction error model kappa, the split's error and the whole budget per unit of A = sum |x w|, which the
 * library asserts to be within gamma_2048. */
int glc_debug_encode_matrix_bound(uint32_t *ne, uint32_t *pieces, uint32_t *products, uint32_t *k_block, uint32_t *seg_blocks,
                                  uint32_t *planes, double *kappa, double *split_eps, double *budget);

/* K2 (+ K3 where the channel count needs it) exactly as glc_encode_range_device runs them, on caller-supplied
 * coefficients: d_coeffs holds (frame_end - frame_begin) * channels rows of 1024 floats, laid out as
 * glc_mdct_forward_device writes them; d_pcm / t0 / t_count / n_samples are read only for raw planes.
 * Arguments are checked as glc_encode_range_device checks them (halo included); the work is queued on
 * the context's stream and nothing is synchronised.  tests/test_quantizer_edges.py drives the quantiser
 * through this at its decision boundaries. */
int glc_debug_quantize_device(glc_ctx *ctx, const float *d_coeffs, const float *d_pcm, uint64_t t0, uint64_t t_count,
                              uint64_t n_samples, uint16_t channels, uint64_t frame_begin, uint64_t frame_end,
                              void *d_records);

/* D2 (k_overlap_add) exactly as the decode rounds launch it, on caller-supplied blocks: d_blocks holds the
 * frames [blk_frame0, blk_frame0 + n_block_frames) of a stream of n_frames frames as [frame][channel][2048]
 * (blk_frame0 = -1: slot 0 is the carried frame in front of frame 0, which hop 0 never reads); hops
 * [hop_begin, hop_end) go to d_out (cap floats; any 4-byte aligned device pointer), hop n_frames being the bare
 * tail.  Arguments are checked (hop range, the frames the hops read lie inside d_blocks, cap); the work is
 * queued on the context's stream and nothing is synchronised.  tests/test_decode_edges.py drives the
 * overlap-add through this with -0.0 / inf / NaN operands and launches of more than 32768 hops, which no
 * decode entry point can feed it. */
int glc_debug_overlap_add_device(glc_ctx *ctx, const float *d_blocks, int64_t blk_frame0, uint64_t n_block_frames,
                                 uint64_t n_frames, uint16_t channels, uint64_t hop_begin, uint64_t hop_end, float *d_out,
                                 uint64_t cap);

/* The segment-aware compaction (P1-P3, k_pack_*<true>) exactly as a round of glc_encode_batch runs it - frame map,
 * blob layout, memset and launch are the round's own code - on caller-supplied records of a virtual stream: clip i
 * of clip_frames[i] >= 1 frames owns the records slot_i .. slot_i + clip_frames[i] - 1 of d_records, the record
 * behind them is the junk frame between two clips (d_records holds sum(clip_frames[i] + 1) records) and slot_{i+1}
 * follows it.  d_blob (cap bytes) receives header (64 B) | clip directory u64[2 n_clips] (pairs and raw rows in front
 * of clip i) | the sections of glc_compact_device_records over the real frames, every section 64-byte aligned; cap
 * must be at least 64 + align64(16 n_clips) + align64(n_real) + 2 align64(4 M) + 4096 M + 64 for n_real real frames
 * of M rows.  d_records and d_blob must be 8-byte aligned.  Synchronises; the sizes come back through `info`.
 * tests/test_compact_edges.py drives the batch compaction through this with junk records that hold dense rows
 * and raw flags, which no encode leaves there in a chosen place. */
int glc_debug_compact_batch_device(glc_ctx *ctx, const void *d_records, const uint64_t *clip_frames, uint64_t n_clips,
                                   uint16_t channels, void *d_blob, uint64_t cap, glc_compact_info *info);

/* The per-clip pack (A1-A3) alone, exactly as a round of glc_encode_batch_device_compact launches it - frame map, clip
 * table and launch are the driver's own code - on caller-supplied records of a virtual stream laid out as for
 * glc_debug_compact_batch_device: clip i of clip_frames[i] >= 1 frames, one junk record behind each clip.  d_arena,
 * arena_bytes, d_cursor and d_entries as in glc_encode_batch_device_compact (include/glc.h).  Queued on the context's
 * stream behind the table upload; not synchronised.  tests/test_compact_store.py drives the pack through this with
 * junk records that hold dense rows and raw flags, nnz fields that disagree with their rows and 1100 clips in a round;
 * tests/test_channel_axis.py with rows per clip that are no multiple of 4, up to 513 channels. */
int glc_debug_compact_store_device(glc_ctx *ctx, const void *d_records, const uint64_t *clip_frames, uint64_t n_clips,
                                   uint16_t channels, void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
                                   glc_store_entry *d_entries);

/* R2 (launch_rows_from_compact, totals compared) alone, exactly as glc_decode_device_compact launches it for ONE blob of `n_frames`
 * frames at d_blob (64-byte aligned, blob_bytes >= the fixed sections): the row tables it builds come back to
 * the host - M = n_frames * channels entries each, any pointer may be NULL - with the status words.  row_begin
 * counts u32 and row_raw i16 from d_blob (-1: no raw plane).  Synchronises.  tests/test_compact_decode.py holds
 * the tables of a blob of more than 1024 * 1024 rows (the second chunk of the block-sum scan) to a model
 * through this: decoding that many frames would take the test minutes. */
int glc_debug_rows_from_compact(glc_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint64_t n_frames, uint16_t channels,
                                uint64_t *row_begin, uint32_t *row_cnt, float *row_scale, int64_t *row_raw,
                                uint64_t *row_raw_len, glc_compact_status *status);

/* R2 of a window (the same launch_rows_from_compact, totals not compared) alone, exactly as
 * glc_decode_crops_device_compact launches it for ONE window of a long clip: frames [first_frame, first_frame + frames)
 * of the blob of `n_frames` frames at d_blob.  The tables of the window's frames * channels rows come back as above -
 * row_begin and row_raw from d_blob, in the blob's own terms, so they are the matching slices of
 * glc_debug_rows_from_compact's, and for the window of all frames the same tables - with the status words.  Both hooks
 * are one body.  Synchronises.  tests/test_compact_crops.py holds windows at the scan's edges, and one behind row 1024 * 1024 of a
 * blob of that many rows, to the model through this; tests/test_channel_axis.py the windows of the oracle's streams of
 * 4 to 513 channels. */
int glc_debug_rows_from_compact_window(glc_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint64_t n_frames, uint16_t channels,
                                       uint64_t first_frame, uint64_t frames, uint64_t *row_begin, uint32_t *row_cnt,
                                       float *row_scale, int64_t *row_raw, uint64_t *row_raw_len, glc_compact_status *status);

/* The draw planner (k_store_plan_crops) alone, exactly as glc_decode_crops_device_store launches it - the checks and
 * the geometry are the call's own code - with what it wrote copied back: dir, out->n_clips records of 32 bytes {u64
 * address, u64 capacity, u32 first_row, u32 rows, u32 win[2]}; desc, out->n_clips * max_hops records of 40 bytes {i32
 * prev, i32 cur, u32 first, u32 cnt, u64 dst, u64 cstride, u64 j0}; verdict, out->n_clips words (0, GLC_COMPACT_NO_BLOB
 * or GLC_COMPACT_BAD_CROP).  The planner never dereferences the arena and nothing is written to d_out, so d_arena may
 * be any 64-byte aligned number and arena_bytes 2^40: offsets beyond 4 GiB and lengths near the 32-bit row limit are
 * reached without the memory.  Synchronises.  tests/test_store_draw.py holds the planner to a model through this, and
 * tests/test_channel_axis.py does at the channel counts whose sample frames begin 1, 8, 255 and 512 positions into a
 * hop's grid (512 % channels). */
int glc_debug_store_plan_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                const int64_t *d_starts, uint64_t length, const float *d_out, const glc_clip_layout *out,
                                void *dir, void *desc, uint32_t *verdict);

/* ... in its ragged form, exactly as glc_decode_ragged_crops_device_store launches it: d_want as that call takes it
 * (device, or NULL), desc out->n_clips * max_descs records (glc_store_ragged_slots), and `valid`, out->n_clips host
 * int64_t: what the planner wrote as d_valid, into a table of the context's.  The arena is only a number here too.
 * Synchronises.  tests/test_store_ragged.py holds the ragged planner to its model through this. */
int glc_debug_store_plan_ragged_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                       const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                       const int64_t *d_starts, const int64_t *d_want, uint64_t length, const float *d_out,
                                       const glc_clip_layout *out, void *dir, void *desc, uint32_t *verdict, int64_t *valid);

/* The carry kernel of the streaming decode (k_stream_dec_carry) alone, for ONE lane whose carry lies at d_carry[0 ..
 * 2 * 1024 * channels): save == 0 copies the two carried halves into the second halves of block slots `prev` and prev + 1
 * of d_blocks ([n_slots][channels][2048] floats); save != 0 writes the carry from slots `prev` (-1: absent) and `cur` as a
 * push that ends with the frame in `cur` does.  Slots outside [0, n_slots) are GLC_EINVAL.  Synchronises.
 * tests/test_stream_decode.py drives it with halves of -0.0, which no decode produces, and checks the sign bit. */
int glc_debug_stream_dec_carry_device(glc_ctx *ctx, int save, int32_t prev, int32_t cur, uint16_t channels, float *d_blocks,
                                      uint64_t n_slots, float *d_carry);

/* The packed bytes an in-place glc_store_compact_device of `ctx` moves per round (include/glc.h): a multiple of 64, 0
 * restores the default.  tests/test_store_compact.py puts blobs of a few hundred bytes across round boundaries with
 * rounds of 1 KiB and 4 KiB; tools/store_compact_bench.cpp measures the rounds the default was chosen from. */
int glc_debug_set_store_compact_round(glc_ctx *ctx, uint64_t bytes);

/* What the library holds of the device at this moment, over all contexts, stream encoders and stream decoders of the
 * process: counts[0] device buffers, [1] pinned host buffers, [2] streams of its own (a caller's stream,
 * glc_ctx_set_stream, is not one), [3] events.  Every one of them belongs to a context, a stream encoder or a stream
 * decoder (or lives for the length of one call) and is released with it, so the counts after glc_ctx_destroy /
 * glc_stream_enc_close / glc_stream_dec_close are the counts before the matching create / open, whatever ran in between
 * and however it ended (tests/test_ctx_resources.py, tests/test_stream_decode.py).  Relaxed atomic counters:
 * no context, no device, nothing is waited for; meaningful when no other thread is inside the library. */
int glc_debug_live_resources(uint64_t counts[4]);

/* The shader clock the device HOLDS under load (measurement only; bench.py's roofline.clock_ghz_held).
 * `begin` starts one sleeping wave on a stream of its own that runs for `window_us` microseconds beside
 * whatever the caller queues meanwhile and reads the shader-cycle counter against the constant 100 MHz
 * counter; `end` waits for it and returns cycles / ticks x 0.1 GHz.  The caller keeps the device busy
 * with the kernel of interest for at least the window. */
int glc_debug_clock_probe_begin(glc_ctx *ctx, uint32_t window_us);
int glc_debug_clock_probe_end(glc_ctx *ctx, float *ghz);

#ifdef __cplusplus
}
#endif
#endif /* GLC_DEBUG_H */
