/*
 * glc.h — C ABI of the MI355X-native MDCT / quantiser hot path of the gapless lossy codec.
 *
 * Drop-in boundary for the reference crate `gapless_lossy_codec` (v0.5.0).  The reference has no
 * FFI seam today: `Encoder` / `Decoder` are concrete Rust structs in src/codec.rs.  Each entry
 * point below names the reference item it replaces (file:line into the reference tree); a thin
 * Rust shim keeps the Rust signatures and forwards here.
 *
 * Conventions
 *   - plain pointers and sizes, no C++/torch types; all integers little-endian host order
 *   - return 0 (GLC_OK) on success, a negative glc_status otherwise; the text of the last
 *     failure is available from glc_last_error()
 *   - a glc_ctx is NOT thread-safe (≙ `&mut self`, src/codec.rs:421,744); distinct contexts may
 *     be used from distinct threads
 *   - inputs the reference would panic on (channels == 0, <= 512 samples per
 *     channel, ragged channel lengths that under-run a frame) return GLC_EINVAL instead
 *   - there is NO CPU fallback: every compute entry point fails with GLC_ENODEV / GLC_EHIP when
 *     no gfx950 device is usable
 */
#ifndef GLC_H
#define GLC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLC_FRAME_SIZE 2048u /* src/codec.rs:15 FRAME_SIZE */
#define GLC_HOP_SIZE 1024u   /* src/codec.rs:16 HOP_SIZE  */
#define GLC_FRAMES_PER_CHUNK 500u /* src/codec.rs:18 */

typedef enum glc_status {
  GLC_OK = 0,
  GLC_EINVAL = -1,  /* bad argument / input the reference panics on */
  GLC_EHIP = -2,    /* HIP runtime or kernel failure */
  GLC_ENOMEM = -3,  /* host or device allocation failed */
  GLC_EFORMAT = -4, /* malformed .glc byte stream (bincode error in load_encoded) */
  GLC_ENODEV = -5,  /* no usable gfx950 device */
  GLC_EIO = -6      /* file I/O error (save_encoded / load_encoded) */
} glc_status;

/* ≙ Encoder / Decoder (src/codec.rs:396-402, :571-577): MDCT table, window, perceptual model,
 * device workspaces and the HIP stream the kernels run on. */
typedef struct glc_ctx glc_ctx;
/* ≙ EncodedAudio (src/codec.rs:31-37), owned by the library. */
typedef struct glc_frames glc_frames;

/* ≙ AudioHeader + GaplessInfo (src/codec.rs:39-53) + summary counts. */
typedef struct glc_info {
  uint32_t sample_rate;
  uint16_t channels;
  uint16_t reserved;
  uint64_t total_samples;
  uint32_t encoder_delay;
  uint32_t padding;
  uint64_t original_length;
  uint64_t n_frames;
  uint64_t n_raw_frames; /* frames carrying raw_pcm: Some(..) */
  uint64_t total_nnz;    /* sum of sparse list lengths */
} glc_info;

/* Result of the padding arithmetic of Encoder::encode (src/codec.rs:433-455, :543-547). */
typedef struct glc_plan {
  uint64_t n_frames;     /* 0 if the reference would panic */
  uint64_t padded_len;   /* per-channel length of padded[0] */
  uint64_t per_channel;  /* per_chan[0].len() */
  uint32_t encoder_delay;
  uint32_t padding;
} glc_plan;

/* ---- context -------------------------------------------------------------------------- */

/* Encoder::new(sample_rate) src/codec.rs:406-418 and Decoder::new(_, sample_rate) :581-592.
 * Builds MdctTables (:326-356) and PerceptualWeights (:102-183) on the host with the system
 * libm, uploads them to HIP device `device`, creates the stream and workspaces. */
int glc_ctx_create(int device, uint32_t sample_rate, glc_ctx **out);
void glc_ctx_destroy(glc_ctx *ctx);
/* Message of the last failure on `ctx` (or of the last context-less failure if ctx == NULL). */
const char *glc_last_error(const glc_ctx *ctx);
/* The HIP stream (hipStream_t) every kernel of this context is launched on.  It is a stream of the context's own,
 * created non-blocking: it does NOT wait for work a caller has queued elsewhere (not even on the legacy default
 * stream).  A device buffer that another stream is still filling or reading must be synchronised with by the
 * caller - or the context put on that stream with glc_ctx_set_stream - before an entry point is given it. */
void *glc_ctx_stream(glc_ctx *ctx);
int glc_ctx_device(const glc_ctx *ctx);
/* Run this context's kernels on a caller-owned hipStream_t instead (e.g. the stream a host
 * framework times with its own events).  The caller keeps ownership; NULL restores the
 * context's private stream. */
int glc_ctx_set_stream(glc_ctx *ctx, void *hip_stream);
/* Block until all work queued on the context's stream has finished. */
int glc_ctx_synchronize(glc_ctx *ctx);
/* Device-side stopwatch on the context's stream: `begin` records a hipEvent, `end` records a
 * second one, waits for it and returns the elapsed milliseconds between the two — the time the
 * kernels queued in between spent on that stream. */
int glc_ctx_timer_begin(glc_ctx *ctx);
int glc_ctx_timer_end(glc_ctx *ctx, float *elapsed_ms);

/* ---- encode --------------------------------------------------------------------------- */

/* Padding / frame-count arithmetic only (host, no device): src/codec.rs:433-455. */
int glc_plan_encode(uint64_t n_samples, uint16_t channels, glc_plan *out);

/* Encoder::encode(&mut self, samples: &[f32], channels: u16) -> Result<EncodedAudio>
 * src/codec.rs:421-565.  `pcm` is interleaved host memory, borrowed for the call. */
int glc_encode(glc_ctx *ctx, const float *pcm, uint64_t n_samples, uint16_t channels,
               glc_frames **out);

/* Fixed-size per-frame record the device path emits (one per frame):
 *   u32 is_raw, u32 reserved, then per channel {f32 scale, u32 nnz}, padded to 16 B,
 *   then int16 payload[channels][2048]: compressed frames hold the dense quantised row in
 *   payload[c][0..1023]; raw frames hold the channel-planar windowed i16 block (Q1). */
uint64_t glc_record_bytes(uint16_t channels);

/* Device-resident frame-range encode: the body of the rayon loop at src/codec.rs:462-541 for
 * frames [frame_begin, frame_end) of a stream of `n_samples` interleaved samples.
 *   d_pcm      device pointer to interleaved f32 PCM covering per-channel sample indices
 *              [t0, t0 + t_count) of the stream (a shard with its halo, or the whole stream
 *              with t0 = 0); samples outside the stream are the encoder's zero padding
 *   d_records  device buffer of (frame_end - frame_begin) * glc_record_bytes(channels) bytes
 *   d_coeffs   optional device buffer [(frame_end-frame_begin)*channels][1024] f32 receiving
 *              the MDCT coefficients (parity tap); NULL to use the context workspace
 * Work is queued on glc_ctx_stream(ctx) and NOT synchronised. */
int glc_encode_range_device(glc_ctx *ctx, const float *d_pcm, uint64_t t0, uint64_t t_count,
                            uint64_t n_samples, uint16_t channels, uint64_t frame_begin,
                            uint64_t frame_end, void *d_records, float *d_coeffs);

/* The transform alone: window (src/codec.rs:476-481) + MdctTables::mdct_block (:359-374) for every
 * frame-channel of [frame_begin, frame_end) -> d_coeffs[(frame-frame_begin)*channels + c][1024].
 * Same arguments as glc_encode_range_device; used for kernel-level timing and the parity tap. */
int glc_mdct_forward_device(glc_ctx *ctx, const float *d_pcm, uint64_t t0, uint64_t t_count,
                            uint64_t n_samples, uint16_t channels, uint64_t frame_begin,
                            uint64_t frame_end, float *d_coeffs);

/* Host assembly of EncodedAudio from `n_frames` consecutive records (all shards concatenated in
 * frame order): builds the sparse (u16, i16) lists in ascending k (src/codec.rs:303-306) and the
 * header / gapless info (:543-564). */
int glc_frames_from_records(uint32_t sample_rate, uint64_t n_samples, uint16_t channels,
                            const void *records, uint64_t n_frames, glc_frames **out);

/* Same result as glc_frames_from_records, from records still on the device (this context's
 * device; e.g. right after glc_encode_range_device, or on the gather root): the sparse lists are
 * compacted on the device (scan + ballot pack, ascending k) and only the bitstream's payload —
 * (u16, i16) pairs, scale factors, raw planes of raw frames — crosses to the host.  Synchronises. */
int glc_frames_from_device_records(glc_ctx *ctx, const void *d_records, uint64_t n_frames,
                                   uint64_t n_samples, uint16_t channels, glc_frames **out);

/* Compact form of a contiguous frame range: one self-describing blob holding exactly the
 * bitstream's payload for those frames (per-frame raw flags, per-row scale factor and list length,
 * the (u16 index, i16 value) lists of src/codec.rs:303-306 back to back, raw_pcm planes of raw
 * frames) - about 1/8 of the fixed-size records on tonal material.  It is what crosses PCIe after an
 * encode and what a multi-GPU job gathers to its root: every rank compacts its own frame
 * range, the blobs travel (RCCL send/recv or gather, sizes from glc_compact_info.bytes), and the root
 * assembles EncodedAudio from the blobs in frame order.  Layout: DESIGN.md section 3. */
typedef struct glc_compact_info {
  uint64_t n_frames;
  uint64_t n_pairs;    /* total sparse-list entries */
  uint64_t n_raw_rows; /* frame-channels that belong to raw frames */
  uint64_t bytes;      /* size of the blob (what has to travel) */
} glc_compact_info;
/* Capacity a blob buffer needs for any `n_frames` frames of `channels` channels (worst case). */
uint64_t glc_compact_bound(uint16_t channels, uint64_t n_frames);
/* Device-side compaction (scan + ballot pack, ascending k) of `n_frames` records at d_records into
 * the device buffer d_blob (cap >= glc_compact_bound).  Runs on the context's stream and
 * synchronises it (the sizes come back through `info`).  n_frames may be 0 (an empty shard).
 * d_records and d_blob must both be 8-byte aligned (the kernels read rows as 8-byte vectors and write the
 * header as 64-bit words; glc_record_bytes is a multiple of 16, so any frame of an aligned record array
 * is a valid start); a misaligned pointer is refused with GLC_EINVAL before any device work. */
int glc_compact_device_records(glc_ctx *ctx, const void *d_records, uint64_t n_frames, uint16_t channels,
                               void *d_blob, uint64_t cap, glc_compact_info *info);
/* Host twin of the same packing, for records that are already in host memory. */
int glc_compact_records(const void *records, uint64_t n_frames, uint16_t channels, void *blob, uint64_t cap,
                        glc_compact_info *info);
/* Host assembly of EncodedAudio (header + gapless info as src/codec.rs:543-564) from `n_blobs`
 * host-resident blobs (each 8-byte aligned) that together cover the stream's frames in order.  Every
 * count in a blob is validated against its size; GLC_EFORMAT on inconsistency. */
int glc_frames_from_compact(uint32_t sample_rate, uint64_t n_samples, uint16_t channels,
                            const void *const *blobs, const uint64_t *blob_bytes, uint32_t n_blobs,
                            glc_frames **out);

/* ---- decode --------------------------------------------------------------------------- */

/* Length Decoder::decode will return: min(original_length, (n_frames+1)*1024*ch - delay). */
uint64_t glc_decoded_len(const glc_frames *in);

/* Decoder::decode(&mut self, &EncodedAudio, _) -> Result<Vec<f32>>  src/codec.rs:744-768
 * (including decode_streaming :595-741, overlap-add and the gapless trim). */
int glc_decode(glc_ctx *ctx, const glc_frames *in, float *pcm_out, uint64_t cap,
               uint64_t *n_out);

/* Device-resident decode: the whole un-trimmed stream decode_streaming emits ((n_frames + 1) *
 * 1024 * channels samples, src/codec.rs:688-732) is written to the device buffer d_all (capacity
 * cap_all samples); *start / *n_out give the gapless-trimmed window Decoder::decode would return
 * (:756-765) inside it.  Work is queued on glc_ctx_stream(ctx) and NOT synchronised, except for
 * the one-off upload of the sparse rows: a context keeps the rows of the last stream it decoded on
 * the device, so decoding the same glc_frames object again (any glc_decode_* entry point) uploads
 * nothing. */
int glc_decode_device(glc_ctx *ctx, const glc_frames *in, float *d_all, uint64_t cap_all,
                      uint64_t *start, uint64_t *n_out);

/* One shard of the same decode (multi-GPU): hops [hop_begin, hop_end) of the
 * un-trimmed stream, hop_end <= n_frames + 1, written to d_out (hop hop_begin at d_out[0], capacity
 * cap samples).  Hop h is the second half of frame h-1 plus the first half of frame h
 * (src/codec.rs:688-705), hop n_frames the bare overlap tail (:722-729); a range that does not
 * start at 0 recomputes frame hop_begin-1 as its halo, so disjoint ranges decoded on different
 * GPUs concatenate to exactly the whole-stream output.  Queued on the context's stream. */
int glc_decode_range_device(glc_ctx *ctx, const glc_frames *in, uint64_t hop_begin,
                            uint64_t hop_end, float *d_out, uint64_t cap);

/* The inverse transform alone: dequantisation (src/codec.rs:651-665) + MdctTables::imdct_block
 * (:377-390) + window (:672-675) - or the raw-frame path (:626-644) - for every frame-channel of
 * [frame_begin, frame_end) -> d_blocks[(frame-frame_begin)*channels + c][2048] f32, before any
 * overlap-add.  Used for kernel-level timing and as the parity tap of the decode side (the
 * counterpart of glc_mdct_forward_device).  Queued on the context's stream, not synchronised. */
int glc_imdct_device(glc_ctx *ctx, const glc_frames *in, uint64_t frame_begin, uint64_t frame_end,
                     float *d_blocks);

/* Decoder::decode_streaming src/codec.rs:595-741: un-trimmed output delivered in chunks of at
 * least FRAMES_PER_CHUNK*1024*channels samples (AudioChunk, :81-85).  `begin` decodes on the
 * device; `next` copies the next chunk (returns its size through n_out, sets *is_last on the
 * final chunk, which carries the overlap tail :722-732).
 * An open session survives every encode entry point, glc_ctx_set_stream and the debug switches.  Every decode-side
 * call closes it - glc_decode*, glc_decode_batch*, the round-trip, compact, crop and store families - and so does a
 * glc_decode / glc_decode_device / glc_decode_range_device / glc_imdct_device that is refused for its capacity or range
 * (not one refused for a null argument); `next` is then GLC_EINVAL.  A `next` refused for the other sample format
 * leaves the session open. */
int glc_decode_stream_begin(glc_ctx *ctx, const glc_frames *in);
int glc_decode_stream_next(glc_ctx *ctx, float *chunk, uint64_t cap, uint64_t *n_out,
                           int *is_last);

/* ---- container (.glc = bincode 1.x of EncodedAudio) ------------------------------------- */

/* save_encoded / load_encoded src/codec.rs:774-786. */
uint64_t glc_serialized_size(const glc_frames *f);
int glc_serialize(const glc_frames *f, uint8_t *buf, uint64_t cap, uint64_t *written);
int glc_deserialize(const uint8_t *buf, uint64_t len, glc_frames **out);
int glc_save(const glc_frames *f, const char *path);
int glc_load(const char *path, glc_frames **out);
void glc_frames_free(glc_frames *f);

/* ---- EncodedAudio accessors ----------------------------------------------------------- */

int glc_frames_info(const glc_frames *f, glc_info *out);
/* EncodedFrame.raw_pcm.is_some() */
int glc_frame_is_raw(const glc_frames *f, uint64_t frame);
/* EncodedFrame.sparse_coeffs_per_channel[channel]: copies up to cap pairs, returns the list
 * length through n (idx/q may be NULL to query). */
int glc_frame_sparse(const glc_frames *f, uint64_t frame, uint32_t channel, uint16_t *idx,
                     int16_t *q, uint32_t cap, uint32_t *n);
/* EncodedFrame.scale_factors[channel] */
int glc_frame_scale(const glc_frames *f, uint64_t frame, uint32_t channel, float *scale);
/* EncodedFrame.raw_pcm: copies up to cap samples, returns the length through n. */
int glc_frame_raw(const glc_frames *f, uint64_t frame, int16_t *pcm, uint64_t cap, uint64_t *n);

/* ---- EncodedAudio as flat arrays: the structured bridge to the reference's nested Vecs ------- */

/* EncodedAudio (src/codec.rs:31-69) as the flat pools a glc_frames keeps, so that a host fills or
 * reads `Vec<EncodedFrame>` with one slice copy per list and no byte stream in between.  Every Vec of
 * the schema keeps its own length (any well-formed .glc round-trips):
 *   frame f: sparse_coeffs_per_channel = lists  list_begin[f] .. list_begin[f+1]   (indices into list_off)
 *            list l                    = pairs  list_off[l]   .. list_off[l+1]     ((u16 index, i16 value),
 *                                        4 bytes each: index in the low half, the layout of src/codec.rs:303-306
 *                                        written little-endian - what bincode emits for Vec<(u16, i16)>)
 *            scale_factors             = scales scale_begin[f] .. scale_begin[f+1]
 *            raw_pcm                   = None if raw_tag[f] == 0, else raw raw_begin[f] .. raw_begin[f+1]
 * As a VIEW (glc_frames_get_view) the pointers are borrowed from the glc_frames and stay valid until it
 * is freed.  As PARTS (glc_frames_from_parts) they are the caller's arrays, copied by the call. */
typedef struct glc_frames_view {
  uint32_t sample_rate;     /* AudioHeader, src/codec.rs:39-46 */
  uint16_t channels;
  uint16_t reserved;
  uint64_t total_samples;
  uint32_t encoder_delay;   /* GaplessInfo, src/codec.rs:48-53 */
  uint32_t padding;
  uint64_t original_length;
  uint64_t n_frames;
  uint64_t n_lists;         /* all sparse lists of the stream */
  uint64_t n_pairs;
  uint64_t n_scales;
  uint64_t n_raw;           /* i16 samples in the raw pool */
  const uint64_t *list_begin;   /* [n_frames + 1] */
  const uint64_t *list_off;     /* [n_lists + 1]  */
  const uint32_t *pairs;        /* [n_pairs]      */
  const uint64_t *scale_begin;  /* [n_frames + 1] */
  const float *scales;          /* [n_scales]     */
  const uint8_t *raw_tag;       /* [n_frames]     */
  const uint64_t *raw_begin;    /* [n_frames + 1] */
  const int16_t *raw;           /* [n_raw]        */
} glc_frames_view;

/* Borrow the pools of `f` (≙ reading the EncodedAudio that Encoder::encode returned, src/codec.rs:421). */
int glc_frames_get_view(const glc_frames *f, glc_frames_view *out);

/* Build an EncodedAudio from flat arrays (≙ the `&EncodedAudio` Decoder::decode takes, src/codec.rs:744).
 * Every offset is validated (monotonic, inside its pool); GLC_EFORMAT otherwise.  `stream_id`: 0, or a
 * caller-chosen identity < 2^63 of this stream's CONTENT - the caller promises that two objects built
 * with the same non-zero id hold the same stream.  A context recognises the id of the stream whose
 * sparse rows (and inverse-transform plan) it still holds on the device and decodes it again without
 * preparing or uploading anything (glc_ctx_resident_stream). */
int glc_frames_from_parts(const glc_frames_view *parts, uint64_t stream_id, glc_frames **out);

/* The same constructor for a host whose lists live in separate allocations (the reference's
 * Vec<Vec<(u16, i16)>>): pointer + length per list, per-frame scale and raw vectors by pointer; the
 * payload is copied once, straight into the pools.  list l of frame f is lists[Σ_{g<f} lists_per_frame[g] + l]. */
typedef struct glc_frames_gather {
  uint32_t sample_rate;
  uint16_t channels;
  uint16_t reserved;
  uint64_t total_samples;
  uint32_t encoder_delay;
  uint32_t padding;
  uint64_t original_length;
  uint64_t n_frames;
  const uint32_t *lists_per_frame;   /* [n_frames]                sparse_coeffs_per_channel.len() */
  const void *const *list_ptr;       /* [Σ lists_per_frame]       pointer to the list's 4-byte pairs */
  const uint32_t *list_len;          /* [Σ lists_per_frame]       pairs in the list */
  const uint32_t *scales_per_frame;  /* [n_frames]                scale_factors.len() */
  const float *const *scale_ptr;     /* [n_frames] */
  const int16_t *const *raw_ptr;     /* [n_frames]                NULL = raw_pcm: None */
  const uint64_t *raw_len;           /* [n_frames] */
} glc_frames_gather;
int glc_frames_from_gather(const glc_frames_gather *g, uint64_t stream_id, glc_frames **out);

/* Identity of a glc_frames: the stream_id it was built with (glc_frames_from_parts / _gather), or a
 * process-unique number >= 2^63 for objects the library built itself. */
uint64_t glc_frames_stream_id(const glc_frames *f);
/* Identity of the stream whose sparse rows `ctx` holds on the device (0: none). */
uint64_t glc_ctx_resident_stream(const glc_ctx *ctx);
/* Decoder::decode of the resident stream, without a glc_frames: for a host that has recognised the
 * stream by its id and so need not flatten its nested vectors again.  GLC_EINVAL if `stream_id` is not
 * the resident stream (then build the glc_frames and call glc_decode). */
int glc_decode_resident(glc_ctx *ctx, uint64_t stream_id, float *pcm_out, uint64_t cap, uint64_t *n_out);

/* Encoder::encode with a hook: `fn(user, view, frame_begin, frame_end)` is called each time the frames
 * [frame_begin, frame_end) have arrived on the host (ranges ascend and tile [0, n_frames)), while the
 * device still works on later frames - where a host builds its nested EncodedFrame vectors, hidden
 * behind the rest of the encode instead of after it.  The calls are made on the calling thread, in the
 * time it would otherwise spend blocked on the device (ranges of a few dozen frames while it polls,
 * the remainder at the end).  `view` covers frames [0, frame_end) and is valid only during the call.
 * A non-zero return aborts the encode (GLC_EINVAL).  `out` may be NULL when the hook has taken
 * everything it needs. */
typedef int (*glc_frames_hook)(void *user, const glc_frames_view *view, uint64_t frame_begin, uint64_t frame_end);
int glc_encode_hooked(glc_ctx *ctx, const float *pcm, uint64_t n_samples, uint16_t channels,
                      glc_frames_hook fn, void *user, glc_frames **out);

/* ---- WAV file I/O twin (src/audio.rs; host only, no device) ---------------------------------- */

/* load_wav src/audio.rs:39-64: RIFF/WAVE PCM (8/16/24/32-bit integer -> s / 2^(bits-1), 8-bit is
 * unsigned in the file) and 32-bit IEEE float (passed through), incl. WAVE_FORMAT_EXTENSIBLE.
 * Returns a malloc'd interleaved buffer; release it with glc_free. */
int glc_wav_load(const char *path, float **samples, uint64_t *n_samples, uint32_t *sample_rate,
                 uint16_t *channels);
/* export_to_wav src/audio.rs:100-132: 16-bit PCM, (s * 32767).clamp(-32768, 32767) as i16. */
int glc_wav_save16(const char *path, const float *samples, uint64_t n_samples, uint32_t sample_rate,
                   uint16_t channels);
void glc_free(void *p);

/* ---- FLAC file I/O twin (src/flac.rs, src/audio.rs:68-96; host only, no device) ----------- */

/* encode_flac_with_level src/flac.rs:947-1053 (encode_flac :1056-1063 is level 5): the reference's
 * own encoder, byte for byte - 16-bit, (s * 32767).clamp(-32768, 32767) as i16, block 1152
 * (levels 0-2) or 4096, verbatim (level 0) or fixed predictor of order 1/2/3/3/4.. by level,
 * partitioned Rice with 4-bit parameters, independent channels, STREAMINFO with the MD5 of the
 * samples.  GLC_EINVAL for < 16 samples per channel, level > 8 (the reference's two Err cases)
 * and channels == 0 (a division by zero there).  *out is malloc'd; release it with glc_free. */
int glc_flac_encode(const float *samples, uint64_t n_samples, uint32_t sample_rate,
                    uint16_t channels, uint8_t level, uint8_t **out, uint64_t *out_len);
/* export_to_flac_with_level src/flac.rs:1066-1077 (export_to_flac :1080-1087 is level 5). */
int glc_flac_save(const char *path, const float *samples, uint64_t n_samples, uint32_t sample_rate,
                  uint16_t channels, uint8_t level);
/* load_flac src/audio.rs:68-85 (the reference delegates to the claxon crate): any RFC 9639
 * stream - constant / verbatim / fixed / LPC subframes, left-side / side-right / mid-side stereo,
 * both Rice code books, wasted bits - with both CRCs checked; samples become s / 2^(bits-1).
 * Returns a malloc'd interleaved buffer; release it with glc_free. */
int glc_flac_load(const char *path, float **samples, uint64_t *n_samples, uint32_t *sample_rate,
                  uint16_t *channels);
int glc_flac_decode(const uint8_t *buf, uint64_t len, float **samples, uint64_t *n_samples,
                    uint32_t *sample_rate, uint16_t *channels);

/* ---- integer PCM at the host boundary -------------------------------------------------------- */

/* The reference's program only ever feeds its encoder samples widened from an integer file
 * (load_wav / load_flac: `s as f32 / (1 << (bits-1)) as f32`, src/audio.rs:52-60, :72-81) and narrows
 * what its decoder returns to 16 bits straight away (convert_f32_to_i16, src/audio.rs:11-16,
 * src/flac.rs:955-958).  The entry points below do both conversions on the device, bit for bit, so
 * that 2 bytes per sample cross PCIe instead of 4 and the host never walks the audio. */
typedef enum glc_pcm_format {
  GLC_PCM_S16 = 1, /* int16_t samples, bits 1..16 */
  GLC_PCM_S32 = 2, /* int32_t samples, bits 1..32, the value sign-extended in the container */
  GLC_PCM_F32 = 3  /* float samples, already widened (`bits` is ignored) */
} glc_pcm_format;

/* out[i] = (float)in[i] / max, max = 2^(bits-1) - and -2^31 for bits == 32: the reference shifts an
 * i32 literal into its sign bit and so inverts 32-bit files (quirk Q11, kept).  d_in: n samples in
 * device memory, aligned to their size; d_out: n floats.  GLC_PCM_F32 is a device-to-device copy.
 * Queued on glc_ctx_stream(ctx), not synchronised. */
int glc_pcm_widen_device(glc_ctx *ctx, const void *d_in, glc_pcm_format fmt, uint32_t bits, uint64_t n,
                         float *d_out);
/* glc_encode of the samples load_wav / load_flac would have produced from these integers - the same
 * frames - without the float copy: the integers are uploaded and widened on the device. */
int glc_encode_int(glc_ctx *ctx, const void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples,
                   uint16_t channels, glc_frames **out);
/* convert_f32_to_i16(Decoder::decode(..)): what glc_decode returns, narrowed by
 * `(s * 32767.0).clamp(-32768.0, 32767.0) as i16` (NaN gives 0) on the device. */
int glc_decode_i16(glc_ctx *ctx, const glc_frames *in, int16_t *pcm_out, uint64_t cap, uint64_t *n_out);
/* glc_decode_range_device with the same narrowing; d_out is any 2-byte aligned device pointer. */
int glc_decode_range_device_i16(glc_ctx *ctx, const glc_frames *in, uint64_t hop_begin, uint64_t hop_end,
                                int16_t *d_out, uint64_t cap);
/* glc_decode_stream_next with the same narrowing, after the same glc_decode_stream_begin.  A stream
 * is read through one of the two calls from its first chunk to its last: mixing them is GLC_EINVAL. */
int glc_decode_stream_next_i16(glc_ctx *ctx, int16_t *chunk, uint64_t cap, uint64_t *n_out, int *is_last);

/* load_audio_file_lossless (src/audio.rs:19-36: .wav or .flac by lower-cased extension) before the
 * widening: integer sources of at most 16 bits come back as GLC_PCM_S16 (8-bit WAV made signed), wider
 * ones as GLC_PCM_S32, float WAV as GLC_PCM_F32 (*bits = 32).  *samples is malloc'd (glc_free). */
int glc_audio_load_pcm(const char *path, void **samples, glc_pcm_format *fmt, uint32_t *bits,
                       uint64_t *n_samples, uint32_t *sample_rate, uint16_t *channels);
/* glc_wav_save16 / glc_flac_encode / glc_flac_save of samples that are 16-bit already. */
int glc_wav_save16_i16(const char *path, const int16_t *samples, uint64_t n_samples, uint32_t sample_rate,
                       uint16_t channels);
int glc_flac_encode_i16(const int16_t *samples, uint64_t n_samples, uint32_t sample_rate, uint16_t channels,
                        uint8_t level, uint8_t **out, uint64_t *out_len);
int glc_flac_save_i16(const char *path, const int16_t *samples, uint64_t n_samples, uint32_t sample_rate,
                      uint16_t channels, uint8_t level);

/* ---- batches of short clips ------------------------------------------------------------ */

/* Encoder::encode of n_clips independent streams of `channels` channels at the context's sample rate
 * in one call: whole clips are packed into rounds of one launch chain each, instead of one chain, one
 * upload and one download per clip.  out[i] receives an owned glc_frames, byte-identical
 * (glc_serialize) to what glc_encode returns for clip i alone.  n_clips == 0 is GLC_OK.  A clip that
 * glc_encode refuses (glc_plan_encode gives it 0 frames; a null pointer) or channels == 0 fails the
 * whole call with GLC_EINVAL - the message names the clip - and leaves every out[i] NULL. */
int glc_encode_batch(glc_ctx *ctx, const float *const *pcm, const uint64_t *n_samples, uint64_t n_clips,
                     uint16_t channels, glc_frames **out);

/* Decoder::decode of n_streams streams into ONE packed buffer: stream i's trimmed samples are
 * pcm_out[offsets[i] .. offsets[i+1]), bit-identical to glc_decode of it alone; offsets has
 * n_streams + 1 entries, offsets[0] == 0, and is filled whenever the arguments are non-null (the
 * running sums of glc_decoded_len), so cap == 0 sizes the buffer: GLC_EINVAL "output buffer too small".
 * Nothing behind offsets[n_streams] is written.  All streams must have the same header.channels
 * (GLC_EINVAL); their sample rates may differ.  A malformed stream fails the whole call (GLC_EFORMAT).
 * Afterwards no stream is resident on the context (glc_ctx_resident_stream is 0) and an open
 * glc_decode_stream_* session is closed.  n_streams == 0 is GLC_OK. */
int glc_decode_batch(glc_ctx *ctx, const glc_frames *const *in, uint64_t n_streams, float *pcm_out, uint64_t cap,
                     uint64_t *offsets);

/* glc_encode_batch of integer clips: one `fmt` and one `bits` for the whole call (as `channels` is one for
 * the whole call; callers group).  out[i] is byte-identical to glc_encode_int(ctx, pcm[i], fmt, bits,
 * n_samples[i], channels) - and so to glc_encode / glc_encode_batch of the widened floats.  The integers are
 * what is staged and uploaded; the device widens a whole round in one pass.  pcm[i] is aligned to its sample
 * size.  GLC_PCM_F32 forwards to glc_encode_batch; fmt / bits are validated as glc_encode_int validates them
 * (GLC_EINVAL).  Every rule of glc_encode_batch holds unchanged. */
int glc_encode_batch_int(glc_ctx *ctx, const void *const *pcm, glc_pcm_format fmt, uint32_t bits,
                         const uint64_t *n_samples, uint64_t n_clips, uint16_t channels, glc_frames **out);

/* glc_decode_batch writing 16-bit PCM: the same contract with int16_t elements (offsets in samples), stream
 * i's span equal to glc_decode_i16 of it alone - narrowed on the device by the batch overlap-add itself.
 * pcm_out is any 2-byte aligned host pointer. */
int glc_decode_batch_i16(glc_ctx *ctx, const glc_frames *const *in, uint64_t n_streams, int16_t *pcm_out,
                         uint64_t cap, uint64_t *offsets);

/* ---- round trip: what the codec does to audio, without a stream on the host ---------------- */

/* The reference's own tests are "encode, decode, compare" (tests/test_codec.rs), and a lossy codec is a
 * degradation stage for whoever trains on audio: PCM in, degraded PCM out.  After an encode the frame
 * records are in device memory and hold everything the decoder reads, so the calls below build the
 * decoder's row tables from them ON THE DEVICE (one small kernel per round of 4096 frames) instead of
 * compacting, downloading, assembling an EncodedAudio, walking it and uploading its rows again.  Their
 * samples are bit for bit those of glc_decode(glc_encode(..)).
 * All of them leave no stream resident on the context (glc_ctx_resident_stream is 0) and close an open
 * glc_decode_stream_* session - the rule of glc_decode_batch.  Workspaces are sized by the round, not by
 * the stream; a call that has to grow one synchronises the stream for that, a call that finds them
 * large enough only queues. */

/* Decoder::decode of the stream that `n_frames` records at d_records describe (device memory of this
 * context's device, 16-byte aligned, layout: glc_record_bytes; n_samples gives original_length as in
 * glc_frames_from_device_records, whose EncodedAudio this decodes - where a record's nnz field and its
 * dense row disagree, the first min(nnz, 1024) non-zeros count, as there).  The gapless-trimmed samples
 * go to device memory at d_out[0 .. *n_out) (any 4-byte aligned pointer); nothing behind them is
 * written.  *n_out is arithmetic: min(original_length, (n_frames + 1) * 1024 * channels - delay).
 * Queued on glc_ctx_stream(ctx) and NOT synchronised; nothing is copied to the host.
 * GLC_EINVAL: a null or misaligned pointer, a record count that does not match the stream length,
 * cap < *n_out ("output buffer too small", *n_out filled). */
int glc_decode_device_records(glc_ctx *ctx, const void *d_records, uint64_t n_frames, uint64_t n_samples,
                              uint16_t channels, float *d_out, uint64_t cap, uint64_t *n_out);

/* Encoder::encode + Decoder::decode of device-resident interleaved PCM into device-resident PCM:
 * d_out[0 .. *n_out) = glc_decode(glc_encode(d_pcm[0 .. n_samples))), *n_out == n_samples for every
 * input the encoder accepts.  Rounds of at most 4096 frames - transform, quantiser, row tables, inverse
 * transform, overlap-add - with the overlap carried from round to round as the streaming decode
 * carries it.  Entirely queued on glc_ctx_stream(ctx), NOT synchronised, no copy to the host.  d_pcm and
 * d_out must not overlap.  Errors as glc_encode and as above. */
int glc_roundtrip_device(glc_ctx *ctx, const float *d_pcm, uint64_t n_samples, uint16_t channels, float *d_out,
                         uint64_t cap, uint64_t *n_out);

/* The same at the host boundary: the samples go up once and come down once (round by round, beside the
 * kernels of the neighbouring rounds).  fmt / bits: as glc_encode_int (GLC_PCM_F32: plain floats).
 * out_fmt: GLC_PCM_F32 (pcm_out holds floats: what glc_decode returns) or GLC_PCM_S16 (int16_t: what
 * glc_decode_i16 returns, narrowed on the device by the overlap-add); anything else is GLC_EINVAL.
 * cap counts samples of the output format.  Synchronises before it returns. */
int glc_roundtrip(glc_ctx *ctx, const void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples,
                  uint16_t channels, void *pcm_out, glc_pcm_format out_fmt, uint64_t cap, uint64_t *n_out);

/* What the last glc_roundtrip_device / glc_roundtrip on this context encoded, from a device reduction
 * over the record headers: the counts glc_frames_info gives for glc_encode of the same samples, and
 * serialized_bytes == glc_serialized_size of it - the bitrate without the stream.  Synchronises the
 * context's stream.  GLC_EINVAL when no round trip has completed on this context.  The record is that of the last
 * COMPLETED call of the two: calls of every other family, glc_decode_device_records (it encodes nothing) and calls
 * refused by an argument check leave it as it is ("What a call leaves on its context"). */
typedef struct glc_roundtrip_info {
  uint64_t n_frames;
  uint64_t n_raw_frames;
  uint64_t total_nnz;
  uint64_t serialized_bytes;
} glc_roundtrip_info;
int glc_roundtrip_last_info(glc_ctx *ctx, glc_roundtrip_info *out);

/* ---- round trip of a batch of device-resident clips, any layout --------------------------- */

/* Where the clips of a batch lie in ONE device buffer, in elements (floats) from its start: clip i begins
 * at i * clip_stride.  Interleaved (planar == 0): sample t of channel c of a clip at t * channels + c.
 * Planar: at c * channel_stride + t - a (B, C, T) tensor, or any slice of one whose innermost stride is 1.
 * Clip i has lengths[i] samples per channel (`length` each when lengths == NULL); what lies behind them,
 * between the planes and between the clips belongs to the caller and is neither read nor written. */
typedef struct glc_clip_layout {
  uint64_t n_clips;
  uint16_t channels;
  int      planar;          /* 0: a clip is [t][c] interleaved; 1: [c][t], one plane per channel */
  uint64_t clip_stride;     /* elements from clip i to clip i+1 */
  uint64_t channel_stride;  /* planar: elements from plane c to plane c+1 of a clip; ignored otherwise */
  uint64_t length;          /* per-channel samples of every clip when lengths == NULL */
  const uint64_t *lengths;  /* host array [n_clips] of per-channel samples, or NULL */
} glc_clip_layout;

/* glc_roundtrip_device of every clip of a batch in one call: for every clip i the lengths[i] * channels
 * samples of clip i in `out` are bit for bit glc_decode(glc_encode(clip i of `in`)), and NO other element of
 * d_out is written.  `out` may differ from `in` in `planar` and in the strides; n_clips, channels and the
 * lengths must agree.  d_out == d_pcm with the same layout runs in place; any other overlap of the two
 * extents is GLC_EINVAL (the extent of a layout is that of the padded batch: (n_clips - 1) * clip_stride plus
 * what a clip of the longest length occupies, so the padding behind a short last clip is part of it).  Offsets are 64-bit: a layout may span more than 2^32 elements.
 * Whole clips are packed into rounds of at most 4096 frames (8192 for mono) - one gather, one transform,
 * one quantiser, one row-table, one inverse-transform and one overlap-add launch chain per ROUND, whatever
 * the number of clips; a clip longer than a round is staged whole and goes through the rounds of
 * glc_roundtrip_device.  Queued on glc_ctx_stream(ctx), NOT synchronised, nothing is copied to the host.
 * The call blocks on the host only where a workspace has to grow (the rule above) and until the small
 * table upload of the previous batch call has left its pinned staging memory; it waits for no kernel of
 * that call.  Afterwards no stream is resident and an open decode session is closed.
 * GLC_EINVAL, checked before anything is queued: a null pointer, channels == 0, a clip the encoder refuses
 * (<= 512 samples per channel; the message names the clip), a stride smaller than what a clip or plane
 * occupies, layouts that do not match.  n_clips == 0 is GLC_OK. */
int glc_roundtrip_batch_device(glc_ctx *ctx, const float *d_pcm, const glc_clip_layout *in, float *d_out,
                               const glc_clip_layout *out);

/* glc_roundtrip_last_info for every clip of the last glc_roundtrip_batch_device on this context:
 * infos[i] is what glc_roundtrip_last_info gives after glc_roundtrip_device of clip i alone, from per-clip
 * device counters.  Synchronises the context's stream.  GLC_EINVAL when no batch round trip has completed
 * on this context or n_clips is not that call's.  Calls of other families, refused calls and a call with n_clips == 0
 * leave the record of the last completed batch call as it is. */
int glc_roundtrip_batch_last_info(glc_ctx *ctx, glc_roundtrip_info *infos, uint64_t n_clips);

/* ---- decode of compact blobs that are in device memory: a compressed clip store in HBM ------ */

/* The compact blob (glc_compact_device_records, glc_compact_records, glc_frames_to_compact) is the form of a
 * stream that is as small as the bitstream, and it is almost the decoder's row table already.  The calls below
 * decode blobs where they lie: one small device pass (R2: the header check, two scans, one wave per row that
 * checks the row's bounds and that its list ascends strictly below 1024) builds the row tables around the
 * payload, which is not copied.  A corpus of clips can so be kept in device memory at bitstream size and any
 * selection of it decoded into a (B, C, T) tensor with no host in the loop.
 * A blob is untrusted: a header that does not pass glc_frames_from_compact's check (magic, channels, exactly
 * the frame count n_samples gives, counts its rows can hold, `bytes` exactly the sum of the sections and
 * <= blob_bytes) decodes as silence and is read no further; a row whose list leaves the pair pool, is longer
 * than 1024 or is not strictly ascending below 1024, and the rows of a raw frame whose planes the blob does
 * not hold, decode as an empty list.  No load leaves [blob, blob + blob_bytes).  glc_decode_compact_last_status
 * says what was found; the calls themselves return GLC_OK (nothing comes back to the host).
 * d_blob must be 64-byte aligned (every section then keeps the alignment it has inside the blob), blob_bytes
 * at least the fixed sections of a blob of that many frames.  The family's rules hold: no stream is resident
 * afterwards, an open decode session is closed, a call synchronises only where a workspace has to grow. */

/* Decoder::decode of the stream ONE compact blob in device memory holds (all its frames, in order): the samples
 * of glc_decode(glc_frames_from_compact(sample_rate, n_samples, channels, blob)) bit for bit, gapless-trimmed,
 * at d_out[0 .. *n_out); nothing behind them is written.  n_samples gives the header as in
 * glc_frames_from_compact.  Queued on glc_ctx_stream(ctx), NOT synchronised, nothing is copied to the host.
 * The row tables take 32 bytes per row of the stream.
 * GLC_EINVAL, before anything is queued: a null or misaligned pointer, channels == 0, an n_samples the encoder
 * refuses, blob_bytes too small, cap < *n_out (*n_out filled), an output that overlaps the blob. */
int glc_decode_device_compact(glc_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint64_t n_samples,
                              uint16_t channels, float *d_out, uint64_t cap, uint64_t *n_out);

/* The same for n_clips blobs, one per clip, into ONE strided device buffer described by a glc_clip_layout
 * (out->lengths[i] * channels must be n_samples[i], the decoded length of clip i): whole clips packed into rounds
 * as glc_decode_batch packs them, one R2, one inverse-transform and one strided overlap-add launch chain per ROUND
 * whatever the number of clips; a clip longer than a round goes through the rounds of the single call.
 * No element of d_out outside the clips' true samples is written.  The blobs may lie anywhere in device memory.
 * GLC_EINVAL as above, and for a layout whose strides are too small or whose extent overlaps a blob.
 * n_clips == 0 is GLC_OK. */
int glc_decode_batch_device_compact(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes,
                                    const uint64_t *n_samples, float *d_out, const glc_clip_layout *out);

/* What R2 found in the last of the two calls above (or of glc_decode_crops_device_compact / glc_decode_crops_device_store below): per clip the flag word, the number of rejected rows and
 * the first of them (row = frame * channels + channel; 0 when none was rejected).  A bad header rejects every
 * row.  The two SUM flags are reported only: they reject nothing.  Synchronises the context's stream.
 * GLC_EINVAL when no such call has completed on this context or n_clips is not that call's.  The words are those of the
 * last completed call ALONE (every call starts its counters from zero); calls of other families, refused calls and
 * calls with n_clips == 0 leave them as they are. */
#define GLC_COMPACT_BAD_HEADER    1u  /* the header check failed: the clip is silence */
#define GLC_COMPACT_ROW_BOUNDS    2u  /* a row longer than 1024 or reaching behind n_pairs */
#define GLC_COMPACT_NOT_CANONICAL 4u  /* a list that is not strictly ascending below 1024 */
#define GLC_COMPACT_RAW_RANGE     8u  /* a raw frame whose planes the blob does not hold */
#define GLC_COMPACT_PAIR_SUM     16u  /* the rows' counts do not add up to n_pairs */
#define GLC_COMPACT_RAW_SUM      32u  /* the rows of raw frames are not n_raw_rows */
typedef struct glc_compact_status { uint32_t flags; uint32_t reserved; uint64_t n_bad_rows; uint64_t first_bad_row; } glc_compact_status;
int glc_decode_compact_last_status(glc_ctx *ctx, glc_compact_status *status, uint64_t n_clips);

/* ---- windows of stored clips: crops of compact blobs ---------------------------------------- */

/* A window of a decoded clip, in samples PER CHANNEL: [start, start + length). */
typedef struct glc_crop { uint64_t start, length; } glc_crop;

/* Host only: what a crop of a clip of n_samples interleaved samples needs of the clip's stream - the frames
 * [first_frame, first_frame + n_frames) (the frame in front of the first kept hop included: its second half
 * overlaps into that hop; no frame for the bare tail hop) and the hops [first_hop, first_hop + n_hops) of the
 * un-trimmed stream, from the hop of the first kept sample to the hop of the last one.  The crop lies at the
 * un-trimmed interleaved positions [512 + start * channels, 512 + (start + length) * channels): the encoder's delay
 * counts interleaved samples.  glc_decode_crops_device_compact plans with this function.
 * GLC_EINVAL: a null pointer, an n_samples / channels the encoder refuses, length == 0, start + length beyond the
 * clip's samples per channel. */
typedef struct glc_crop_plan { uint64_t first_frame, n_frames, first_hop, n_hops; } glc_crop_plan;
int glc_plan_crop(uint64_t n_samples, uint16_t channels, const glc_crop *crop, glc_crop_plan *out);

/* A batch of windows of stored clips in one call: entry i is the interleaved samples [crops[i].start * channels,
 * (crops[i].start + crops[i].length) * channels) of what glc_decode_device_compact gives for d_blobs[i] (blob_bytes[i],
 * n_samples[i]) - bit for bit, for every content of the blob, damaged ones included - written as clip i of `out`
 * (any glc_clip_layout; out->lengths[i], or out->length, must be crops[i].length).  No other element of d_out is
 * written.  The same blob may appear any number of times and the blobs may lie in any address order.
 * Only the frames glc_plan_crop names go through the inverse transform, and only their rows get a row table (32
 * bytes per WINDOW row): the pairs and raw planes in front of a window are found by a reduction over the cnt and
 * is_raw sections of the rows in front, nothing behind a window is read.  Crops are packed into rounds as
 * glc_decode_batch_device_compact packs clips, each counting its window's frames + 1; one launch chain per ROUND
 * whatever the number of crops; a window of more frames than a round goes through the rounds of the single call,
 * restricted to its frames.  Queued on glc_ctx_stream(ctx), NOT synchronised, nothing is copied to the host.
 * Untrusted blobs: the header check is that of the calls above (a blob that fails gives +0.0); a window's rows are
 * kept or rejected by the rules above.  Rows outside the window's frames are not validated and cannot affect the
 * crop, except through their cnt / is_raw in front of the window, which move the origins of its lists and planes
 * exactly as they do in the whole-blob call.  No load leaves [blob, blob + blob_bytes).
 * glc_decode_compact_last_status afterwards: one status per CROP; n_bad_rows and first_bad_row count the window's
 * rows, in the stream's row numbering (a bad header: all rows of the window, and the first of them - which the
 * status cannot tell from "none" when that row is 0 and the flag is not looked at).  GLC_COMPACT_PAIR_SUM and
 * GLC_COMPACT_RAW_SUM are NEVER set by this call: it does not read behind the window.
 * GLC_EINVAL, before anything is queued: everything glc_decode_batch_device_compact refuses (but the layout's lengths
 * are the crops'), length == 0, start + length beyond the clip's samples per channel, a layout length that is not
 * the crop's, an output extent that overlaps a blob.  n_clips == 0 is GLC_OK.  The family's rules hold. */
int glc_decode_crops_device_compact(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes,
                                    const uint64_t *n_samples, const glc_crop *crops,
                                    float *d_out, const glc_clip_layout *out);

/* Host only: the compact blob of a whole stream, the inverse of glc_frames_from_compact - the bytes
 * glc_compact_records gives for the records of that stream (padding zeroed), so that a .glc file can be put into
 * a device store with one upload.  cap >= info->bytes is enough (glc_compact_bound is always enough); blob must be
 * 8-byte aligned.  Rows of raw frames get scale 0.0f and cnt 0: EncodedAudio holds neither for them and no decoder
 * reads them (a blob packed from the ENCODER's records keeps the quantiser's scale there - the only bytes in which
 * the two can differ).  GLC_EINVAL (glc_last_error(NULL) says why) for a stream a blob cannot hold - a frame whose vectors
 * are not exactly `channels` lists and `channels` scales, a raw frame that is not 2048 * channels samples, a list
 * that is not strictly ascending below 1024 - and when cap is too small, with info->bytes filled. */
int glc_frames_to_compact(const glc_frames *f, void *blob, uint64_t cap, glc_compact_info *info);

/* ---- encode of a batch of device-resident clips into per-clip compact blobs: filling the store -- */

/* What the device says about clip i of glc_encode_batch_device_compact. */
typedef struct glc_store_entry {   /* 32 bytes, written by the device */
  uint64_t offset;      /* of the clip's blob from d_arena, a multiple of 64 */
  uint64_t bytes;       /* size of the blob (its header's `bytes`) */
  uint64_t n_pairs;
  uint32_t n_raw_rows;
  uint32_t stored;      /* 1: the blob is in the arena; 0: it did not fit, nothing of it was written */
} glc_store_entry;

/* Sum of glc_compact_bound over the clips of a layout: an arena of that many bytes holds them all from cursor 0.
 * Saturates at UINT64_MAX; 0 for a null layout, channels == 0 or a clip the encoder refuses. */
uint64_t glc_compact_store_bound(const glc_clip_layout *in);

/* glc_encode_range_device + glc_compact_device_records of every clip of a batch (any glc_clip_layout) in one call,
 * the write side of the store: the blob of clip i holds exactly the bytes those two calls give for clip i alone -
 * the single-stream compact blob of its frames, padding zeroed, rows of raw frames with the quantiser's scale -
 * so glc_decode_device_compact, glc_decode_batch_device_compact and glc_frames_from_compact read it as it stands.
 * Placement is the device's: *d_cursor (a device uint64_t the caller owns, 8-byte aligned) is the first free byte
 * of the arena.  Every round reads it, rounds it up to 64 and places its clips in clip order, clip i at the
 * exclusive running sum of the blob sizes (each a multiple of 64), and leaves the cursor at the end of that sum:
 * offsets ascend with i across rounds and calls, and consecutive calls with the same cursor append with no
 * synchronisation between them.  A clip is stored when offset + bytes <= arena_bytes.  The cursor keeps
 * counting whether or not a clip was stored, so the stored clips are a prefix of everything ever appended, the
 * entry of a clip that was not stored still reports the offset and size it would have had (stored == 0), and the
 * final cursor is the arena size that would have sufficed.  No byte of the arena outside the stored blobs is
 * written, no element of d_pcm outside the clips' true samples is read (padding may hold NaN).
 * d_entries[i] (device, 8-byte aligned, in->n_clips of them) is written for every clip.
 * Rounds as in glc_roundtrip_batch_device: one gather, one transform and quantiser chain and three pack launches
 * per ROUND whatever the number of clips; a clip longer than a round is staged whole, encoded into a records
 * workspace of n_frames * glc_record_bytes and packed as a round of its own.  Queued on glc_ctx_stream(ctx), NOT
 * synchronised, nothing is copied to the host; the call blocks only where a workspace has to grow and on the
 * pinned table image of the previous batch call.  Afterwards no stream is resident and an open decode session is
 * closed.
 * GLC_EINVAL, before anything is queued: a null pointer, d_arena not 64-byte aligned, d_cursor / d_entries not
 * 8-byte aligned, what glc_roundtrip_batch_device refuses of a layout (the message names the clip), an arena or
 * entries range that overlaps the input extent.  n_clips == 0 is GLC_OK and leaves the cursor alone. */
int glc_encode_batch_device_compact(glc_ctx *ctx, const float *d_pcm, const glc_clip_layout *in,
                                    void *d_arena, uint64_t arena_bytes,
                                    uint64_t *d_cursor, glc_store_entry *d_entries);

/* ---- drawing crops from the store by device-side index and start ---------------------------- */

/* Two more status flags, set only by glc_decode_crops_device_store and glc_decode_ragged_crops_device_store (which
 * has its own rule for a usable selection), always together with GLC_COMPACT_BAD_HEADER. */
#define GLC_COMPACT_NO_BLOB   64u   /* the entry holds no usable blob: stored == 0, offset not a multiple of 64,
                                       or [offset, offset + bytes) not inside the arena */
#define GLC_COMPACT_BAD_CROP 128u   /* the selection is unusable: clip index outside [0, n_entries), a stored length
                                       the encoder refuses or above max_length, start < 0, start + length beyond the clip */

/* Host only: the slots a crop of `length` samples per channel needs wherever it starts - the most hops
 * (glc_plan_crop's n_hops) and frames (n_frames) any start gives in any clip:
 *   max_hops = floor((1024 ch - ch + 512 % ch + length ch - 1) / (1024 ch)) + 1,  max_frames = max_hops + 1.
 * A crop begins at the un-trimmed interleaved position 512 + start * ch, which is 512 modulo ch: 1024 ch - ch + 512 % ch
 * is the latest place in a hop it can have.  Both bounds are reached by some start of every clip long enough.
 * GLC_EINVAL: a null pointer, channels == 0, length == 0, a length * channels that wraps. */
int glc_store_crop_slots(uint64_t length, uint16_t channels, uint64_t *max_hops, uint64_t *max_frames);

/* Crops of ONE length drawn from a store as its write side left it, selected by DEVICE data: crop i of out->n_clips
 * is samples [d_starts[i], d_starts[i] + length) per channel of stored clip d_clips[i].  d_arena / arena_bytes: the
 * arena; d_entries[n_entries]: its index - what glc_encode_batch_device_compact wrote, concatenated over any number
 * of calls, or entries a host built for blobs it uploaded itself; d_lengths[e]: samples per channel of stored clip e
 * (the blob does not hold it); max_length: a host upper bound of those lengths.  All four index arrays are int64_t
 * / 32-byte entries on the device, 8-byte aligned, and none is read by the host.
 * For every crop whose entry and selection are usable, clip i of `out` is bit for bit what
 * glc_decode_crops_device_compact writes for d_blobs[i] = d_arena + entry.offset, blob_bytes[i] = entry.bytes,
 * n_samples[i] = d_lengths[clip] * channels, crops[i] = {start, length} - damaged blobs included - and
 * glc_decode_compact_last_status gives the same words.  A crop whose entry (GLC_COMPACT_NO_BLOB) or selection
 * (GLC_COMPACT_BAD_CROP; it wins when both apply, the entry of an index out of range is not read) is unusable is
 * +0.0 over its length * channels samples, with status flags = that bit | GLC_COMPACT_BAD_HEADER, n_bad_rows = 0,
 * first_bad_row = 0; its neighbours are not affected.  No element of d_out outside the crops is written.  No load
 * leaves the arena, d_entries[0 .. n_entries), d_lengths[0 .. n_entries) or the two selection arrays, whatever they
 * hold.
 * Every crop owns a fixed block of glc_store_crop_slots(length) table rows, block slots and hop descriptors, so the
 * rounds - floor(4097 / (max_frames + 1)) crops each - and every launch depend on n_clips, length and channels alone.
 * One planner kernel per call resolves the selection on the device; then one windowed R2, inverse-transform and
 * overlap-add chain per round.  Queued on glc_ctx_stream(ctx), NOT synchronised.  The call makes NO host-to-device
 * copy, does not wait for the pinned table image of earlier batch calls, and its host work does not depend on
 * n_clips apart from the launches of ceil(n_clips / crops per round) chains; it blocks only where a workspace has
 * to grow.  Afterwards no stream is resident and an open decode session is closed.
 * GLC_EINVAL, before anything is queued: a null pointer, channels == 0, d_arena not 64-byte aligned, an index array
 * not 8-byte aligned, length == 0, max_length < length, a max_length the encoder refuses or whose frames * channels
 * exceed 32 bits, out->lengths given and not all `length` (out->length != length without them), strides too small,
 * n_entries == 0, max_frames + 1 > 4097 (such windows stay with glc_decode_crops_device_compact), an output extent
 * that overlaps the arena or an index array.  n_clips == 0 is GLC_OK. */
int glc_decode_crops_device_store(glc_ctx *ctx,
                                  const void *d_arena, uint64_t arena_bytes,
                                  const glc_store_entry *d_entries, const int64_t *d_lengths, uint64_t n_entries,
                                  uint64_t max_length,
                                  const int64_t *d_clips, const int64_t *d_starts, uint64_t length,
                                  float *d_out, const glc_clip_layout *out);

/* ---- ragged crops from the store: short clips zero-padded on the device --------------------- */

/* Host only: the slots a RAGGED crop of `length` samples per channel needs (below): the descriptors of its valid
 * part - one per hop - plus those of its padding - one per 1024 ch interleaved positions - at their most over every
 * valid length 1 .. length and every start, and the frames, which are glc_store_crop_slots' (a valid part is no longer
 * than the row).  With f(v) = floor((1024 ch - ch + 512 % ch + v ch - 1) / (1024 ch)) + 1 + ceil((length - v) ch /
 * (1024 ch)),  max_descs = max(f(1), f(min(2, length))): the most are needed by a valid part of one sample per
 * channel, or of two, that starts as late in its hop as a start can put it; it is glc_store_crop_slots' max_hops or
 * one more.  GLC_EINVAL: a null pointer, channels == 0, length == 0, a length * channels that wraps. */
int glc_store_ragged_slots(uint64_t length, uint16_t channels, uint64_t *max_descs, uint64_t *max_frames);

/* glc_decode_crops_device_store for a ragged corpus: every crop owns an output row of `length` samples per channel,
 * takes as many of them from its clip as the clip has, and the rest of the row is zeros.  The arguments are that
 * call's, plus d_want (device int64_t[n_clips], 8-byte aligned, or NULL: every crop wants `length`) and d_valid
 * (device int64_t[n_clips], 8-byte aligned, or NULL).  With n = d_lengths[d_clips[i]], s = d_starts[i] and w = d_want ?
 * d_want[i] : length, the selection of crop i is usable when the clip index is inside [0, n_entries), n is a length the
 * encoder accepts and at most max_length, 0 <= s < n and 1 <= w <= length; otherwise its verdict is
 * GLC_COMPACT_BAD_CROP and the entry is not read.  A usable selection whose entry is unusable is GLC_COMPACT_NO_BLOB, by
 * that call's rule.  The valid length of a usable crop is v = min(w, n - s) >= 1:
 *   samples [0, v) per channel of clip i of `out` are bit for bit what glc_decode_crops_device_compact writes for
 *     d_blobs[i] = d_arena + entry.offset, blob_bytes[i] = entry.bytes, n_samples[i] = n * channels, crops[i] = {s, v} -
 *     damaged blobs included - and glc_decode_compact_last_status gives that call's words, one per crop;
 *   samples [v, length) of every channel are +0.0;
 *   d_valid[i] = v.
 * An unusable crop is +0.0 over its length * channels samples, with status flags = its verdict | GLC_COMPACT_BAD_HEADER,
 * n_bad_rows = first_bad_row = 0, and d_valid[i] = 0.  Exactly the length * channels elements of every crop are
 * written and no other element of d_out; out->lengths[i], or out->length, must be `length`.  max_length < length is
 * legal: every clip is then short.  No load leaves the arena, d_entries[0 .. n_entries), d_lengths[0 .. n_entries), the
 * two selection arrays or d_want[0 .. n_clips), whatever they hold; d_valid is only written, by ordinary stores.
 * A crop owns the table rows and block slots of glc_store_crop_slots(length) - its valid part is no longer than that -
 * and glc_store_ragged_slots(length)'s max_descs descriptors; the rounds are floor(4097 / (max_frames + 1)) crops.  The
 * family's rules are glc_decode_crops_device_store's word for word: queued on glc_ctx_stream(ctx), NOT synchronised; no
 * host-to-device copy, no wait for the pinned table image; the number and shape of the launches depend on n_clips,
 * length and channels alone - not on the selection, the wanted lengths or how many clips are short; the call blocks
 * only where a workspace has to grow; afterwards no stream is resident and an open decode session is closed.
 * GLC_EINVAL, before anything is queued: everything glc_decode_crops_device_store refuses except max_length < length
 * (a length * channels that wraps is refused by name), d_want or d_valid not 8-byte aligned, d_want or d_valid
 * overlapping the output extent, d_valid overlapping the arena or an input array.  n_clips == 0 is GLC_OK.
 * The _i16 twin writes 16-bit PCM narrowed as glc_decode_crops_device_store_i16 narrows: padding and unusable crops
 * are 0, the layout counts int16_t elements, everything else is the same. */
int glc_decode_ragged_crops_device_store(glc_ctx *ctx,
                                         const void *d_arena, uint64_t arena_bytes,
                                         const glc_store_entry *d_entries, const int64_t *d_lengths, uint64_t n_entries,
                                         uint64_t max_length,
                                         const int64_t *d_clips, const int64_t *d_starts, const int64_t *d_want,
                                         uint64_t length,
                                         float *d_out, const glc_clip_layout *out, int64_t *d_valid);
int glc_decode_ragged_crops_device_store_i16(glc_ctx *ctx,
                                             const void *d_arena, uint64_t arena_bytes,
                                             const glc_store_entry *d_entries, const int64_t *d_lengths, uint64_t n_entries,
                                             uint64_t max_length,
                                             const int64_t *d_clips, const int64_t *d_starts, const int64_t *d_want,
                                             uint64_t length,
                                             int16_t *d_out, const glc_clip_layout *out, int64_t *d_valid);

/* ---- evicting clips from the store: compact arena and index on the device ------------------- */

/* What d_new_index holds for an entry that was not kept. */
#define GLC_STORE_DROPPED      (-1)  /* keep[i] == 0 */
#define GLC_STORE_UNUSABLE     (-2)  /* stored == 0, offset or bytes not a multiple of 64, bytes == 0,
                                        or [offset, offset + bytes) not inside the source arena */
#define GLC_STORE_OUT_OF_ORDER (-3)  /* begins below the end of an earlier candidate */

/* Drops clips from a store and closes the gaps: the kept blobs move to the front of d_dst in index order, the index
 * is rewritten to match, and *d_cursor is left where the next glc_encode_batch_device_compact appends.  The
 * selection d_keep[n_entries] (non-zero = keep) is device data, and everything is decided on the device.
 * Candidates: entry i is a candidate when keep[i] != 0 and it is usable: stored != 0, offset % 64 == 0,
 *   bytes % 64 == 0, bytes != 0, offset <= arena_bytes and bytes <= arena_bytes - offset.
 * Kept: a candidate is kept when its offset is not below E_i, the maximum of offset + bytes over ALL candidates
 *   j < i (0 when there is none).  Every store the encoder wrote passes (its offsets ascend with i across rounds
 *   and calls), and so does every host-made store laid out in index order.
 * Placement: the kept entries, in index order, are numbered 0 .. n_out - 1; number k goes to the destination offset
 *   that is the sum of `bytes` of the kept entries in front of it, from 0, every one a multiple of 64.
 *   d_entries_out[k] = {new offset, bytes, n_pairs, n_raw_rows, stored}, stored = (new offset <= dst_bytes && bytes <=
 *   dst_bytes - new offset): in place always 1; out of place a blob that does not fit is not written, and the sum
 *   and the cursor count on - the encoder's rule.  d_lengths_out[k] = d_lengths[i].  d_new_index[i] = k, or
 *   GLC_STORE_DROPPED, which wins over GLC_STORE_UNUSABLE, which wins over GLC_STORE_OUT_OF_ORDER.  *d_n_out = n_out.
 *   *d_cursor = the sum over all kept entries: written, never read.  Entries and lengths [n_out, n_entries) of the
 *   output arrays are written as all-zero words: a stale index gives GLC_COMPACT_NO_BLOB or GLC_COMPACT_BAD_CROP in a
 *   draw, it does not read old bytes.
 * Bytes: for every kept, stored entry the `bytes` bytes at its new offset in d_dst are the bytes that were at its old
 *   offset in d_arena, verbatim; the call does not look into a blob (a damaged one stays exactly as damaged).  In
 *   place no byte of the arena at or above *d_cursor is written.  Out of place no byte of d_dst outside the stored
 *   blobs is written and the source arena is not written at all.  No load leaves [d_arena, d_arena + arena_bytes),
 *   d_entries[0 .. n_entries), d_lengths[0 .. n_entries) or d_keep[0 .. n_entries), whatever they hold.
 * Aliasing: d_dst is d_arena with dst_bytes == arena_bytes (in place) or an arena disjoint from it.  d_entries_out may
 *   be d_entries and d_lengths_out may be d_lengths: the results are as if every input had been read before any output
 *   was written.  Any other overlap among the arenas and arrays is GLC_EINVAL.
 * In place the bytes move in rounds through a staging buffer the context owns (64 MiB packed bytes per round, two
 *   buffers); the host does not know the packed total and queues ceil(arena_bytes / round) + 1 launches, of which those
 *   behind the total return at once.  A caller who knows a bound on the bytes in use (a cursor it has read before)
 *   may pass it as arena_bytes and gets fewer launches - entries that reach behind the bound are then UNUSABLE.
 *   Out of place one gather goes straight into d_dst.
 * Family rules: queued on glc_ctx_stream(ctx) and NOT synchronised; no host-to-device or device-to-host copy; the
 *   call blocks only where its workspace (16 bytes per entry, the staging) has to grow; the number and shape of its
 *   launches depend on n_entries, arena_bytes and the round size alone.  It is not a decode and not an encode: the
 *   resident stream, an open decode session, the kept plan and every "last info / last status" record of the context
 *   stay exactly as they were.
 * GLC_EINVAL, checked before anything is queued: a null pointer (d_lengths and d_lengths_out are both NULL or both
 *   given), an arena not 64-byte aligned, an array not 8-byte aligned (d_keep needs no alignment), n_entries == 0,
 *   the overlaps above, in place with dst_bytes != arena_bytes. */
int glc_store_compact_device(glc_ctx *ctx,
                             void *d_arena, uint64_t arena_bytes,
                             const glc_store_entry *d_entries, const int64_t *d_lengths, uint64_t n_entries,
                             const uint8_t *d_keep,
                             void *d_dst, uint64_t dst_bytes,
                             glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                             int64_t *d_new_index,
                             uint64_t *d_n_out, uint64_t *d_cursor);

/* ---- integer PCM on the device batch and store paths: S16 / S32 in, S16 out ------------------ */

/* The integer twins of the five device-resident batch calls.  Each follows its float twin's contract word for word -
 * rounds, launches per round independent of the number of clips, no copy to or from the host, no synchronisation
 * except for workspace growth, the pinned-table rule, what the call leaves on its context - except where stated here.
 *
 * Input side (glc_encode_batch_device_compact_int, glc_roundtrip_batch_device_pcm): `fmt` is GLC_PCM_S16 (int16_t
 * samples of `bits` = 1..16 bits), GLC_PCM_S32 (int32_t, 1..32) or GLC_PCM_F32 (`bits` ignored: the call forwards
 * to its float twin), validated as glc_encode_int validates them.  The strides and lengths of the glc_clip_layout
 * count ELEMENTS of the sample type; d_pcm is aligned to its sample size and to nothing more - odd strides and slices
 * that start on any element are legal.  Every sample is widened in the gather itself by the rule of
 * glc_pcm_widen_device (one device function serves both: `(float)s / 2^(bits-1)`, -2^31 for bits == 32), so the blob
 * of clip i is byte for byte what glc_encode_batch_device_compact stores for the same clip widened by
 * glc_pcm_widen_device; entries, cursor arithmetic and the round-trip output are identical likewise.  Nothing
 * outside the clips' true samples is read.  The zeros behind a clip are +0.0, the reference's padding, not widened
 * integer zeros (no output can tell the two apart).
 *
 * Output side (out_fmt == GLC_PCM_S16 and the three _i16 calls): what the float call writes, narrowed as the
 * reference's 16-bit writers narrow (`(s * 32767.0).clamp(-32768.0, 32767.0) as i16`, NaN -> 0).  The layout counts
 * int16_t elements, d_out is any 2-byte aligned pointer, no element outside the clips or crops is written.  An
 * unusable crop of the store draw is 0 over its samples.  glc_decode_compact_last_status and
 * glc_roundtrip_batch_last_info return exactly the words of the float call.  out_fmt is GLC_PCM_F32 or GLC_PCM_S16;
 * anything else is GLC_EINVAL.
 *
 * Overlap is judged on BYTE extents.  The round trip in place is accepted only when pointer, layout and format are
 * all the same (S16 -> S16 too); every other overlap, an input and an output of different widths on one buffer
 * included, is GLC_EINVAL, as are an extent that overlaps the arena, a blob or an index array where the float
 * twin refuses it. */
int glc_encode_batch_device_compact_int(glc_ctx *ctx, const void *d_pcm, glc_pcm_format fmt, uint32_t bits,
                                        const glc_clip_layout *in, void *d_arena, uint64_t arena_bytes,
                                        uint64_t *d_cursor, glc_store_entry *d_entries);
int glc_roundtrip_batch_device_pcm(glc_ctx *ctx, const void *d_pcm, glc_pcm_format fmt, uint32_t bits,
                                   const glc_clip_layout *in, void *d_out, glc_pcm_format out_fmt,
                                   const glc_clip_layout *out);
int glc_decode_batch_device_compact_i16(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes,
                                        const uint64_t *n_samples, int16_t *d_out, const glc_clip_layout *out);
int glc_decode_crops_device_compact_i16(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes,
                                        const uint64_t *n_samples, const glc_crop *crops, int16_t *d_out,
                                        const glc_clip_layout *out);
int glc_decode_crops_device_store_i16(glc_ctx *ctx,
                                      const void *d_arena, uint64_t arena_bytes,
                                      const glc_store_entry *d_entries, const int64_t *d_lengths, uint64_t n_entries,
                                      uint64_t max_length,
                                      const int64_t *d_clips, const int64_t *d_starts, uint64_t length,
                                      int16_t *d_out, const glc_clip_layout *out);

/* ---- streaming encode: PCM in chunks, many live streams per launch chain ------------------- */

/* Frame f of a stream reads the per-channel samples [1024 f - 512, 1024 f + 1536), so it is final once
 * 1024 f + 1536 samples have arrived, whatever follows; only the last frames depend on the total length.  A stream
 * pushed in ANY chunking serialises to exactly the bytes glc_encode gives for the concatenation.
 *
 * Host only: what a push of n_new samples per channel completes on a lane that has received `received` so far.
 * Without `finish`: the frames done after R samples are max(1, (R + 512) / 1024) - 1; held back afterwards is
 * everything from sample 1024 done - 512 on (everything while done == 0), never more than 2047 samples per channel.
 * With `finish` the total L = received + n_new ends the stream: all remaining frames of the encode plan of L samples
 * of one channel are completed, with the reference's zero padding behind L, and carry is 0.
 * GLC_EINVAL: a null pointer, a sum that wraps, a finish at L <= 512 (the reference panics there). */
typedef struct glc_stream_push_plan {
  uint64_t first_frame;  /* frames completed before this push */
  uint64_t n_frames;     /* frames this push completes */
  uint64_t carry;        /* samples per channel held back afterwards; 0 after a finish */
} glc_stream_push_plan;
int glc_plan_stream_push(uint64_t received, uint64_t n_new, int finish, glc_stream_push_plan *out);

/* A session of n_streams independent lanes of `channels` channels on one context.  The session owns the lanes'
 * held-back samples in device memory of its own (widened floats, two buffers of 2048 * channels per lane); the host
 * keeps the samples received and the frames done per lane.  No workspace of the context holds lane state: any other
 * call on the context may run between two pushes.  Close a session before its context is destroyed.  open, close,
 * reset and the getters leave the context as it was.  A session is not thread-safe, like its context.
 * GLC_EINVAL: a null pointer, channels == 0, n_streams == 0 or so many that the buffers' size wraps. */
typedef struct glc_stream_enc glc_stream_enc;
int glc_stream_enc_open(glc_ctx *ctx, uint16_t channels, uint64_t n_streams, glc_stream_enc **out);
void glc_stream_enc_close(glc_stream_enc *s);
/* Lane `stream` back to "nothing received": what it held back and its host segments are dropped. */
int glc_stream_enc_reset(glc_stream_enc *s, uint64_t stream);
/* Samples per channel one lane may take in one device push: the frames it completes then fit one round. */
uint64_t glc_stream_enc_max_push(uint16_t channels);

/* Device push.  Lane i receives the in->lengths[i] (or in->length) samples per channel of clip i of the layout
 * (in->n_clips == n_streams, in->channels == the session's; a length may be 0); layout, sample types, strides and
 * alignment are those of glc_encode_batch_device_compact_int, and nothing outside those samples is read.  finish[i]
 * != 0 (host array, or NULL for none) ends lane i with this chunk, which may be empty; the lane is fresh afterwards.
 * Every lane that completes at least one frame yields one SEGMENT, in ascending lane order: segs[j] (host, room for
 * n_streams, filled before the call returns, *n_segs of them) names the lane and the frame range, d_entries[j]
 * (device, room for n_streams) is written by the device, and the blob is byte for byte what glc_encode_range_device
 * of those frames of the whole stream followed by glc_compact_device_records gives.  Placement, the 64-byte
 * alignment, the `stored` rule and the cursor that counts on are exactly those of glc_encode_batch_device_compact.
 * A lane that completes nothing writes no entry; only what it holds back changes.
 * Segments are packed into rounds as clips are, each counting its frames + 1 (one more per round in front); per round
 * one stager launch - it replaces the gather: the virtual stream from what was held back and what arrived, and (first
 * round) every lane's new held-back samples -, the transform and quantiser chain and the three pack launches, whatever
 * the number of lanes.  Queued on glc_ctx_stream of the session's context, NOT synchronised; no copy to the host and
 * none from it but the pinned table image; the call blocks only where a workspace has to grow and on the table image
 * of the previous batch call.  Afterwards the context is as glc_encode_batch_device_compact leaves it: no stream
 * resident, an open decode session closed; this holds for every accepted push, whether or not it completes a frame.
 * GLC_EINVAL, before anything is queued and changing nothing: a null or misaligned pointer, a layout that does not
 * match the session or whose strides are too small, a chunk above glc_stream_enc_max_push or a finish that
 * glc_plan_stream_push refuses (the message names the lane), an arena or entries range that overlaps the input,
 * a session that has taken a host push. */
typedef struct glc_stream_seg { uint64_t stream, first_frame, n_frames; } glc_stream_seg;
int glc_stream_enc_push_device(glc_stream_enc *s, const void *d_pcm, glc_pcm_format fmt, uint32_t bits,
                               const glc_clip_layout *in, const uint8_t *finish,
                               void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
                               glc_store_entry *d_entries, glc_stream_seg *segs, uint64_t *n_segs);

/* Host push.  pcm[i]: the n_samples[i] interleaved samples lane i receives (a multiple of channels, may be 0 and
 * pcm[i] then NULL); finish as above.  The chunks are staged in pinned memory and uploaded, the device push runs into
 * an arena the session owns (sized so that every blob fits), and the new blobs come down - which synchronises - and
 * are appended to the lane's list.  A chunk above glc_stream_enc_max_push is split into several pushes, so it may
 * give several segments.  The segments are what a sender ships as they appear; glc_frames_from_compact assembles them.
 * A finished lane refuses further samples (GLC_EINVAL) until glc_stream_enc_frames or glc_stream_enc_reset.
 * A session is used through host pushes or through device pushes, never both: the first push decides.
 * Totals that are no multiple of `channels` stay with glc_encode.  A refused push changes nothing. */
int glc_stream_enc_push(glc_stream_enc *s, const void *const *pcm, glc_pcm_format fmt, uint32_t bits,
                        const uint64_t *n_samples, const uint8_t *finish);
/* The segments lane `stream` has completed through host pushes and not handed over yet. */
int glc_stream_enc_segments(const glc_stream_enc *s, uint64_t stream, uint64_t *n_blobs);
/* Segment k of them: borrowed, valid until the lane is taken, reset or the session closed.  Any output may be NULL. */
int glc_stream_enc_segment(const glc_stream_enc *s, uint64_t stream, uint64_t k, const void **blob, uint64_t *bytes,
                           uint64_t *first_frame, uint64_t *n_frames);
/* After the finish: the lane's stream assembled from its segments (the context's sample rate, L * channels samples),
 * then the lane is cleared.  GLC_EINVAL while the lane is not finished. */
int glc_stream_enc_frames(glc_stream_enc *s, uint64_t stream, glc_frames **out);

/* ---- joining a streamed clip's segments into one store blob ---------------------------------- */

/* A clip that glc_stream_enc_push_device stored in k chunks lies in the arena as k segment blobs; every other consumer
 * of the store (batch decode, windowed decode, the draw, eviction) takes ONE blob per clip.  This call writes, for
 * every clip, the blob of the whole clip into a destination store.  A segment holds byte for byte the rows the
 * whole-stream encode gives for its frames, so the clip's blob is compact_header(ch, F, P, R, bytes) - F, P, R the
 * sums over its segments - followed by the five sections, each the segments' sections concatenated in frame order,
 * all padding zero: nothing is recomputed, nothing is lossy, and the result is byte for byte what
 * glc_encode_batch_device_compact stores for the whole clip.
 * segs[n_segs] (host, as the encoder pushes returned them) ascends by (stream, first_frame).  The segments of one
 *   `stream` value form one clip: they are consecutive, the first has first_frame == 0, each has n_frames > 0 and starts
 *   where the one before ends.  The clips are numbered 0, 1, .. in order of appearance.  d_entries[j] (device, never
 *   read by the host) names segment j's blob in d_arena.  lengths[c] (host, or NULL): samples per channel of clip c;
 *   the clip's frames must then be glc_plan_encode(lengths[c], 1).n_frames.
 * Usable segment (decided on the device; blobs and entries are untrusted): its entry passes the GLC_COMPACT_NO_BLOB
 *   rule of the draw (stored != 0, offset a multiple of 64, [offset, offset + bytes) inside the arena); its header
 *   passes the compact header rule with exactly the segment's n_frames and entry.bytes available; the sum over its cnt
 *   section is n_pairs; channels times the number of non-zero is_raw bytes is n_raw_rows.  d_seg_status[j] = 0 for a
 *   usable segment, else GLC_COMPACT_NO_BLOB | GLC_COMPACT_BAD_HEADER (entry; nothing of the segment is read),
 *   GLC_COMPACT_BAD_HEADER (header; nothing behind it is read), GLC_COMPACT_PAIR_SUM and / or GLC_COMPACT_RAW_SUM.
 *   Lists are not checked for canonical form: the decode does that, as always.
 * A clip is joined only when all its segments are usable.  A refused clip writes nothing to the destination, its
 *   entry is all zero words (a draw sees GLC_COMPACT_NO_BLOB) and it counts 0 bytes in the placement.
 * Placement is the encoder's: *d_cursor is read and rounded up to 64; the clips are placed in clip order at the
 *   exclusive running sum of their sizes; stored = 1 when the clip fits dst_bytes; the cursor counts on for clips that
 *   do not fit; no byte of d_dst outside the stored blobs is written.  d_entries_out[c] = {offset, bytes, P, R, stored};
 *   d_lengths_out[c] = lengths[c], 0 for a refused clip.
 * No load leaves [d_arena, d_arena + arena_bytes) or d_entries[0 .. n_segs), whatever they hold.
 * Family rules: queued on glc_ctx_stream(ctx), NOT synchronised; no copy to the host and none from it but the pinned
 *   table image (the segment and clip tables); the call blocks only where its workspace has to grow and on the table
 *   image of the previous batch call; three launches whose shape depends on n_segs, the clip count and a host bound on
 *   the joined bytes, never on content.  Like eviction it is neither a decode nor an encode: the resident stream, an
 *   open decode session, the kept plan and every "last info / last status" record stay as they were.
 * GLC_EINVAL, before anything is queued and changing nothing: a null pointer (lengths and d_lengths_out both or
 *   neither), channels == 0, an arena not 64-byte aligned, d_entries / d_cursor / d_entries_out / d_lengths_out not
 *   8-byte aligned, d_seg_status not 4-byte aligned, a segment list that breaks the rules above, a clip of more than
 *   2^32 - 1 rows, any overlap among the two arenas, d_entries and the output arrays.  n_segs == 0 is GLC_OK and
 *   leaves the cursor alone. */
int glc_store_join_segments_device(glc_ctx *ctx,
                                   const void *d_arena, uint64_t arena_bytes,
                                   const glc_store_entry *d_entries,
                                   const glc_stream_seg *segs, uint64_t n_segs,
                                   const uint64_t *lengths, uint16_t channels,
                                   void *d_dst, uint64_t dst_bytes, uint64_t *d_cursor,
                                   glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                                   uint32_t *d_seg_status);

/* Host only, the same join over blobs in host memory (what glc_stream_enc_segment hands out, in frame order): the same
 * bytes under the same usability rule, each blob judged against its own header's frame count (not 0, not more than
 * blob_bytes - 64, not more than 2^32 - 1 rows: a count that could make the section sizes wrap is refused before any
 * size is formed) and its blob_bytes.  n_blobs == 0 is GLC_EINVAL: there is no clip without a segment.  info (never NULL) receives the joined counts; GLC_EINVAL with glc_last_error(NULL) naming the
 * segment for an unusable one, and for a cap below info->bytes (info is then filled).  blobs and out 8-byte aligned. */
int glc_compact_join(const void *const *blobs, const uint64_t *blob_bytes, uint32_t n_blobs, uint16_t channels,
                     void *out, uint64_t cap, glc_compact_info *info);

/* ---- cutting stored clips into frame ranges: split, trim, resend ------------------------------ */

/* The inverse of the join: the blob of frames [first_frame, first_frame + n_frames) of a stored clip, as a store entry of
 * its own.  A blob's five sections are indexed by frame, by row or by the rows in front, so the piece is
 * compact_header(ch, nf, P, R, bytes) followed by five contiguous windows of the source's sections, all padding zero:
 * is_raw[f0 .. f0 + nf), the scale and cnt rows [ch f0, ch (f0 + nf)), the P pairs behind the P0 pairs of the rows in
 * front, the R raw planes behind the R0 in front - P the sum of the window's cnt words, R channels times its non-zero
 * is_raw bytes.  Nothing is recomputed and nothing is lossy: the pieces of a partition are byte for byte the segment
 * blobs glc_stream_enc_push_device stores for those frames, they pass the header rule and the join's segment rule, and
 * glc_store_join_segments_device over them gives the source back.  A piece is a clip to every consumer of the store
 * (decode, crops, the draw, eviction) and a segment to glc_stream_dec_push_device.
 * cuts[n_cuts] (host): any order, a clip any number of times, ranges may overlap; n_frames > 0; output i belongs to cut
 *   i.  d_entries[n_entries] (device, never read by the host) is the source store's index.  lengths[i] (host, or NULL):
 *   samples per channel of piece i, which must plan to n_frames frames (glc_plan_encode(lengths[i], 1)); NULL stands
 *   for 1024 * n_frames, which does.  d_lengths_out[i] receives it, 0 for a refused cut.
 * Usable cut (decided on the device; entries and blobs are untrusted), the first rule that fails:
 *   GLC_COMPACT_BAD_CROP: clip >= n_entries (the entry is not read).
 *   GLC_COMPACT_NO_BLOB | GLC_COMPACT_BAD_HEADER: the entry fails the draw's rule (stored != 0, offset a multiple of 64,
 *     [offset, offset + bytes) inside the arena); nothing of the blob is read.
 *   GLC_COMPACT_BAD_HEADER: the header fails the compact header rule with its OWN frame count - not 0, not more than
 *     2^32 - 1 rows, not more than entry.bytes - 64, bounded before any size is formed as glc_compact_join bounds it -
 *     and entry.bytes available; nothing behind the header is read.
 *   GLC_COMPACT_BAD_CROP: first_frame + n_frames beyond the header's n_frames.
 *   GLC_COMPACT_ROW_BOUNDS: a cnt word above 1024 in front of the window or in it, or P0 + P above the header's n_pairs;
 *   GLC_COMPACT_RAW_RANGE: R0 + R above the header's n_raw_rows (the two may be set together).
 *   Nothing behind the window's last row and frame is read, as in the crop calls: GLC_COMPACT_PAIR_SUM and
 *   GLC_COMPACT_RAW_SUM are NEVER set, and damage behind the window does not refuse a cut.  Lists are not checked for
 *   canonical form: the decode does that, as always.  d_cut_status[i] = 0 for a usable cut.
 * A refused cut writes nothing to the destination, its entry is all zero words (a draw sees GLC_COMPACT_NO_BLOB) and it
 *   counts 0 bytes in the placement.
 * Placement is the encoder's, word for word the join's: *d_cursor is read and rounded up to 64; the pieces are placed in
 *   cut order at the exclusive running sum of their sizes; stored = 1 when the piece fits dst_bytes; the cursor counts
 *   on for pieces that do not fit; no byte of d_dst outside the stored blobs is written.  d_entries_out[i] = {offset,
 *   bytes, P, R, stored}.
 * No load leaves d_entries[0 .. n_entries) or [d_arena, d_arena + arena_bytes), whatever they hold, and for a usable
 *   entry none leaves that entry's own [offset, offset + bytes).
 * Family rules: queued on glc_ctx_stream(ctx), NOT synchronised; no copy to the host and none from it but the pinned
 *   table image (the cut table); the call blocks only where its workspace has to grow and on the table image of the
 *   previous batch call; three launches whose shape depends on n_cuts and a host bound on the pieces' bytes (the sum of
 *   the worst-case sizes of n_frames frames, capped by dst_bytes), never on content.  Like the join it is neither a
 *   decode nor an encode: the resident stream, an open decode session, the kept plan and every "last info / last
 *   status" record stay as they were.
 * GLC_EINVAL, before anything is queued and changing nothing: a null pointer (only lengths may be NULL), channels == 0,
 *   an arena not 64-byte aligned, d_entries / d_cursor / d_entries_out / d_lengths_out not 8-byte aligned, d_cut_status
 *   not 4-byte aligned, a cut with n_frames == 0, a piece of more than 2^32 - 1 rows, a lengths[i] that does not plan
 *   to n_frames, any overlap among the two arenas, d_entries and the output arrays.  n_cuts == 0 is GLC_OK and leaves
 *   the cursor alone. */
typedef struct glc_store_cut { uint64_t clip, first_frame, n_frames; } glc_store_cut;
int glc_store_cut_device(glc_ctx *ctx,
                         const void *d_arena, uint64_t arena_bytes,
                         const glc_store_entry *d_entries, uint64_t n_entries,
                         const glc_store_cut *cuts, uint64_t n_cuts,
                         const uint64_t *lengths, uint16_t channels,
                         void *d_dst, uint64_t dst_bytes, uint64_t *d_cursor,
                         glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                         uint32_t *d_cut_status);

/* Host only, the same cut of a blob in host memory: the same bytes under the same rules, blob_bytes in the place of
 * entry.bytes.  info (never NULL) receives the piece's counts; GLC_EINVAL with glc_last_error(NULL) naming what was
 * wrong for an unusable blob or window, for n_frames == 0, and for a cap below info->bytes (info is then filled).
 * blob and out 8-byte aligned. */
int glc_compact_cut(const void *blob, uint64_t blob_bytes, uint16_t channels,
                    uint64_t first_frame, uint64_t n_frames,
                    void *out, uint64_t cap, glc_compact_info *info);

/* ---- streaming decode: segment blobs in, PCM out, many live streams per launch chain ------- */

/* The receiving half of a stream: the segments glc_stream_enc_* emits are decoded as they arrive, and the
 * concatenation of a lane's outputs over ANY chunking is bit for bit glc_decode(glc_frames_from_compact(segments)).
 *
 * Host only: what a push of n_frames frames emits on a lane that has taken frames_done so far.  A stream of L samples
 * per channel has nf = glc_plan_encode(L, 1).n_frames frames, and decoded sample t of channel c lies at the un-trimmed
 * interleaved position 512 + t * channels + c; the receiver learns L only at the finish.  After D frames a lane has
 * emitted emitted(D) = 1024 D - 512 samples per channel (0 at D = 0) - whole hops cannot be emitted: with two or more
 * channels the reference's trim cuts into the last ones.  Without `finish` the push emits [emitted(D), emitted(D + n));
 * with `finish` and the total length total_len = L, which must plan to exactly frames_done + n_frames frames, it
 * emits [emitted(D), L): at most 512 samples and a hop per channel more.  emitted(D) < L for every D <= nf.
 * GLC_EINVAL: a null pointer, a sum that wraps, a finish whose total_len does not plan to frames_done + n_frames. */
typedef struct glc_stream_dec_plan {
  uint64_t first_sample;  /* per channel: samples emitted before this push */
  uint64_t n_samples;     /* per channel: samples this push emits */
} glc_stream_dec_plan;
int glc_plan_stream_dec_push(uint64_t frames_done, uint64_t n_frames, int finish, uint64_t total_len,
                             glc_stream_dec_plan *out);

/* A session of n_streams independent lanes of `channels` channels on one context.  The session owns the lanes' carry
 * in device memory of its own (2 * 1024 * channels floats per lane: the finished, not yet emitted sums of the last
 * hop, and the second half of the last frame's windowed block); the host keeps the frames done per lane.  No workspace
 * of the context holds lane state: any other call on the context may run between two pushes, and several sessions may
 * live on one context.  Close a session before its context is destroyed.  open, close, reset and the getters leave
 * the context as it was.  A session is not thread-safe, like its context.
 * GLC_EINVAL: a null pointer, channels == 0, n_streams == 0 or so many that the buffer's size wraps. */
typedef struct glc_stream_dec glc_stream_dec;
int glc_stream_dec_open(glc_ctx *ctx, uint16_t channels, uint64_t n_streams, glc_stream_dec **out);
void glc_stream_dec_close(glc_stream_dec *s);
/* Lane `stream` back to "no frame taken". */
int glc_stream_dec_reset(glc_stream_dec *s, uint64_t stream);
/* Frames one lane may take in one push (over all its segments of the push). */
uint64_t glc_stream_dec_max_push(uint16_t channels);
int glc_stream_dec_frames_done(const glc_stream_dec *s, uint64_t stream, uint64_t *n);

/* Device push.  segs[n_segs] (host) and d_entries[n_segs] (device, 8-byte aligned, never read by the host) are what
 * glc_stream_enc_push_device returned, possibly concatenated over several encoder pushes: ascending by (stream,
 * first_frame), a lane's segments consecutive and starting at its frames done - so a clip stored as k segments
 * decodes in one call.  d_arena / arena_bytes: the arena the entries point into (64-byte aligned).  finish[i] != 0
 * (host array per lane, or NULL for none) ends lane i with this push at total_len[i] samples per channel (total_len
 * may be NULL when nothing finishes); a finish may bring no frames.  A finished lane is fresh afterwards.
 * `out` describes n_streams clips in d_out (out->n_clips == n_streams, out->channels == the session's): lane i's
 * emitted samples - glc_plan_stream_dec_push of its frames - are clip i, and out->lengths[i] (or out->length) must be
 * exactly that plan's n_samples, 0 included.  out_fmt: GLC_PCM_F32 (d_out holds floats) or GLC_PCM_S16 (int16_t,
 * narrowed in the overlap-add as the _i16 calls narrow); the layout counts elements of that type.  No element of
 * d_out outside the lanes' spans is written.
 * A segment is a whole blob whose header must carry exactly the segment's frame count.  Untrusted: a segment whose
 * entry is unusable (stored == 0, an offset that is no multiple of 64, [offset, offset + bytes) not inside the arena:
 * GLC_COMPACT_NO_BLOB | GLC_COMPACT_BAD_HEADER, nothing of it is read) or whose header fails the check
 * (GLC_COMPACT_BAD_HEADER) contributes +0.0 blocks for all its frames; rows are kept or rejected by the rules of the
 * compact decode family; neighbouring segments and lanes are not affected; no load leaves the arena or
 * d_entries[0 .. n_segs).  glc_decode_compact_last_status afterwards gives one status per SEGMENT.
 * Segments are packed into rounds as the batch decode packs clips; per round one row-table pass, at most two carry
 * launches, one inverse transform and one overlap-add, whatever the number of lanes, behind one planner launch per
 * push.  Queued on glc_ctx_stream of the session's context, NOT synchronised; nothing is copied to the host and
 * nothing from it but the pinned table image; the call blocks only where a workspace has to grow and on the table
 * image of the previous batch call.  Afterwards the context is as the compact decode family leaves it: no stream
 * resident, an open decode session closed, the kept plan dropped.
 * GLC_EINVAL, before anything is queued and changing nothing (the lanes included): a null or misaligned pointer, a
 * segment out of order, not at its lane's frames done or of no frames, a lane above glc_stream_dec_max_push, a finish
 * glc_plan_stream_dec_push refuses, a layout that does not match, an output extent that overlaps the arena or the
 * entries, an out_fmt other than the two, a session that has taken a host push. */
int glc_stream_dec_push_device(glc_stream_dec *s, const void *d_arena, uint64_t arena_bytes,
                               const glc_store_entry *d_entries, const glc_stream_seg *segs, uint64_t n_segs,
                               const uint8_t *finish, const uint64_t *total_len,
                               void *d_out, glc_pcm_format out_fmt, const glc_clip_layout *out);

/* Host push.  blobs[j] / blob_bytes[j]: segment segs[j] in host memory (what glc_stream_enc_segment hands out), in
 * the order above.  The blobs go through pinned staging into an arena the session owns, the entries are made by the
 * host, the device push runs and lane i's samples come down to pcm_out[i] (interleaved, of out_fmt; may be NULL where
 * the lane emits nothing), n_out[i] of them (per lane, all channels counted; the caller sizes pcm_out[i] with
 * glc_plan_stream_dec_push).  Synchronises.  A session is used through host pushes or through device pushes, never
 * both: the first push decides.  A refused push changes nothing. */
int glc_stream_dec_push(glc_stream_dec *s, const void *const *blobs, const uint64_t *blob_bytes,
                        const glc_stream_seg *segs, uint64_t n_segs, const uint8_t *finish, const uint64_t *total_len,
                        void *const *pcm_out, glc_pcm_format out_fmt, uint64_t *n_out);

/* ---- tables (for inspection / parity tests) ---------------------------------------------- */

/* Copies of the host tables of a context: MdctTables.cos_table [1024*2048] (row k), window
 * [2048], norm; PerceptualWeights.weights [1024] and critical_bands (<= 51 edges).
 * Any pointer may be NULL. */
int glc_ctx_tables(const glc_ctx *ctx, float *cos_table, float *window, float *norm,
                   float *weights, uint32_t *band_edges, uint32_t *n_edges);

const char *glc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GLC_H */
