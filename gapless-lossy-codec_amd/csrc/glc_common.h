// glc_common.h — definitions shared by the host sources and, where marked GLC_HD, the device code of the MI355X codec hot path.
// Constants mirror /root/reference/src/codec.rs:15-29.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/glc.h"

// GLC_HD: stated once for the host drivers and the device kernels, which call the same function.
#if defined(__HIP__) || defined(__HIPCC__)
#define GLC_HD __host__ __device__
#else
#define GLC_HD
#endif

namespace glc {

constexpr uint32_t kFrame = GLC_FRAME_SIZE;  // FRAME_SIZE, src/codec.rs:15
constexpr uint32_t kHop = GLC_HOP_SIZE;      // HOP_SIZE,   src/codec.rs:16
constexpr uint32_t kMaxEdges = 51;           // <= 50 band edges + final n, src/codec.rs:154,181
constexpr float kNoiseFloorDb = -48.0f;      // src/codec.rs:22
constexpr float kQuality = 0.7f;             // src/codec.rs:23
constexpr float kCompressionThreshold = 0.85f;  // src/codec.rs:29

// Host tables: MdctTables (src/codec.rs:316-356) + PerceptualWeights (:93-184) + the
// per-bin / per-band constants the device quantiser needs (all derived with the same f32
// expressions the reference evaluates per frame, hoisted because they are frame-invariant).
struct HostTables {
  std::vector<float> cos_table;    // [1024][2048], row k  (reference layout)
  std::vector<float> cos_table_t;  // [2048][1024], row i  (device layout for the forward MDCT)
  std::vector<float> window;       // [2048]
  float norm = 0.f;
  std::vector<float> weights;      // [1024]
  std::vector<uint32_t> edges;     // band edges
  // derived, frame-invariant pieces of compute_masking_thresholds (:218-228):
  std::vector<float> band_pf;      // per band: (1-q).max(.01) and 1/avg_w.max(.1) stay separate
  std::vector<float> band_len;     // (end-start) as f32
  std::vector<float> indiv;        // per bin: 1.0 / weights[i].max(0.1)
  std::vector<uint16_t> band_of;   // per bin: band index
  float cf = 0.f;                  // (1.0 - QUALITY_FACTOR).max(0.01)
  float noise_floor = 0.f;         // 10f32.powf(NOISE_FLOOR_DB / 20.0)
  uint32_t sample_rate = 0;
};

void build_host_tables(uint32_t sample_rate, HostTables &t);
// The table operand of the matrix form of the screened transform (glc_kernels.h MatrixBound): the two bf16 pieces
// t1 = bf16_rn(T), t2 = bf16_rn(T - t1) of T[k][i] for k >= c0 (a multiple of 32), from t.cos_table, in the order
// the instruction's fragments are loaded: [K-block of 16 i][tile of 32 columns][piece][lane 0..63][8 values],
// lane l of a fragment holding column tile * 32 + l % 32 at i = 16 block + 8 (l / 32) .. + 7.
void build_bound_table_image(const HostTables &t, uint32_t c0, std::vector<uint16_t> &out);
uint16_t bf16_round_nearest_even(float x);  // finite x; a value that rounds past the largest bf16 gives infinity

// Padding arithmetic of Encoder::encode, src/codec.rs:433-455.
GLC_HD inline glc_plan plan_encode(uint64_t n_samples, uint16_t channels) {
  glc_plan p{};
  if (channels == 0) return p;  // `i % ch` panics, src/codec.rs:430
  const uint64_t ch = channels;
  auto per_channel = [&](uint64_t c) { return n_samples > c ? (n_samples - c + ch - 1) / ch : 0; };
  auto padded = [](uint64_t len) { return ((kHop / 2 + len + kHop - 1) / kHop) * kHop + kHop / 2; };
  const uint64_t l0 = per_channel(0);
  const uint64_t p0 = padded(l0);
  const uint64_t nf = p0 < kFrame ? 1 : (p0 - kFrame) / kHop + 1;  // :449-455
  const uint64_t last_end = (nf - 1) * kHop + kFrame;              // slice end, :474
  // per_channel(c) descends with c: the last channel is the shortest (a ragged tail leaves it one sample short)
  if (padded(per_channel(ch - 1)) < last_end) return p;  // reference panics: slice out of range
  p.n_frames = nf;
  p.padded_len = p0;
  p.per_channel = l0;
  p.encoder_delay = kHop / 2;                                  // :547
  p.padding = static_cast<uint32_t>(p0 - l0 - kHop / 2);       // :546
  return p;
}

// Per-channel samples [lo, hi) that frames [f0, f1) read (f1 > f0), clipped to a stream of `per_channel`:
// [hop*f0 - hop/2, hop*(f1-1) - hop/2 + frame), src/codec.rs:449-474.
struct SampleWindow {
  uint64_t lo, hi;
};
inline SampleWindow frame_sample_window(uint64_t f0, uint64_t f1, uint64_t per_channel) {
  const uint64_t lo = f0 * kHop > kHop / 2 ? f0 * kHop - kHop / 2 : 0;
  const uint64_t hi = (f1 - 1) * kHop + kFrame - kHop / 2;
  return {lo, hi < per_channel ? hi : per_channel};
}
// The upload mark of a round of frames [f0, f0 + nf): the INTERLEAVED samples of the stream's n_samples that must be on
// the device before its kernels run - everything up to the end of its window, halo included.
inline uint64_t upload_mark(uint64_t f0, uint64_t nf, uint64_t per_channel, uint32_t ch, uint64_t n_samples) {
  const uint64_t hi = frame_sample_window(f0, f0 + nf, per_channel).hi * ch;
  return hi < n_samples ? hi : n_samples;
}

// What a push of n_new samples per channel completes on a lane of a streaming encode that has `received` so far
// (include/glc.h glc_plan_stream_push), the ONE statement of it.  Frame f reads [hop f - hop/2, hop f - hop/2 + frame):
// it is final once hop f + frame - hop/2 samples are there.  false: a wrapping sum, or a finish the encoder refuses.
inline uint64_t stream_frames_done(uint64_t received) {
  const uint64_t a = (received + kHop / 2) / kHop;
  return (a > 1 ? a : 1) - 1;
}
// the lane's first sample that is still held back after `done` frames
inline uint64_t stream_held_from(uint64_t done) { return done ? done * kHop - kHop / 2 : 0; }
inline bool plan_stream_push(uint64_t received, uint64_t n_new, bool finish, glc_stream_push_plan *out) {
  if (n_new > UINT64_MAX - received || received + n_new > UINT64_MAX - 2 * kFrame) return false;
  const uint64_t total = received + n_new, done0 = stream_frames_done(received);
  if (finish) {
    const glc_plan plan = plan_encode(total, 1);
    if (plan.n_frames == 0) return false;
    *out = glc_stream_push_plan{done0, plan.n_frames - done0, 0};
    return true;
  }
  const uint64_t done1 = stream_frames_done(total);
  *out = glc_stream_push_plan{done0, done1 - done0, total - stream_held_from(done1)};
  return true;
}

// What a push of frames [done, done + n) emits on a lane of a streaming decode (include/glc.h
// glc_plan_stream_dec_push), the ONE statement of it.  A stream of L samples per channel has nf = plan_encode(L, 1)
// frames; decoded sample t of channel c lies at the un-trimmed interleaved position 512 + t ch + c (the delay counts
// interleaved samples, Q3), and the receiver learns L only at the finish.  After D frames a lane has emitted
// emitted(D) = 1024 D - 512 samples per channel (0 at D = 0): everything up to there is final whatever follows and
// emitted(D) < L for every D <= nf, so nothing emitted is trimmed later.  A finish with the total L must plan to
// exactly done + n frames and emits [emitted(done), L).  false: a wrapping sum, or such a finish.
inline uint64_t stream_dec_emitted(uint64_t done) { return done ? done * kHop - kHop / 2 : 0; }
inline bool plan_stream_dec_push(uint64_t done, uint64_t n, bool finish, uint64_t total_len, glc_stream_dec_plan *out) {
  if (n > UINT64_MAX - done || done + n > (UINT64_MAX >> 12)) return false;
  const uint64_t first = stream_dec_emitted(done);
  if (finish) {
    if (total_len > (UINT64_MAX >> 12) || plan_encode(total_len, 1).n_frames != done + n || done + n == 0) return false;
    *out = glc_stream_dec_plan{first, total_len - first};
    return true;
  }
  *out = glc_stream_dec_plan{first, stream_dec_emitted(done + n) - first};
  return true;
}

// Gapless trim of a decoded stream, src/codec.rs:756-765: the interleaved samples [start, start + n) of
// the (n_frames + 1) hops.  The delay counts INTERLEAVED samples (quirk Q3).
struct Trim {
  uint64_t start, n;
};
GLC_HD inline Trim gapless_trim(uint64_t n_frames, uint32_t ch, uint64_t encoder_delay, uint64_t original_length) {
  Trim t{0, (n_frames + 1) * static_cast<uint64_t>(kHop) * ch};
  if (t.n > encoder_delay) {
    t.start = encoder_delay;
    t.n -= encoder_delay;
  }
  if (t.n > original_length) t.n = original_length;
  return t;
}
// What a decode round of frames [f0, f0 + nf) contributes to the trimmed output: the un-trimmed interleaved positions
// [lo, hi) of its hops - with the bare tail hop where it is the stream's `last` round, whose nf may be 0 - that the
// trim keeps.  hi >= lo; the spans of a stream's rounds tile [trim.start, trim.start + trim.n).
struct OutSpan {
  uint64_t lo, hi;
};
inline OutSpan decode_round_span(const Trim &trim, uint64_t per_hop, uint64_t f0, uint64_t nf, bool last) {
  const uint64_t c_lo = f0 * per_hop, c_hi = (f0 + nf + (last ? 1 : 0)) * per_hop, end = trim.start + trim.n;
  const uint64_t lo = c_lo > trim.start ? (c_lo < end ? c_lo : end) : trim.start, hi = c_hi < end ? c_hi : end;
  return {lo, hi > lo ? hi : lo};
}

// What a crop of the decoded clip needs of its stream (include/glc.h glc_plan_crop; DESIGN section 3, "a window of a
// compact blob"): the ONE statement of that geometry.  false: what glc_plan_crop refuses.
GLC_HD inline bool plan_crop(uint64_t n_samples, uint16_t channels, const glc_crop &crop, glc_crop_plan *out) {
  const glc_plan plan = plan_encode(n_samples, channels);
  if (plan.n_frames == 0) return false;
  const uint64_t ch = channels, per_hop = static_cast<uint64_t>(kHop) * ch;
  const Trim trim = gapless_trim(plan.n_frames, channels, plan.encoder_delay, n_samples);
  const uint64_t len = trim.n / ch;  // the decoded clip, per channel
  if (crop.length == 0 || crop.length > len || crop.start > len - crop.length) return false;
  // un-trimmed positions [lo, hi): the delay counts INTERLEAVED samples (Q3)
  const uint64_t lo = trim.start + crop.start * ch, hi = lo + crop.length * ch;
  const uint64_t h_lo = lo / per_hop, h_hi = (hi - 1) / per_hop;  // hops of the first and of the last kept sample
  // hop h = second half of frame h - 1 + first half of frame h: the halo frame in front, none for the bare tail hop
  const uint64_t f_lo = (h_lo > 1 ? h_lo : 1) - 1, f_hi = h_hi < plan.n_frames - 1 ? h_hi : plan.n_frames - 1;
  *out = glc_crop_plan{f_lo, f_hi - f_lo + 1, h_lo, h_hi - h_lo + 1};
  return true;
}

// The slots a crop of `length` samples per channel needs wherever it starts (include/glc.h glc_store_crop_slots): it
// lies at the un-trimmed interleaved positions [lo, lo + length * ch), lo = 512 + start * ch, and spans the most
// hops when lo lies as late in its hop as a start can put it - at 1024 ch - ch + 512 % ch, the largest value below
// 1024 ch that is 512 modulo ch.  One frame more than hops: the halo frame.  length >= 1, length * ch must not wrap.
struct CropSlots {
  uint64_t max_hops, max_frames;
};
GLC_HD inline CropSlots store_crop_slots(uint64_t length, uint32_t ch) {
  const uint64_t per_hop = static_cast<uint64_t>(kHop) * ch;
  const uint64_t hops = (per_hop - ch + (kHop / 2) % ch + length * ch - 1) / per_hop + 1;
  return {hops, hops + 1};
}
// The slots of a RAGGED crop (include/glc.h glc_store_ragged_slots): of the `length` samples of its output row the
// first v are the clip's - 1 <= v <= length, v = min(wanted, clip length - start) - and the rest +0.0.  Frames: a
// valid part of v <= length samples needs no more than a crop of `length` does.  Descriptors: one per hop of the
// valid part and one per 1024 ch positions of the padding [v ch, length ch).  With P = 1024 ch, L = length ch,
// x = v ch and the valid part `a` positions into its first hop that is hops(a, x) + pads(x), hops = floor((a + x -
// 1) / P) + 1, pads = ceil((L - x) / P) = floor((L - x + P - 1) / P).  The two numerators add up to S = a + L + P -
// 2 whatever x is, so the sum is floor(S / P) + 1 where the remainders of the two add up to less than P - that is,
// where (a + x - 1) % P <= S % P - and floor(S / P) elsewhere.  It grows with a, so a is the latest place of
// store_crop_slots; there a + x - 1 = P + (512 % ch - 1) + (x - ch), whose remainder is least at x = ch, or, where
// ch divides 512, at x = 2 ch (x = ch then ends exactly on the hop's last position).  If any x reaches the larger
// value, that one does: the most descriptors are those of a valid part of ONE sample per channel, or of two, which
// starts as late in its hop as a start can put it.  x = L is the fixed draw's crop: max_descs >= max_hops, and at
// most one more.  length >= 1, length * ch must not wrap.
struct RaggedSlots {
  uint64_t max_descs, max_frames;
};
GLC_HD inline RaggedSlots store_ragged_slots(uint64_t length, uint32_t ch) {
  const uint64_t per_hop = static_cast<uint64_t>(kHop) * ch, span = length * ch, a = per_hop - ch + (kHop / 2) % ch;
  auto descs = [&](uint64_t x) { return (a + x - 1) / per_hop + 1 + (span - x + per_hop - 1) / per_hop; };
  const uint64_t one = descs(ch), two = descs(length >= 2 ? 2ull * ch : ch);
  return {one > two ? one : two, store_crop_slots(length, ch).max_frames};
}
// Crops of a round of glc_decode_crops_device_store: each counts its slot's frames + 1, as the crops of the pointer
// call count their windows', against the 4096 frames + 1 of a decode round.
constexpr uint64_t kStoreRoundBudget = 4097;

// Fixed-size device record (see include/glc.h glc_record_bytes).
inline uint64_t record_header_bytes(uint32_t ch) { return ((8ull + 8ull * ch) + 15ull) & ~15ull; }
inline uint64_t record_bytes(uint32_t ch) {
  return record_header_bytes(ch) + 2ull * kFrame * ch;
}
// The header's fields: {u32 raw flag, u32 0}, then per channel {f32 scale, u32 nnz}.  `rec` (16-byte aligned bytes) may
// be const or not, and so is the field.
template <typename T, typename B>
GLC_HD inline auto &record_field(B *at) {
  return *reinterpret_cast<typename std::conditional<std::is_const<B>::value, const T, T>::type *>(at);
}
template <typename B>
GLC_HD inline auto &record_raw(B *rec) { return record_field<uint32_t>(rec); }
template <typename B>
GLC_HD inline auto &record_scale(B *rec, uint32_t c) { return record_field<float>(rec + 8 + 8 * c); }
template <typename B>
GLC_HD inline auto &record_nnz(B *rec, uint32_t c) { return record_field<uint32_t>(rec + 8 + 8 * c + 4); }

// Compact ("bitstream payload") form of a contiguous frame range, one self-describing blob:
//   header (64 B) | is_raw u8[n_frames] | scale f32[M] | cnt u32[M] | pairs u32[n_pairs] |
//   raw i16[n_raw_rows][2048]          M = n_frames * channels, every section 64-byte aligned
// cnt[m] is the sparse-list length of row m (0 for the rows of raw frames); pairs are the lists
// back to back in row order, (u16 idx | i16 q << 16) ascending in idx; raw holds the 2048-sample
// planes of the rows of raw frames in row order (channel-planar per frame, quirk Q1).  This is what
// crosses PCIe after an encode and what a multi-GPU job gathers: ~1/8 of the fixed-size records.
constexpr uint32_t kCompactMagic = 0x42434C47u;  // "GLCB"
struct CompactHeader {
  uint32_t magic;
  uint32_t channels;
  uint64_t n_frames;
  uint64_t n_pairs;
  uint64_t n_raw_rows;
  uint64_t bytes;  // whole blob, header included
  uint64_t reserved[3];
};
static_assert(sizeof(CompactHeader) == 64, "compact header is 64 bytes");
GLC_HD inline CompactHeader compact_header(uint32_t ch, uint64_t n_frames, uint64_t n_pairs, uint64_t n_raw_rows, uint64_t bytes) {
  return CompactHeader{kCompactMagic, ch, n_frames, n_pairs, n_raw_rows, bytes, {0, 0, 0}};
}
// The layout and the header rule below are the only statement of either: the host drivers and the device
// kernels (P1-P3 write a blob, R2 reads one) call the same functions.
GLC_HD inline uint64_t align64(uint64_t v) { return (v + 63ull) & ~63ull; }
struct CompactLayout {
  uint64_t o_israw, o_scale, o_cnt, o_pairs;  // byte offsets of the fixed sections
  uint64_t bound;                             // worst-case blob size for this range
};
// The sections of a blob of n_frames frames that are M = n_frames * ch rows.  dir_bytes: a directory between the
// header and the raw flags (the blob of a batch round keeps its clips' there)
GLC_HD inline CompactLayout compact_sections(uint64_t n_frames, uint64_t M, uint64_t dir_bytes = 0) {
  CompactLayout l;
  l.o_israw = sizeof(CompactHeader) + align64(dir_bytes);
  l.o_scale = l.o_israw + align64(n_frames);
  l.o_cnt = l.o_scale + align64(4 * M);
  l.o_pairs = l.o_cnt + align64(4 * M);
  // a row is either compressed (<= 1024 pairs = 4096 B) or raw (2048 i16 = 4096 B)
  l.bound = l.o_pairs + 4096ull * M + 64ull;
  return l;
}
GLC_HD inline CompactLayout compact_layout(uint32_t ch, uint64_t n_frames, uint64_t dir_bytes = 0) {
  return compact_sections(n_frames, n_frames * ch, dir_bytes);
}
GLC_HD inline uint64_t compact_raw_offset(const CompactLayout &l, uint64_t n_pairs) { return align64(l.o_pairs + 4 * n_pairs); }

// A compact header from the device or a caller: magic, channel count, a frame count of at most (or,
// `exact`, exactly) `n_frames`, pair and raw-row counts its rows can hold (a raw frame is raw in every channel),
// and a `bytes` that is exactly its sections and fits the `avail` bytes the blob arrived in.  The first rule
// that fails; the counts are bounded before the sizes are formed from them, so nothing wraps.
enum class HeaderFault { kNone, kIdentity, kCounts, kBytes };
GLC_HD inline HeaderFault compact_header_fault(const CompactHeader &h, uint32_t ch, uint64_t n_frames, uint64_t dir_bytes,
                                               bool exact, uint64_t avail) {
  if (h.magic != kCompactMagic || h.channels != ch || h.n_frames > n_frames || (exact && h.n_frames != n_frames))
    return HeaderFault::kIdentity;
  const uint64_t M = h.n_frames * ch;
  if (h.n_pairs > M * kHop || h.n_raw_rows > M || h.n_raw_rows % ch != 0) return HeaderFault::kCounts;
  const uint64_t need = compact_raw_offset(compact_sections(h.n_frames, M, dir_bytes), h.n_pairs) + h.n_raw_rows * kFrame * 2;
  return h.bytes != need || avail < need ? HeaderFault::kBytes : HeaderFault::kNone;
}
// ... as text: nullptr, or what is wrong
const char *compact_header_error(const CompactHeader &h, uint32_t ch, uint64_t n_frames, bool exact, uint64_t avail);

void set_global_error(const std::string &msg);

// EncodedAudio of a stream planned by plan_encode (src/codec.rs:546-562): the header, zeroed per-frame
// index vectors, list_off = {0} and room for one list and one scale per row.  May throw std::bad_alloc.
void init_frames(glc_frames *F, uint32_t sample_rate, uint64_t n_samples, uint16_t channels, const glc_plan &plan);

// Host assembly of EncodedAudio from compact blobs in frame order (glc_frames_from_compact).
// `trusted`: the blobs were produced by this process's own pack kernels (lists known canonical).
int index_compact_meta(glc_frames *F, uint32_t ch, const CompactHeader &h, const uint8_t *meta, uint64_t f_at,
                       uint64_t p_at, uint64_t r_at, bool trusted, bool *canonical);
int index_compact_rows(glc_frames *F, uint32_t ch, uint64_t n_frames, uint64_t n_pairs, uint64_t n_raw_rows,
                       const uint8_t *israw, const float *scale, const uint32_t *cnt, uint64_t f_at, uint64_t p_at,
                       uint64_t r_at, bool trusted, bool *canonical);
int frames_from_compact(uint32_t sample_rate, uint64_t n_samples, uint16_t channels, const void *const *blobs,
                        const uint64_t *blob_bytes, uint32_t n_blobs, bool trusted, glc_frames **out);

}  // namespace glc

namespace glc {
uint64_t next_frames_uid();  // never 0

// Audio files as the integers they hold (glc_audio_load_pcm): the one parser per format, which the
// float loaders widen.  *samples is malloc'd.  A FLAC stream of at most 16 bits whose decoded values
// leave the 16-bit range (only a malformed one does) keeps them in GLC_PCM_S32.
int wav_load_pcm(const char *path, void **samples, glc_pcm_format *fmt, uint32_t *bits, uint64_t *n_samples,
                 uint32_t *sample_rate, uint16_t *channels);
int flac_decode_pcm(const uint8_t *buf, uint64_t len, void **samples, glc_pcm_format *fmt, uint32_t *bits,
                    uint64_t *n_samples, uint32_t *sample_rate, uint16_t *channels);
int flac_load_pcm(const char *path, void **samples, glc_pcm_format *fmt, uint32_t *bits, uint64_t *n_samples,
                  uint32_t *sample_rate, uint16_t *channels);
// `s as f32 / (1 << (bits - 1)) as f32` over what the calls above return (src/audio.rs:58, :79): takes
// `pcm` over (frees it, or hands a GLC_PCM_F32 buffer through).  nullptr: out of memory.
float *widen_take(void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n);
// convert_f32_to_i16, src/audio.rs:11-16 = src/flac.rs:955-958
inline int16_t narrow_i16(float s) {
  float v = s * 32767.0f;
  if (v != v) return 0;  // NaN passes through clamp and casts to 0
  if (v < -32768.0f) v = -32768.0f;
  if (v > 32767.0f) v = 32767.0f;
  return static_cast<int16_t>(v);
}
}

// EncodedAudio (src/codec.rs:31-69) in a flat, general form: every Vec of the schema keeps its
// own length so that any well-formed bincode stream round-trips byte-for-byte.
struct glc_frames {
  uint32_t sample_rate = 0;
  uint16_t channels = 0;
  uint64_t total_samples = 0;
  uint32_t encoder_delay = 0;
  uint32_t padding = 0;
  uint64_t original_length = 0;
  uint64_t n_frames = 0;
  // per frame
  std::vector<uint64_t> list_begin;   // [n_frames+1] -> index into list_off (sparse lists)
  std::vector<uint64_t> scale_begin;  // [n_frames+1] -> index into scales
  std::vector<uint8_t> raw_tag;       // [n_frames]   Option tag
  std::vector<uint64_t> raw_begin;    // [n_frames+1] -> index into raw
  // pools
  std::vector<uint64_t> list_off;  // [n_lists+1] -> index into pairs
  std::vector<uint32_t> pairs;     // (u16 idx) | (u16 q << 16), stream order
  std::vector<float> scales;
  std::vector<int16_t> raw;
  // true when every sparse list is known to be strictly ascending with idx < 1024 (streams
  // assembled from this library's own records); streams read from bytes are checked at decode
  bool lists_canonical = false;
  // process-unique identity of this (immutable) object: lets a context recognise a stream whose
  // sparse rows it already holds on the device (glc_decode_* called again on the same frames)
  uint64_t uid = glc::next_frames_uid();
};
