// glc.hpp — header-only C++ mirror of the reference's public codec API over the C ABI (glc.h).
//
// Same names, argument meaning and results as the Rust items in src/codec.rs of
// ajcm474/gapless-lossy-codec v0.5.0 (file:line cited per member); `anyhow::Result` becomes an
// exception (glc::Error, carrying the glc_status code).  Inputs the reference panics on throw
// glc::Error(GLC_EINVAL).  All arithmetic happens in libglc_hip.so on a gfx950 device.
#pragma once
#include <cstdint>
#include <exception>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "glc.h"

namespace glc {

constexpr unsigned FRAME_SIZE = GLC_FRAME_SIZE;              // src/codec.rs:15
constexpr unsigned HOP_SIZE = GLC_HOP_SIZE;                  // src/codec.rs:16
constexpr unsigned FRAMES_PER_CHUNK = GLC_FRAMES_PER_CHUNK;  // src/codec.rs:18

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

namespace detail {
inline void check(int rc, const glc_ctx *ctx = nullptr) {
  if (rc != GLC_OK) {
    const char *m = glc_last_error(ctx);
    if (!m || !*m) m = glc_last_error(nullptr);
    throw Error(rc, m ? m : "glc error");
  }
}
}  // namespace detail

struct AudioHeader {  // src/codec.rs:39-45
  uint32_t sample_rate;
  uint16_t channels;
  uint64_t total_samples;
};
struct GaplessInfo {  // src/codec.rs:47-53
  uint32_t encoder_delay, padding;
  uint64_t original_length;
};
struct EncodedFrame {  // src/codec.rs:56-69
  std::vector<std::vector<std::pair<uint16_t, int16_t>>> sparse_coeffs_per_channel;
  std::vector<float> scale_factors;
  bool has_raw_pcm = false;  // Option<Vec<i16>>
  std::vector<int16_t> raw_pcm;
};
struct AudioChunk {  // src/codec.rs:81-85
  std::vector<float> samples;
  bool is_last;
};

// EncodedAudio (src/codec.rs:31-37): owns the library-side object; frames are read on demand.
class EncodedAudio {
 public:
  EncodedAudio() = default;
  explicit EncodedAudio(glc_frames *h) : h_(h) {}
  EncodedAudio(EncodedAudio &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  EncodedAudio &operator=(EncodedAudio &&o) noexcept {
    if (this != &o) {
      glc_frames_free(h_);
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  EncodedAudio(const EncodedAudio &) = delete;
  EncodedAudio &operator=(const EncodedAudio &) = delete;
  ~EncodedAudio() { glc_frames_free(h_); }

  AudioHeader header() const {
    const glc_info i = info();
    return {i.sample_rate, i.channels, i.total_samples};
  }
  GaplessInfo gapless_info() const {
    const glc_info i = info();
    return {i.encoder_delay, i.padding, i.original_length};
  }
  uint64_t n_frames() const { return info().n_frames; }
  EncodedFrame frame(uint64_t f) const {
    EncodedFrame out;
    if (glc_frame_is_raw(h_, f) == 1) {
      uint64_t n = 0;
      detail::check(glc_frame_raw(h_, f, nullptr, 0, &n));
      out.has_raw_pcm = true;
      out.raw_pcm.resize(n);
      detail::check(glc_frame_raw(h_, f, out.raw_pcm.data(), n, &n));
    }
    for (uint32_t c = 0;; ++c) {
      uint32_t n = 0;
      if (glc_frame_sparse(h_, f, c, nullptr, nullptr, 0, &n) != GLC_OK) break;
      std::vector<uint16_t> idx(n);
      std::vector<int16_t> q(n);
      detail::check(glc_frame_sparse(h_, f, c, idx.data(), q.data(), n, &n));
      out.sparse_coeffs_per_channel.emplace_back();
      for (uint32_t j = 0; j < n; ++j) out.sparse_coeffs_per_channel.back().emplace_back(idx[j], q[j]);
    }
    for (uint32_t c = 0;; ++c) {
      float s;
      if (glc_frame_scale(h_, f, c, &s) != GLC_OK) break;
      out.scale_factors.push_back(s);
    }
    return out;
  }
  // bincode::serialize / deserialize of the struct (what save_encoded / load_encoded write)
  std::vector<uint8_t> to_bytes() const {
    std::vector<uint8_t> b(glc_serialized_size(h_));
    uint64_t w = 0;
    detail::check(glc_serialize(h_, b.data(), b.size(), &w));
    return b;
  }
  static EncodedAudio from_bytes(const uint8_t *p, uint64_t n) {
    glc_frames *h = nullptr;
    detail::check(glc_deserialize(p, n, &h));
    return EncodedAudio(h);
  }
  const glc_frames *handle() const { return h_; }

  // ---- the structured bridge (glc.h glc_frames_view / glc_frames_gather): EncodedAudio.frames as nested
  // vectors in one pass over the flat pools, and back by one pointer per vector - no byte stream
  static EncodedFrame frame_from_view(const glc_frames_view &v, uint64_t f) {
    EncodedFrame out;
    const uint64_t l0 = v.list_begin[f], l1 = v.list_begin[f + 1];
    out.sparse_coeffs_per_channel.resize(l1 - l0);
    for (uint64_t l = l0; l < l1; ++l) {
      auto &dst = out.sparse_coeffs_per_channel[l - l0];
      const uint64_t a = v.list_off[l], b = v.list_off[l + 1];
      dst.reserve(b - a);
      for (uint64_t j = a; j < b; ++j) dst.emplace_back(static_cast<uint16_t>(v.pairs[j] & 0xFFFFu), static_cast<int16_t>(v.pairs[j] >> 16));
    }
    if (v.scale_begin[f + 1] > v.scale_begin[f]) out.scale_factors.assign(v.scales + v.scale_begin[f], v.scales + v.scale_begin[f + 1]);
    out.has_raw_pcm = v.raw_tag[f] != 0;
    if (out.has_raw_pcm && v.raw_begin[f + 1] > v.raw_begin[f]) out.raw_pcm.assign(v.raw + v.raw_begin[f], v.raw + v.raw_begin[f + 1]);
    return out;
  }
  std::vector<EncodedFrame> frames() const {  // EncodedAudio.frames, src/codec.rs:35
    glc_frames_view v;
    detail::check(glc_frames_get_view(h_, &v));
    std::vector<EncodedFrame> out;
    out.reserve(v.n_frames);
    for (uint64_t f = 0; f < v.n_frames; ++f) out.push_back(frame_from_view(v, f));
    return out;
  }
  // EncodedAudio { header, frames, gapless_info } from the host's own nested vectors.  `stream_id`: 0, or the
  // caller's identity (< 2^63) of this stream's content - a Decoder that still holds it decodes it again
  // without uploading anything (glc.h glc_frames_from_parts).
  static EncodedAudio from_frames(const AudioHeader &h, const std::vector<EncodedFrame> &frames, const GaplessInfo &g,
                                  uint64_t stream_id = 0) {
    static_assert(sizeof(std::pair<uint16_t, int16_t>) == 4, "(u16, i16) pairs are the library's packed pairs");
    static const int16_t none[1] = {0};
    const size_t nf = frames.size();
    std::vector<uint32_t> lists_per(nf), list_len, scales_per(nf);
    std::vector<const void *> list_ptr;
    std::vector<const float *> scale_ptr(nf);
    std::vector<const int16_t *> raw_ptr(nf);
    std::vector<uint64_t> raw_len(nf);
    for (size_t f = 0; f < nf; ++f) {
      const EncodedFrame &fr = frames[f];
      lists_per[f] = static_cast<uint32_t>(fr.sparse_coeffs_per_channel.size());
      for (const auto &l : fr.sparse_coeffs_per_channel) list_ptr.push_back(l.data()), list_len.push_back(static_cast<uint32_t>(l.size()));
      scales_per[f] = static_cast<uint32_t>(fr.scale_factors.size());
      scale_ptr[f] = fr.scale_factors.data();
      raw_ptr[f] = fr.has_raw_pcm ? (fr.raw_pcm.empty() ? none : fr.raw_pcm.data()) : nullptr;
      raw_len[f] = fr.has_raw_pcm ? fr.raw_pcm.size() : 0;
    }
    glc_frames_gather gg{};
    gg.sample_rate = h.sample_rate, gg.channels = h.channels, gg.total_samples = h.total_samples;
    gg.encoder_delay = g.encoder_delay, gg.padding = g.padding, gg.original_length = g.original_length;
    gg.n_frames = nf;
    gg.lists_per_frame = lists_per.data(), gg.list_ptr = list_ptr.data(), gg.list_len = list_len.data();
    gg.scales_per_frame = scales_per.data(), gg.scale_ptr = scale_ptr.data(), gg.raw_ptr = raw_ptr.data(), gg.raw_len = raw_len.data();
    glc_frames *out = nullptr;
    detail::check(glc_frames_from_gather(&gg, stream_id, &out));
    return EncodedAudio(out);
  }
  uint64_t stream_id() const { return glc_frames_stream_id(h_); }

 private:
  glc_info info() const {
    glc_info i{};
    detail::check(glc_frames_info(h_, &i));
    return i;
  }
  glc_frames *h_ = nullptr;
};

// The frames and hops a crop of a decoded clip needs (glc_plan_crop); throws where it refuses.
inline glc_crop_plan plan_crop(uint64_t n_samples, uint16_t channels, const glc_crop &crop) {
  glc_crop_plan p{};
  detail::check(glc_plan_crop(n_samples, channels, &crop, &p));
  return p;
}

// The hops and frames a crop of `length` samples per channel needs wherever it starts (glc_store_crop_slots).
struct CropSlots {
  uint64_t max_hops, max_frames;
};
inline CropSlots store_crop_slots(uint64_t length, uint16_t channels) {
  CropSlots s{};
  detail::check(glc_store_crop_slots(length, channels, &s.max_hops, &s.max_frames));
  return s;
}

// The descriptors and frames a ragged crop of `length` samples per channel needs (glc_store_ragged_slots).
struct RaggedSlots {
  uint64_t max_descs, max_frames;
};
inline RaggedSlots store_ragged_slots(uint64_t length, uint16_t channels) {
  RaggedSlots s{};
  detail::check(glc_store_ragged_slots(length, channels, &s.max_descs, &s.max_frames));
  return s;
}

// Arena bytes that hold the blobs of every clip of a layout whatever their content (glc_compact_store_bound).
inline uint64_t compact_store_bound(const glc_clip_layout &in) { return glc_compact_store_bound(&in); }

// Evict clips from a store and close the gaps (glc.h glc_store_compact_device), on any context: the kept blobs of
// d_arena go to the front of d_dst (d_arena itself: in place) in index order, the index is rewritten, *d_cursor is where
// the next encode_batch_device_compact appends.  d_keep[n_entries]: device bytes, non-zero = keep.  d_lengths and
// d_lengths_out: both or neither.  Queued on the context's stream, not synchronised; nothing is copied to the host.
// Encoder::compact_store_device and Decoder::compact_store_device forward here.
inline void compact_store_device(glc_ctx *ctx, void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                 const int64_t *d_lengths, uint64_t n_entries, const uint8_t *d_keep, void *d_dst, uint64_t dst_bytes,
                                 glc_store_entry *d_entries_out, int64_t *d_lengths_out, int64_t *d_new_index, uint64_t *d_n_out,
                                 uint64_t *d_cursor) {
  detail::check(glc_store_compact_device(ctx, d_arena, arena_bytes, d_entries, d_lengths, n_entries, d_keep, d_dst, dst_bytes,
                                         d_entries_out, d_lengths_out, d_new_index, d_n_out, d_cursor), ctx);
}

// Join the segments a StreamEncoder's device pushes stored into one blob per clip (glc.h glc_store_join_segments_device),
// on any context: segs (host) ascending by (stream, first_frame), d_entries (device) in the same order; the clips' blobs
// are appended to the store d_dst at *d_cursor by the encoder's placement rule.  lengths (host) and d_lengths_out: both
// or neither.  Queued on the context's stream, not synchronised; nothing is copied to the host.
// StreamEncoder::join_segments_device forwards here.
inline void join_segments_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                 const std::vector<glc_stream_seg> &segs, const uint64_t *lengths, uint16_t channels, void *d_dst,
                                 uint64_t dst_bytes, uint64_t *d_cursor, glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                                 uint32_t *d_seg_status) {
  detail::check(glc_store_join_segments_device(ctx, d_arena, arena_bytes, d_entries, segs.data(), segs.size(), lengths, channels, d_dst,
                                               dst_bytes, d_cursor, d_entries_out, d_lengths_out, d_seg_status), ctx);
}

// The blob of a whole clip from its segment blobs in frame order, on the host (glc_compact_join): the same bytes.
// An empty list is refused, as an unusable segment is.
inline std::vector<uint8_t> compact_join(const std::vector<const void *> &blobs, const std::vector<uint64_t> &blob_bytes, uint16_t channels) {
  if (blobs.size() != blob_bytes.size()) throw Error(GLC_EINVAL, "compact_join: one size per blob");
  glc_compact_info info{};
  const uint32_t n = static_cast<uint32_t>(blobs.size());
  const int rc = glc_compact_join(blobs.data(), blob_bytes.data(), n, channels, nullptr, 0, &info);  // sizes the blob, or says why there is none
  if (rc != GLC_EINVAL || info.bytes == 0) detail::check(rc);
  std::vector<uint64_t> words(info.bytes / 8 + 1);  // 8-byte aligned
  detail::check(glc_compact_join(blobs.data(), blob_bytes.data(), n, channels, words.data(), info.bytes, &info));
  const uint8_t *p = reinterpret_cast<const uint8_t *>(words.data());
  return std::vector<uint8_t>(p, p + info.bytes);
}

// Cut stored clips into frame ranges (glc.h glc_store_cut_device), on any context: the inverse of join_segments_device.
// cuts (host): any order, a clip any number of times, ranges may overlap; piece i is appended to the store d_dst at
// *d_cursor by the encoder's placement rule.  lengths (host, or null for 1024 * n_frames): one per cut.  Queued on the
// context's stream, not synchronised; nothing is copied to the host.  Encoder::cut_clips_device,
// Decoder::cut_clips_device and StreamEncoder::cut_clips_device forward here.
inline void cut_clips_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, uint64_t n_entries,
                             const std::vector<glc_store_cut> &cuts, const uint64_t *lengths, uint16_t channels, void *d_dst,
                             uint64_t dst_bytes, uint64_t *d_cursor, glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                             uint32_t *d_cut_status) {
  detail::check(glc_store_cut_device(ctx, d_arena, arena_bytes, d_entries, n_entries, cuts.data(), cuts.size(), lengths, channels, d_dst,
                                     dst_bytes, d_cursor, d_entries_out, d_lengths_out, d_cut_status), ctx);
}

// The blob of frames [first_frame, first_frame + n_frames) of a clip's blob, on the host (glc_compact_cut): the same bytes.
inline std::vector<uint8_t> compact_cut(const void *blob, uint64_t blob_bytes, uint16_t channels, uint64_t first_frame, uint64_t n_frames) {
  glc_compact_info info{};
  const int rc = glc_compact_cut(blob, blob_bytes, channels, first_frame, n_frames, nullptr, 0, &info);  // sizes the piece, or says why there is none
  if (rc != GLC_EINVAL || info.bytes == 0) detail::check(rc);
  std::vector<uint64_t> words(info.bytes / 8 + 1);  // 8-byte aligned
  detail::check(glc_compact_cut(blob, blob_bytes, channels, first_frame, n_frames, words.data(), info.bytes, &info));
  const uint8_t *p = reinterpret_cast<const uint8_t *>(words.data());
  return std::vector<uint8_t>(p, p + info.bytes);
}

class Encoder {
 public:
  // Encoder::new(sample_rate: u32) — src/codec.rs:406
  explicit Encoder(uint32_t sample_rate, int device = 0) { detail::check(glc_ctx_create(device, sample_rate, &ctx_)); }
  ~Encoder() { glc_ctx_destroy(ctx_); }
  Encoder(const Encoder &) = delete;
  Encoder &operator=(const Encoder &) = delete;
  // encode(&mut self, samples: &[f32], channels: u16) -> Result<EncodedAudio> — src/codec.rs:421
  EncodedAudio encode(const float *samples, uint64_t n_samples, uint16_t channels) {
    glc_frames *h = nullptr;
    detail::check(glc_encode(ctx_, samples, n_samples, channels, &h), ctx_);
    return EncodedAudio(h);
  }
  // glc_encode_batch: every clip an independent stream of `channels` channels, one call for all of them
  std::vector<EncodedAudio> encode_batch(const std::vector<std::vector<float>> &clips, uint16_t channels) {
    std::vector<const float *> pcm(clips.size());
    std::vector<uint64_t> n(clips.size());
    for (size_t i = 0; i < clips.size(); ++i) pcm[i] = clips[i].data(), n[i] = clips[i].size();
    std::vector<glc_frames *> h(clips.size(), nullptr);
    detail::check(glc_encode_batch(ctx_, pcm.data(), n.data(), clips.size(), channels, h.data()), ctx_);
    std::vector<EncodedAudio> out;
    out.reserve(h.size());
    for (glc_frames *f : h) out.emplace_back(f);
    return out;
  }
  EncodedAudio encode(const std::vector<float> &samples, uint16_t channels) {
    return encode(samples.data(), samples.size(), channels);
  }
  // glc_encode_batch_int: clips of 16-bit / of `bits`-bit samples in 32-bit containers, one width for the call
  // (argument order as in the integer `encode` overloads below)
  std::vector<EncodedAudio> encode_batch(const std::vector<std::vector<int16_t>> &clips, uint16_t channels, uint32_t bits = 16) {
    return encode_batch_int(clips, GLC_PCM_S16, bits, channels);
  }
  std::vector<EncodedAudio> encode_batch(const std::vector<std::vector<int32_t>> &clips, uint32_t bits, uint16_t channels) {
    return encode_batch_int(clips, GLC_PCM_S32, bits, channels);
  }
  // encode of what load_wav / load_flac make of integer samples, s / 2^(bits-1) (src/audio.rs:58, :79),
  // without the float copy: the integers go up and are widened on the device (glc_encode_int)
  EncodedAudio encode(const int16_t *samples, uint64_t n_samples, uint16_t channels, uint32_t bits = 16) {
    glc_frames *h = nullptr;
    detail::check(glc_encode_int(ctx_, samples, GLC_PCM_S16, bits, n_samples, channels, &h), ctx_);
    return EncodedAudio(h);
  }
  EncodedAudio encode(const int32_t *samples, uint32_t bits, uint64_t n_samples, uint16_t channels) {
    glc_frames *h = nullptr;
    detail::check(glc_encode_int(ctx_, samples, GLC_PCM_S32, bits, n_samples, channels, &h), ctx_);
    return EncodedAudio(h);
  }
  EncodedAudio encode(const std::vector<int16_t> &samples, uint16_t channels, uint32_t bits = 16) {
    return encode(samples.data(), samples.size(), channels, bits);
  }
  EncodedAudio encode(const std::vector<int32_t> &samples, uint32_t bits, uint16_t channels) {
    return encode(samples.data(), bits, samples.size(), channels);
  }
  // The same call handing the frames out as they arrive on the host, while the device still works on later
  // ones (glc_encode_hooked): `on_frames(first_frame, frames)` is called on this thread with ascending,
  // contiguous ranges - where an application fills its own Vec<EncodedFrame> under the encode instead of after it.
  EncodedAudio encode(const float *samples, uint64_t n_samples, uint16_t channels,
                      const std::function<void(uint64_t, std::vector<EncodedFrame> &&)> &on_frames) {
    struct Ctx {
      const std::function<void(uint64_t, std::vector<EncodedFrame> &&)> *fn;
      std::exception_ptr error;
    } c{&on_frames, nullptr};
    auto tramp = [](void *user, const glc_frames_view *v, uint64_t f0, uint64_t f1) -> int {
      Ctx &cx = *static_cast<Ctx *>(user);
      try {  // no exception may cross the C frames of the library
        std::vector<EncodedFrame> part;
        part.reserve(f1 - f0);
        for (uint64_t f = f0; f < f1; ++f) part.push_back(EncodedAudio::frame_from_view(*v, f));
        (*cx.fn)(f0, std::move(part));
        return 0;
      } catch (...) {
        cx.error = std::current_exception();
        return 1;
      }
    };
    glc_frames *h = nullptr;
    const int rc = glc_encode_hooked(ctx_, samples, n_samples, channels, tramp, &c, &h);
    if (c.error) std::rethrow_exception(c.error);
    detail::check(rc, ctx_);
    return EncodedAudio(h);
  }
  // One shard of an encode on device-resident PCM (multi-GPU hosts): frames [frame_begin, frame_end)
  // from the PCM slice [t0, t0 + t_count) per channel, fixed-size records to d_records
  // (glc_record_bytes(channels) each).  Queued on the context's stream; see glc_encode_range_device.
  void encode_range_device(const float *d_pcm, uint64_t t0, uint64_t t_count, uint64_t n_samples, uint16_t channels,
                           uint64_t frame_begin, uint64_t frame_end, void *d_records) {
    detail::check(glc_encode_range_device(ctx_, d_pcm, t0, t_count, n_samples, channels, frame_begin, frame_end,
                                          d_records, nullptr), ctx_);
  }
  // Assemble EncodedAudio from the records of all shards, gathered in frame order on this device.
  EncodedAudio frames_from_device_records(const void *d_records, uint64_t n_frames, uint64_t n_samples, uint16_t channels) {
    glc_frames *h = nullptr;
    detail::check(glc_frames_from_device_records(ctx_, d_records, n_frames, n_samples, channels, &h), ctx_);
    return EncodedAudio(h);
  }
  // glc_encode_batch_device_compact: every clip of a device-resident batch into its own compact blob, placed back to
  // back in d_arena from *d_cursor by the device; d_entries[i] says where clip i went.  Queued, not synchronised.
  void encode_batch_device_compact(const float *d_pcm, const glc_clip_layout &in, void *d_arena, uint64_t arena_bytes,
                                   uint64_t *d_cursor, glc_store_entry *d_entries) {
    detail::check(glc_encode_batch_device_compact(ctx_, d_pcm, &in, d_arena, arena_bytes, d_cursor, d_entries), ctx_);
  }
  // ... from int16_t / int32_t clips holding `bits`-bit PCM (glc_encode_batch_device_compact_int): widened in the
  // gather, the blobs those of the widened clips byte for byte; the layout counts elements of the sample type
  void encode_batch_device_compact(const int16_t *d_pcm, uint32_t bits, const glc_clip_layout &in, void *d_arena, uint64_t arena_bytes,
                                   uint64_t *d_cursor, glc_store_entry *d_entries) {
    detail::check(glc_encode_batch_device_compact_int(ctx_, d_pcm, GLC_PCM_S16, bits, &in, d_arena, arena_bytes, d_cursor, d_entries), ctx_);
  }
  void encode_batch_device_compact(const int32_t *d_pcm, uint32_t bits, const glc_clip_layout &in, void *d_arena, uint64_t arena_bytes,
                                   uint64_t *d_cursor, glc_store_entry *d_entries) {
    detail::check(glc_encode_batch_device_compact_int(ctx_, d_pcm, GLC_PCM_S32, bits, &in, d_arena, arena_bytes, d_cursor, d_entries), ctx_);
  }
  // glc::compact_store_device on this context
  void compact_store_device(void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const int64_t *d_lengths,
                            uint64_t n_entries, const uint8_t *d_keep, void *d_dst, uint64_t dst_bytes, glc_store_entry *d_entries_out,
                            int64_t *d_lengths_out, int64_t *d_new_index, uint64_t *d_n_out, uint64_t *d_cursor) {
    glc::compact_store_device(ctx_, d_arena, arena_bytes, d_entries, d_lengths, n_entries, d_keep, d_dst, dst_bytes, d_entries_out,
                              d_lengths_out, d_new_index, d_n_out, d_cursor);
  }
  // glc::cut_clips_device on this context
  void cut_clips_device(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, uint64_t n_entries,
                        const std::vector<glc_store_cut> &cuts, const uint64_t *lengths, uint16_t channels, void *d_dst, uint64_t dst_bytes,
                        uint64_t *d_cursor, glc_store_entry *d_entries_out, int64_t *d_lengths_out, uint32_t *d_cut_status) {
    glc::cut_clips_device(ctx_, d_arena, arena_bytes, d_entries, n_entries, cuts, lengths, channels, d_dst, dst_bytes, d_cursor, d_entries_out,
                          d_lengths_out, d_cut_status);
  }
  void synchronize() { detail::check(glc_ctx_synchronize(ctx_), ctx_); }
  glc_ctx *ctx() { return ctx_; }

 private:
  template <typename S>
  std::vector<EncodedAudio> encode_batch_int(const std::vector<std::vector<S>> &clips, glc_pcm_format fmt, uint32_t bits,
                                             uint16_t channels) {
    std::vector<const void *> pcm(clips.size());
    std::vector<uint64_t> n(clips.size());
    for (size_t i = 0; i < clips.size(); ++i) pcm[i] = clips[i].data(), n[i] = clips[i].size();
    std::vector<glc_frames *> h(clips.size(), nullptr);
    detail::check(glc_encode_batch_int(ctx_, pcm.data(), fmt, bits, n.data(), clips.size(), channels, h.data()), ctx_);
    std::vector<EncodedAudio> out;
    out.reserve(h.size());
    for (glc_frames *f : h) out.emplace_back(f);
    return out;
  }
  glc_ctx *ctx_ = nullptr;
};

class Decoder {
 public:
  // Decoder::new(channels: usize, sample_rate: u32) — src/codec.rs:581; `channels` is accepted and
  // ignored like the reference (the stream's header decides)
  Decoder(size_t /*channels*/, uint32_t sample_rate, int device = 0) {
    detail::check(glc_ctx_create(device, sample_rate, &ctx_));
  }
  ~Decoder() { glc_ctx_destroy(ctx_); }
  Decoder(const Decoder &) = delete;
  Decoder &operator=(const Decoder &) = delete;
  // decode(&mut self, &EncodedAudio, _) -> Result<Vec<f32>> — src/codec.rs:744
  // glc_decode_batch: stream i's samples are packed[offsets[i] .. offsets[i + 1])
  std::vector<float> decode_batch(const std::vector<const EncodedAudio *> &encoded, std::vector<uint64_t> &offsets) {
    std::vector<const glc_frames *> h(encoded.size());
    uint64_t total = 0;
    for (size_t i = 0; i < encoded.size(); ++i) h[i] = encoded[i]->handle(), total += glc_decoded_len(h[i]);
    offsets.assign(encoded.size() + 1, 0);
    std::vector<float> packed(total);
    detail::check(glc_decode_batch(ctx_, h.data(), h.size(), packed.data(), packed.size(), offsets.data()), ctx_);
    return packed;
  }
  std::vector<float> decode(const EncodedAudio &encoded) {
    std::vector<float> out(glc_decoded_len(encoded.handle()));
    uint64_t n = 0;
    detail::check(glc_decode(ctx_, encoded.handle(), out.data(), out.size(), &n), ctx_);
    out.resize(n);
    return out;
  }
  // convert_f32_to_i16(decode(..)) (src/audio.rs:11-16), narrowed on the device: what the 16-bit writers take
  std::vector<int16_t> decode_i16(const EncodedAudio &encoded) {
    std::vector<int16_t> out(glc_decoded_len(encoded.handle()));
    uint64_t n = 0;
    detail::check(glc_decode_i16(ctx_, encoded.handle(), out.data(), out.size(), &n), ctx_);
    out.resize(n);
    return out;
  }
  // glc_decode_batch_i16: decode_batch with the narrowing of decode_i16, offsets in samples
  std::vector<int16_t> decode_batch_i16(const std::vector<const EncodedAudio *> &encoded, std::vector<uint64_t> &offsets) {
    std::vector<const glc_frames *> h(encoded.size());
    uint64_t total = 0;
    for (size_t i = 0; i < encoded.size(); ++i) h[i] = encoded[i]->handle(), total += glc_decoded_len(h[i]);
    offsets.assign(encoded.size() + 1, 0);
    std::vector<int16_t> packed(total);
    detail::check(glc_decode_batch_i16(ctx_, h.data(), h.size(), packed.data(), packed.size(), offsets.data()), ctx_);
    return packed;
  }
  // The stream whose sparse rows this Decoder still holds on the device (0: none), and its decode without
  // an EncodedAudio (glc.h glc_decode_resident): for callers that recognise a stream by the id they gave it
  uint64_t resident_stream() const { return glc_ctx_resident_stream(ctx_); }
  std::vector<float> decode_resident(uint64_t stream_id, uint64_t decoded_len) {
    std::vector<float> out(decoded_len);
    uint64_t n = 0;
    detail::check(glc_decode_resident(ctx_, stream_id, out.data(), out.size(), &n), ctx_);
    out.resize(n);
    return out;
  }
  // One shard of a decode into device memory: hops [hop_begin, hop_end) of the un-trimmed stream
  // (n_frames + 1 hops of 1024 * channels samples); see glc_decode_range_device.
  void decode_range_device(const EncodedAudio &encoded, uint64_t hop_begin, uint64_t hop_end, float *d_out, uint64_t cap) {
    detail::check(glc_decode_range_device(ctx_, encoded.handle(), hop_begin, hop_end, d_out, cap), ctx_);
  }
  void synchronize() { detail::check(glc_ctx_synchronize(ctx_), ctx_); }
  // decode_streaming(&mut self, Arc<EncodedAudio>, _) -> Receiver<AudioChunk> — src/codec.rs:595:
  // the receiver becomes a callback invoked once per chunk, in order, the last one with is_last
  void decode_streaming(const EncodedAudio &encoded, const std::function<void(AudioChunk &&)> &on_chunk) {
    detail::check(glc_decode_stream_begin(ctx_, encoded.handle()), ctx_);
    const uint64_t cap = static_cast<uint64_t>(FRAMES_PER_CHUNK) * HOP_SIZE * encoded.header().channels;
    for (;;) {
      AudioChunk c{std::vector<float>(cap), false};
      uint64_t n = 0;
      int last = 0;
      detail::check(glc_decode_stream_next(ctx_, c.samples.data(), cap, &n, &last), ctx_);
      c.samples.resize(n);
      c.is_last = last != 0;
      on_chunk(std::move(c));
      if (last) return;
    }
  }
  // decode_streaming with every chunk narrowed to 16 bits on the device: on_chunk(samples, is_last)
  void decode_streaming_i16(const EncodedAudio &encoded, const std::function<void(std::vector<int16_t> &&, bool)> &on_chunk) {
    detail::check(glc_decode_stream_begin(ctx_, encoded.handle()), ctx_);
    const uint64_t cap = static_cast<uint64_t>(FRAMES_PER_CHUNK) * HOP_SIZE * encoded.header().channels;
    for (;;) {
      std::vector<int16_t> c(cap);
      uint64_t n = 0;
      int last = 0;
      detail::check(glc_decode_stream_next_i16(ctx_, c.data(), cap, &n, &last), ctx_);
      c.resize(n);
      on_chunk(std::move(c), last != 0);
      if (last) return;
    }
  }

  // Compact blobs decoded where they lie in device memory (glc.h glc_decode_device_compact): raw device pointers,
  // queued on the context's stream, nothing copied to the host.  Returns the number of samples written to d_out.
  uint64_t decode_device_compact(const void *d_blob, uint64_t blob_bytes, uint64_t n_samples, uint16_t channels, float *d_out,
                                 uint64_t cap) {
    uint64_t n = 0;
    detail::check(glc_decode_device_compact(ctx_, d_blob, blob_bytes, n_samples, channels, d_out, cap, &n), ctx_);
    return n;
  }
  // ... one blob per clip into a strided (interleaved or planar) device batch, one launch chain per round
  void decode_batch_device_compact(const std::vector<const void *> &d_blobs, const std::vector<uint64_t> &blob_bytes,
                                   const std::vector<uint64_t> &n_samples, float *d_out, const glc_clip_layout &out) {
    if (d_blobs.size() != out.n_clips || blob_bytes.size() != out.n_clips || n_samples.size() != out.n_clips)
      throw Error(GLC_EINVAL, "decode_batch_device_compact: one blob, size and length per clip of the layout");
    detail::check(glc_decode_batch_device_compact(ctx_, d_blobs.data(), blob_bytes.data(), n_samples.data(), d_out, &out), ctx_);
  }
  // ... windows of stored clips: crop i of blob i as clip i of the batch, only the windows' frames decoded
  void decode_crops_device_compact(const std::vector<const void *> &d_blobs, const std::vector<uint64_t> &blob_bytes,
                                   const std::vector<uint64_t> &n_samples, const std::vector<glc_crop> &crops, float *d_out,
                                   const glc_clip_layout &out) {
    if (d_blobs.size() != out.n_clips || blob_bytes.size() != out.n_clips || n_samples.size() != out.n_clips || crops.size() != out.n_clips)
      throw Error(GLC_EINVAL, "decode_crops_device_compact: one blob, size, length and crop per clip of the layout");
    detail::check(glc_decode_crops_device_compact(ctx_, d_blobs.data(), blob_bytes.data(), n_samples.data(), crops.data(), d_out, &out), ctx_);
  }
  // ... crops of one length drawn from the store as its write side left it, selected by device arrays: crop i is
  // samples [d_starts[i], d_starts[i] + length) of stored clip d_clips[i]; nothing is uploaded (glc.h
  // glc_decode_crops_device_store)
  void decode_crops_device_store(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const int64_t *d_lengths,
                                 uint64_t n_entries, uint64_t max_length, const int64_t *d_clips, const int64_t *d_starts,
                                 uint64_t length, float *d_out, const glc_clip_layout &out) {
    detail::check(glc_decode_crops_device_store(ctx_, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                                                d_starts, length, d_out, &out), ctx_);
  }
  // ... the three calls above as 16-bit PCM, narrowed on the device as decode_i16 narrows (the layout counts int16_t
  // elements, d_out is any 2-byte aligned pointer; an unusable crop of the store draw is 0)
  void decode_batch_device_compact_i16(const std::vector<const void *> &d_blobs, const std::vector<uint64_t> &blob_bytes,
                                       const std::vector<uint64_t> &n_samples, int16_t *d_out, const glc_clip_layout &out) {
    if (d_blobs.size() != out.n_clips || blob_bytes.size() != out.n_clips || n_samples.size() != out.n_clips)
      throw Error(GLC_EINVAL, "decode_batch_device_compact_i16: one blob, size and length per clip of the layout");
    detail::check(glc_decode_batch_device_compact_i16(ctx_, d_blobs.data(), blob_bytes.data(), n_samples.data(), d_out, &out), ctx_);
  }
  void decode_crops_device_compact_i16(const std::vector<const void *> &d_blobs, const std::vector<uint64_t> &blob_bytes,
                                       const std::vector<uint64_t> &n_samples, const std::vector<glc_crop> &crops, int16_t *d_out,
                                       const glc_clip_layout &out) {
    if (d_blobs.size() != out.n_clips || blob_bytes.size() != out.n_clips || n_samples.size() != out.n_clips || crops.size() != out.n_clips)
      throw Error(GLC_EINVAL, "decode_crops_device_compact_i16: one blob, size, length and crop per clip of the layout");
    detail::check(glc_decode_crops_device_compact_i16(ctx_, d_blobs.data(), blob_bytes.data(), n_samples.data(), crops.data(), d_out, &out),
                  ctx_);
  }
  void decode_crops_device_store_i16(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const int64_t *d_lengths,
                                     uint64_t n_entries, uint64_t max_length, const int64_t *d_clips, const int64_t *d_starts,
                                     uint64_t length, int16_t *d_out, const glc_clip_layout &out) {
    detail::check(glc_decode_crops_device_store_i16(ctx_, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                                                    d_starts, length, d_out, &out), ctx_);
  }
  // ... ragged crops from the store: crop i takes min(d_want[i] or length, what its clip has from d_starts[i] on)
  // samples, the rest of its `length` is zeros and d_valid[i] the count; d_want and d_valid may be null (glc.h
  // glc_decode_ragged_crops_device_store)
  void decode_ragged_crops_device_store(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                        const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                        const int64_t *d_starts, const int64_t *d_want, uint64_t length, float *d_out,
                                        const glc_clip_layout &out, int64_t *d_valid) {
    detail::check(glc_decode_ragged_crops_device_store(ctx_, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                                                       d_starts, d_want, length, d_out, &out, d_valid), ctx_);
  }
  void decode_ragged_crops_device_store_i16(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                            const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                            const int64_t *d_starts, const int64_t *d_want, uint64_t length, int16_t *d_out,
                                            const glc_clip_layout &out, int64_t *d_valid) {
    detail::check(glc_decode_ragged_crops_device_store_i16(ctx_, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length,
                                                           d_clips, d_starts, d_want, length, d_out, &out, d_valid), ctx_);
  }
  // glc::compact_store_device on this context
  void compact_store_device(void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const int64_t *d_lengths,
                            uint64_t n_entries, const uint8_t *d_keep, void *d_dst, uint64_t dst_bytes, glc_store_entry *d_entries_out,
                            int64_t *d_lengths_out, int64_t *d_new_index, uint64_t *d_n_out, uint64_t *d_cursor) {
    glc::compact_store_device(ctx_, d_arena, arena_bytes, d_entries, d_lengths, n_entries, d_keep, d_dst, dst_bytes, d_entries_out,
                              d_lengths_out, d_new_index, d_n_out, d_cursor);
  }
  // glc::cut_clips_device on this context
  void cut_clips_device(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, uint64_t n_entries,
                        const std::vector<glc_store_cut> &cuts, const uint64_t *lengths, uint16_t channels, void *d_dst, uint64_t dst_bytes,
                        uint64_t *d_cursor, glc_store_entry *d_entries_out, int64_t *d_lengths_out, uint32_t *d_cut_status) {
    glc::cut_clips_device(ctx_, d_arena, arena_bytes, d_entries, n_entries, cuts, lengths, channels, d_dst, dst_bytes, d_cursor, d_entries_out,
                          d_lengths_out, d_cut_status);
  }
  // what the device check found in the blobs (or windows) of the last of these calls (synchronises)
  std::vector<glc_compact_status> last_compact_status(uint64_t n_clips = 1) {
    std::vector<glc_compact_status> v(n_clips);
    if (n_clips) detail::check(glc_decode_compact_last_status(ctx_, v.data(), n_clips), ctx_);
    return v;
  }

 private:
  glc_ctx *ctx_ = nullptr;
};

// The compact blob of a whole stream (glc.h glc_frames_to_compact): upload it once, decode it on the device with
// Decoder::decode_device_compact.  The vector is 8-byte aligned storage of exactly the blob's bytes.
inline std::vector<uint64_t> to_compact(const EncodedAudio &encoded, glc_compact_info *info_out = nullptr) {
  glc_compact_info info{};
  const int sized = glc_frames_to_compact(encoded.handle(), nullptr, 0, &info);
  if (sized != GLC_EINVAL || info.bytes == 0) detail::check(sized);  // a stream no blob can hold: the library says why
  std::vector<uint64_t> blob((info.bytes + 7) / 8);
  detail::check(glc_frames_to_compact(encoded.handle(), blob.data(), info.bytes, &info));
  if (info_out) *info_out = info;
  return blob;
}

// Encoder::encode followed by Decoder::decode as one call (glc.h glc_roundtrip): the samples of
// decode(encode(x)), bit for bit, with no EncodedAudio assembled on the host - the decoder reads the
// encoder's frame records where they are on the device.
class RoundTrip {
 public:
  explicit RoundTrip(uint32_t sample_rate, int device = 0) { detail::check(glc_ctx_create(device, sample_rate, &ctx_)); }
  ~RoundTrip() { glc_ctx_destroy(ctx_); }
  RoundTrip(const RoundTrip &) = delete;
  RoundTrip &operator=(const RoundTrip &) = delete;
  // float samples out (what Decoder::decode returns) ...
  std::vector<float> roundtrip(const std::vector<float> &samples, uint16_t channels) {
    return run<float>(samples.data(), GLC_PCM_F32, 32, samples.size(), channels, GLC_PCM_F32);
  }
  std::vector<float> roundtrip(const std::vector<int16_t> &samples, uint16_t channels, uint32_t bits = 16) {
    return run<float>(samples.data(), GLC_PCM_S16, bits, samples.size(), channels, GLC_PCM_F32);
  }
  std::vector<float> roundtrip(const std::vector<int32_t> &samples, uint32_t bits, uint16_t channels) {
    return run<float>(samples.data(), GLC_PCM_S32, bits, samples.size(), channels, GLC_PCM_F32);
  }
  // ... or narrowed to 16 bits on the device (what Decoder::decode_i16 returns)
  std::vector<int16_t> roundtrip_i16(const std::vector<float> &samples, uint16_t channels) {
    return run<int16_t>(samples.data(), GLC_PCM_F32, 32, samples.size(), channels, GLC_PCM_S16);
  }
  std::vector<int16_t> roundtrip_i16(const std::vector<int16_t> &samples, uint16_t channels, uint32_t bits = 16) {
    return run<int16_t>(samples.data(), GLC_PCM_S16, bits, samples.size(), channels, GLC_PCM_S16);
  }
  std::vector<int16_t> roundtrip_i16(const std::vector<int32_t> &samples, uint32_t bits, uint16_t channels) {
    return run<int16_t>(samples.data(), GLC_PCM_S32, bits, samples.size(), channels, GLC_PCM_S16);
  }
  // device-resident interleaved floats in and out, queued on the context's stream and not synchronised
  uint64_t roundtrip_device(const float *d_pcm, uint64_t n_samples, uint16_t channels, float *d_out, uint64_t cap) {
    uint64_t n = 0;
    detail::check(glc_roundtrip_device(ctx_, d_pcm, n_samples, channels, d_out, cap, &n), ctx_);
    return n;
  }
  // counts and serialized size of the stream the last call encoded (synchronises)
  glc_roundtrip_info last_info() {
    glc_roundtrip_info i{};
    detail::check(glc_roundtrip_last_info(ctx_, &i), ctx_);
    return i;
  }
  // glc_roundtrip_batch_device: every clip of a strided (interleaved or planar) device batch in one call, in place
  // when d_out == d_pcm and the layouts agree; queued, not synchronised
  void apply_batch_device(const float *d_pcm, const glc_clip_layout &in, float *d_out, const glc_clip_layout &out) {
    detail::check(glc_roundtrip_batch_device(ctx_, d_pcm, &in, d_out, &out), ctx_);
  }
  // ... from and to integer PCM (glc_roundtrip_batch_device_pcm): int16_t / int32_t clips of `bits` bits widened in the
  // gather, float or int16_t out; in place needs the same pointer, layout and format
  void apply_batch_device(const int16_t *d_pcm, uint32_t bits, const glc_clip_layout &in, float *d_out, const glc_clip_layout &out) {
    detail::check(glc_roundtrip_batch_device_pcm(ctx_, d_pcm, GLC_PCM_S16, bits, &in, d_out, GLC_PCM_F32, &out), ctx_);
  }
  void apply_batch_device(const int16_t *d_pcm, uint32_t bits, const glc_clip_layout &in, int16_t *d_out, const glc_clip_layout &out) {
    detail::check(glc_roundtrip_batch_device_pcm(ctx_, d_pcm, GLC_PCM_S16, bits, &in, d_out, GLC_PCM_S16, &out), ctx_);
  }
  void apply_batch_device(const int32_t *d_pcm, uint32_t bits, const glc_clip_layout &in, float *d_out, const glc_clip_layout &out) {
    detail::check(glc_roundtrip_batch_device_pcm(ctx_, d_pcm, GLC_PCM_S32, bits, &in, d_out, GLC_PCM_F32, &out), ctx_);
  }
  void apply_batch_device(const int32_t *d_pcm, uint32_t bits, const glc_clip_layout &in, int16_t *d_out, const glc_clip_layout &out) {
    detail::check(glc_roundtrip_batch_device_pcm(ctx_, d_pcm, GLC_PCM_S32, bits, &in, d_out, GLC_PCM_S16, &out), ctx_);
  }
  void apply_batch_device(const float *d_pcm, const glc_clip_layout &in, int16_t *d_out, const glc_clip_layout &out) {
    detail::check(glc_roundtrip_batch_device_pcm(ctx_, d_pcm, GLC_PCM_F32, 32, &in, d_out, GLC_PCM_S16, &out), ctx_);
  }
  // per clip of the last apply_batch_device what last_info gives for that clip alone (synchronises)
  std::vector<glc_roundtrip_info> last_batch_info(uint64_t n_clips) {
    std::vector<glc_roundtrip_info> v(n_clips);
    detail::check(glc_roundtrip_batch_last_info(ctx_, v.data(), n_clips), ctx_);
    return v;
  }
  void synchronize() { detail::check(glc_ctx_synchronize(ctx_), ctx_); }
  glc_ctx *ctx() { return ctx_; }

 private:
  template <typename T>
  std::vector<T> run(const void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples, uint16_t channels,
                     glc_pcm_format out_fmt) {
    std::vector<T> out(n_samples);
    uint64_t n = 0;
    detail::check(glc_roundtrip(ctx_, pcm, fmt, bits, n_samples, channels, out.data(), out_fmt, out.size(), &n), ctx_);
    out.resize(n);
    return out;
  }
  glc_ctx *ctx_ = nullptr;
};

// What a push of n_new samples per channel completes on a lane that has `received` so far (glc_plan_stream_push);
// throws where a finish ends a stream the encoder refuses.
inline glc_stream_push_plan plan_stream_push(uint64_t received, uint64_t n_new, bool finish = false) {
  glc_stream_push_plan p{};
  detail::check(glc_plan_stream_push(received, n_new, finish ? 1 : 0, &p));
  return p;
}

// Encoder::encode fed in chunks (glc.h glc_stream_enc_*): n_streams independent lanes of `channels` channels on a
// context of its own.  A lane pushed in any chunking serialises to the bytes Encoder::encode gives for the
// concatenation.  Host pushes (push / segments / encoded) or device pushes (push_device), not both on one object.
class StreamEncoder {
 public:
  struct Segment {
    uint64_t first_frame, n_frames;
    const void *blob;  // borrowed: valid until the lane is taken, reset or the object destroyed
    uint64_t bytes;
  };
  StreamEncoder(uint32_t sample_rate, uint16_t channels, uint64_t n_streams = 1, int device = 0) : channels_(channels), n_(n_streams) {
    detail::check(glc_ctx_create(device, sample_rate, &ctx_));
    const int rc = glc_stream_enc_open(ctx_, channels, n_streams, &s_);
    if (rc != GLC_OK) {
      const Error e(rc, glc_last_error(ctx_));
      glc_ctx_destroy(ctx_);
      throw e;
    }
  }
  ~StreamEncoder() {
    glc_stream_enc_close(s_);  // before its context
    glc_ctx_destroy(ctx_);
  }
  StreamEncoder(const StreamEncoder &) = delete;
  StreamEncoder &operator=(const StreamEncoder &) = delete;
  uint64_t n_streams() const { return n_; }
  uint64_t max_push() const { return glc_stream_enc_max_push(channels_); }
  // every lane at once: pcm[i] / n_samples[i] interleaved samples for lane i, finish[i] != 0 ends it (or nullptr)
  void push(const void *const *pcm, glc_pcm_format fmt, uint32_t bits, const uint64_t *n_samples, const uint8_t *finish) {
    detail::check(glc_stream_enc_push(s_, pcm, fmt, bits, n_samples, finish), ctx_);
  }
  // one lane, the others receive nothing
  void push(uint64_t stream, const float *samples, uint64_t n_samples, bool finish = false) {
    push_one(stream, samples, GLC_PCM_F32, 32, n_samples, finish);
  }
  void push(uint64_t stream, const int16_t *samples, uint64_t n_samples, bool finish = false, uint32_t bits = 16) {
    push_one(stream, samples, GLC_PCM_S16, bits, n_samples, finish);
  }
  void push(uint64_t stream, const int32_t *samples, uint32_t bits, uint64_t n_samples, bool finish = false) {
    push_one(stream, samples, GLC_PCM_S32, bits, n_samples, finish);
  }
  std::vector<Segment> segments(uint64_t stream = 0) const {
    uint64_t n = 0;
    detail::check(glc_stream_enc_segments(s_, stream, &n), ctx_);
    std::vector<Segment> v(n);
    for (uint64_t k = 0; k < n; ++k)
      detail::check(glc_stream_enc_segment(s_, stream, k, &v[k].blob, &v[k].bytes, &v[k].first_frame, &v[k].n_frames), ctx_);
    return v;
  }
  // after the finish: the lane's stream; the lane is fresh afterwards
  EncodedAudio encoded(uint64_t stream = 0) {
    glc_frames *h = nullptr;
    detail::check(glc_stream_enc_frames(s_, stream, &h), ctx_);
    return EncodedAudio(h);
  }
  void reset(uint64_t stream = 0) { detail::check(glc_stream_enc_reset(s_, stream), ctx_); }
  // glc_stream_enc_push_device: queued on the context's stream, not synchronised; returns the segments (host)
  std::vector<glc_stream_seg> push_device(const void *d_pcm, glc_pcm_format fmt, uint32_t bits, const glc_clip_layout &in,
                                          const uint8_t *finish, void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
                                          glc_store_entry *d_entries) {
    std::vector<glc_stream_seg> segs(n_);
    uint64_t n = 0;
    detail::check(glc_stream_enc_push_device(s_, d_pcm, fmt, bits, &in, finish, d_arena, arena_bytes, d_cursor, d_entries, segs.data(), &n),
                  ctx_);
    segs.resize(n);
    return segs;
  }
  // glc::join_segments_device on this context, with this encoder's channel count
  void join_segments_device(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const std::vector<glc_stream_seg> &segs,
                            const uint64_t *lengths, void *d_dst, uint64_t dst_bytes, uint64_t *d_cursor, glc_store_entry *d_entries_out,
                            int64_t *d_lengths_out, uint32_t *d_seg_status) {
    glc::join_segments_device(ctx_, d_arena, arena_bytes, d_entries, segs, lengths, channels_, d_dst, dst_bytes, d_cursor, d_entries_out,
                              d_lengths_out, d_seg_status);
  }
  // glc::cut_clips_device on this context, with this encoder's channel count
  void cut_clips_device(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, uint64_t n_entries,
                        const std::vector<glc_store_cut> &cuts, const uint64_t *lengths, void *d_dst, uint64_t dst_bytes, uint64_t *d_cursor,
                        glc_store_entry *d_entries_out, int64_t *d_lengths_out, uint32_t *d_cut_status) {
    glc::cut_clips_device(ctx_, d_arena, arena_bytes, d_entries, n_entries, cuts, lengths, channels_, d_dst, dst_bytes, d_cursor, d_entries_out,
                          d_lengths_out, d_cut_status);
  }
  void synchronize() { detail::check(glc_ctx_synchronize(ctx_), ctx_); }
  glc_ctx *ctx() { return ctx_; }
  glc_stream_enc *handle() { return s_; }

 private:
  void push_one(uint64_t stream, const void *samples, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples, bool finish) {
    if (stream >= n_) throw Error(GLC_EINVAL, "StreamEncoder::push: no such stream");
    std::vector<const void *> pcm(n_, nullptr);
    std::vector<uint64_t> ns(n_, 0);
    std::vector<uint8_t> fin(n_, 0);
    pcm[stream] = samples, ns[stream] = n_samples, fin[stream] = finish ? 1 : 0;
    push(pcm.data(), fmt, bits, ns.data(), fin.data());
  }
  glc_ctx *ctx_ = nullptr;
  glc_stream_enc *s_ = nullptr;
  uint16_t channels_ = 0;
  uint64_t n_ = 0;
};

// What a push of n_frames frames emits on a lane that has taken frames_done so far (glc_plan_stream_dec_push);
// throws where a finish's total_len does not plan to exactly frames_done + n_frames frames.
inline glc_stream_dec_plan plan_stream_dec_push(uint64_t frames_done, uint64_t n_frames, bool finish = false, uint64_t total_len = 0) {
  glc_stream_dec_plan p{};
  detail::check(glc_plan_stream_dec_push(frames_done, n_frames, finish ? 1 : 0, total_len, &p));
  return p;
}

// Decoder::decode fed in segments (glc.h glc_stream_dec_*): n_streams independent lanes of `channels` channels on a
// context of its own.  The concatenation of a lane's outputs over any chunking is bit for bit Decoder::decode of the
// stream its segments assemble to.  Host pushes (push) or device pushes (push_device), not both on one object.
class StreamDecoder {
 public:
  struct Segment {
    uint64_t first_frame, n_frames;
    const void *blob;
    uint64_t bytes;
  };
  StreamDecoder(uint32_t sample_rate, uint16_t channels, uint64_t n_streams = 1, int device = 0) : channels_(channels), n_(n_streams) {
    detail::check(glc_ctx_create(device, sample_rate, &ctx_));
    const int rc = glc_stream_dec_open(ctx_, channels, n_streams, &s_);
    if (rc != GLC_OK) {
      const Error e(rc, glc_last_error(ctx_));
      glc_ctx_destroy(ctx_);
      throw e;
    }
  }
  ~StreamDecoder() {
    glc_stream_dec_close(s_);  // before its context
    glc_ctx_destroy(ctx_);
  }
  StreamDecoder(const StreamDecoder &) = delete;
  StreamDecoder &operator=(const StreamDecoder &) = delete;
  uint64_t n_streams() const { return n_; }
  uint64_t max_push() const { return glc_stream_dec_max_push(channels_); }
  uint64_t frames_done(uint64_t stream = 0) const {
    uint64_t n = 0;
    detail::check(glc_stream_dec_frames_done(s_, stream, &n), ctx_);
    return n;
  }
  void reset(uint64_t stream = 0) { detail::check(glc_stream_dec_reset(s_, stream), ctx_); }
  // every lane at once (glc_stream_dec_push): pcm_out[i] receives n_out[i] samples of out_fmt
  void push(const void *const *blobs, const uint64_t *blob_bytes, const glc_stream_seg *segs, uint64_t n_segs, const uint8_t *finish,
            const uint64_t *total_len, void *const *pcm_out, glc_pcm_format out_fmt, uint64_t *n_out) {
    detail::check(glc_stream_dec_push(s_, blobs, blob_bytes, segs, n_segs, finish, total_len, pcm_out, out_fmt, n_out), ctx_);
  }
  // one lane, the others receive nothing: the samples its consecutive segments emit; finish with the stream's
  // samples per channel ends it
  std::vector<float> push(uint64_t stream, const std::vector<Segment> &segments, bool finish = false, uint64_t total_len = 0) {
    return push_one<float>(stream, segments, finish, total_len, GLC_PCM_F32);
  }
  std::vector<int16_t> push_i16(uint64_t stream, const std::vector<Segment> &segments, bool finish = false, uint64_t total_len = 0) {
    return push_one<int16_t>(stream, segments, finish, total_len, GLC_PCM_S16);
  }
  // glc_stream_dec_push_device: queued on the context's stream, not synchronised
  void push_device(const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const glc_stream_seg *segs, uint64_t n_segs,
                   const uint8_t *finish, const uint64_t *total_len, void *d_out, glc_pcm_format out_fmt, const glc_clip_layout &out) {
    detail::check(glc_stream_dec_push_device(s_, d_arena, arena_bytes, d_entries, segs, n_segs, finish, total_len, d_out, out_fmt, &out),
                  ctx_);
  }
  void synchronize() { detail::check(glc_ctx_synchronize(ctx_), ctx_); }
  glc_ctx *ctx() { return ctx_; }
  glc_stream_dec *handle() { return s_; }

 private:
  template <typename T>
  std::vector<T> push_one(uint64_t stream, const std::vector<Segment> &segments, bool finish, uint64_t total_len, glc_pcm_format fmt) {
    if (stream >= n_) throw Error(GLC_EINVAL, "StreamDecoder::push: no such stream");
    uint64_t frames = 0;
    std::vector<const void *> blobs;
    std::vector<uint64_t> bytes;
    std::vector<glc_stream_seg> segs;
    for (const Segment &g : segments) {
      blobs.push_back(g.blob), bytes.push_back(g.bytes), segs.push_back(glc_stream_seg{stream, g.first_frame, g.n_frames});
      frames += g.n_frames;
    }
    std::vector<T> out;
    if (!frames && !finish) return out;
    out.resize(plan_stream_dec_push(frames_done(stream), frames, finish, total_len).n_samples * channels_);
    std::vector<uint8_t> fin(n_, 0);
    std::vector<uint64_t> total(n_, 0), n_out(n_, 0);
    std::vector<void *> outs(n_, nullptr);
    fin[stream] = finish ? 1 : 0, total[stream] = total_len, outs[stream] = out.data();
    push(blobs.data(), bytes.data(), segs.data(), segs.size(), fin.data(), total.data(), outs.data(), fmt, n_out.data());
    return out;
  }
  glc_ctx *ctx_ = nullptr;
  glc_stream_dec *s_ = nullptr;
  uint16_t channels_ = 0;
  uint64_t n_ = 0;
};

// save_encoded / load_encoded — src/codec.rs:774-786
inline void save_encoded(const EncodedAudio &e, const std::string &path) { detail::check(glc_save(e.handle(), path.c_str())); }
inline EncodedAudio load_encoded(const std::string &path) {
  glc_frames *h = nullptr;
  detail::check(glc_load(path.c_str(), &h));
  return EncodedAudio(h);
}


// ---- src/audio.rs + src/flac.rs twins (host only) -----------------------------------------------
struct LoadedAudio {  // the (Vec<f32>, u32, u16) tuple of load_audio_file_lossless
  std::vector<float> samples;
  uint32_t sample_rate;
  uint16_t channels;
};
namespace detail {
inline LoadedAudio take(float *p, uint64_t n, uint32_t sr, uint16_t ch) {
  LoadedAudio a{std::vector<float>(p, p + n), sr, ch};
  glc_free(p);
  return a;
}
inline std::string lower_ext(const std::string &path) {
  const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return "";
  std::string e = path.substr(dot + 1);
  for (char &c : e) c = static_cast<char>(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c);
  return e;
}
}  // namespace detail
// load_audio_file_lossless — src/audio.rs:19-36
inline LoadedAudio load_audio_file_lossless(const std::string &path) {
  const std::string ext = detail::lower_ext(path);
  if (ext.empty()) throw Error(GLC_EINVAL, "No file extension");
  float *p = nullptr;
  uint64_t n = 0;
  uint32_t sr = 0;
  uint16_t ch = 0;
  if (ext == "wav") detail::check(glc_wav_load(path.c_str(), &p, &n, &sr, &ch));
  else if (ext == "flac") detail::check(glc_flac_load(path.c_str(), &p, &n, &sr, &ch));
  else throw Error(GLC_EINVAL, "Unsupported file format: " + ext);
  return detail::take(p, n, sr, ch);
}
// load_audio_file_lossless before the widening (glc_audio_load_pcm): the integers the file holds, in exactly one
// of the three vectors - what Encoder::encode takes together with `bits`
struct LoadedPcm {
  glc_pcm_format format;
  uint32_t bits;
  std::vector<int16_t> s16;
  std::vector<int32_t> s32;
  std::vector<float> f32;
  uint32_t sample_rate;
  uint16_t channels;
};
inline LoadedPcm load_audio_file_pcm(const std::string &path) {
  void *p = nullptr;
  LoadedPcm a{};
  uint64_t n = 0;
  detail::check(glc_audio_load_pcm(path.c_str(), &p, &a.format, &a.bits, &n, &a.sample_rate, &a.channels));
  try {
    if (a.format == GLC_PCM_S16) a.s16.assign(static_cast<int16_t *>(p), static_cast<int16_t *>(p) + n);
    else if (a.format == GLC_PCM_S32) a.s32.assign(static_cast<int32_t *>(p), static_cast<int32_t *>(p) + n);
    else a.f32.assign(static_cast<float *>(p), static_cast<float *>(p) + n);
  } catch (...) {
    glc_free(p);
    throw;
  }
  glc_free(p);
  return a;
}
// export_to_wav — src/audio.rs:100-132
inline void export_to_wav(const std::string &path, const std::vector<float> &s, uint32_t sample_rate, uint16_t channels) {
  detail::check(glc_wav_save16(path.c_str(), s.data(), s.size(), sample_rate, channels));
}
inline void export_to_wav(const std::string &path, const std::vector<int16_t> &s, uint32_t sample_rate, uint16_t channels) {
  detail::check(glc_wav_save16_i16(path.c_str(), s.data(), s.size(), sample_rate, channels));
}
// encode_flac_with_level / encode_flac — src/flac.rs:947-1063 (int16_t samples: narrowed already)
inline std::vector<uint8_t> encode_flac_with_level(const std::vector<int16_t> &s, uint32_t sample_rate, uint16_t channels,
                                                   uint8_t compression_level) {
  uint8_t *p = nullptr;
  uint64_t n = 0;
  detail::check(glc_flac_encode_i16(s.data(), s.size(), sample_rate, channels, compression_level, &p, &n));
  std::vector<uint8_t> out(p, p + n);
  glc_free(p);
  return out;
}
inline std::vector<uint8_t> encode_flac(const std::vector<int16_t> &s, uint32_t sample_rate, uint16_t channels) {
  return encode_flac_with_level(s, sample_rate, channels, 5);
}
inline void export_to_flac_with_level(const std::string &path, const std::vector<int16_t> &s, uint32_t sample_rate,
                                      uint16_t channels, uint8_t compression_level) {
  detail::check(glc_flac_save_i16(path.c_str(), s.data(), s.size(), sample_rate, channels, compression_level));
}
inline void export_to_flac(const std::string &path, const std::vector<int16_t> &s, uint32_t sample_rate, uint16_t channels) {
  export_to_flac_with_level(path, s, sample_rate, channels, 5);
}
inline std::vector<uint8_t> encode_flac_with_level(const std::vector<float> &s, uint32_t sample_rate, uint16_t channels,
                                                   uint8_t compression_level) {
  uint8_t *p = nullptr;
  uint64_t n = 0;
  detail::check(glc_flac_encode(s.data(), s.size(), sample_rate, channels, compression_level, &p, &n));
  std::vector<uint8_t> out(p, p + n);
  glc_free(p);
  return out;
}
inline std::vector<uint8_t> encode_flac(const std::vector<float> &s, uint32_t sample_rate, uint16_t channels) {
  return encode_flac_with_level(s, sample_rate, channels, 5);
}
// export_to_flac_with_level / export_to_flac — src/flac.rs:1066-1087, src/audio.rs:87-96
inline void export_to_flac_with_level(const std::string &path, const std::vector<float> &s, uint32_t sample_rate,
                                      uint16_t channels, uint8_t compression_level) {
  detail::check(glc_flac_save(path.c_str(), s.data(), s.size(), sample_rate, channels, compression_level));
}
inline void export_to_flac(const std::string &path, const std::vector<float> &s, uint32_t sample_rate, uint16_t channels) {
  export_to_flac_with_level(path, s, sample_rate, channels, 5);
}

}  // namespace glc
