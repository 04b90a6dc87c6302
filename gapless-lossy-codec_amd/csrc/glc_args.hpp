// glc_args.hpp — what the device batch, store and stream calls of glc_api.hip refuse of their arguments, each rule
// stated once ("The argument rules").  Plain C++17 without a HIP type and without glc_ctx: a host
// program can include it alone (tools/arg_rules_check.cpp).  A rule returns what it found - the tail of the message, or
// null where nothing is wrong - and its caller turns that into fail(ctx, GLC_EINVAL, prefix + ": " + text), so the name
// of a clip is built only where there is a fault to report.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "glc_common.h"

// ------------------------------------------------------------------------------ formats

// Bytes of a sample of `fmt`.
static inline size_t pcm_elem(glc_pcm_format fmt) { return fmt == GLC_PCM_S16 ? 2 : 4; }

// What the integer twins check of `fmt` and `bits`, as glc_encode_int does.
static inline const char *fmt_fault(glc_pcm_format fmt, uint32_t bits) {
  if (fmt != GLC_PCM_S16 && fmt != GLC_PCM_S32 && fmt != GLC_PCM_F32) return "unknown sample format";
  if (fmt != GLC_PCM_F32 && (bits == 0 || bits > (fmt == GLC_PCM_S16 ? 16u : 32u)))
    return "bits must be 1..16 for 16-bit samples, 1..32 for 32-bit ones";
  return nullptr;
}

// D2 writes floats, or narrows to 16 bits: there is no 32-bit integer output.
static inline const char *out_fmt_fault(glc_pcm_format out_fmt) {
  return out_fmt != GLC_PCM_F32 && out_fmt != GLC_PCM_S16 ? "out_fmt must be GLC_PCM_F32 or GLC_PCM_S16" : nullptr;
}

// The input of a batch call: device samples of `fmt` (`bits` wide for the integer formats), the layout counting
// elements of that type.  S1 widens the integers in its gather (glc::launch_stage_clips_int).
struct RtbPcm {
  const void *p;
  glc_pcm_format fmt;
  uint32_t bits;
  size_t elem() const { return pcm_elem(fmt); }
};

// ------------------------------------------------------------------------------ alignment

// `a` is a power of two.  A null pointer is aligned to everything: whether it may be null is another rule.
static inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
template <typename... P>
static bool all_aligned(size_t a, const P *...p) { return (aligned(p, a) && ...); }

// ------------------------------------------------------------------------------ the layout view

// Where clip i of a glc_clip_layout starts, what it occupies, and the extent of the whole layout, in elements.
struct RtbLayout {
  const glc_clip_layout *l;
  uint64_t len(uint64_t i) const { return l->lengths ? l->lengths[i] : l->length; }
  uint64_t at(uint64_t i) const { return i * l->clip_stride; }
  bool planes() const { return l->planar && l->channels > 1; }
  uint64_t occupied_by(uint64_t n) const { return planes() ? (l->channels - 1ull) * l->channel_stride + n : n * l->channels; }
  uint64_t occupies(uint64_t i) const { return occupied_by(len(i)); }
  // The extent is that of the padded batch: every clip slot counts with the length of the LONGEST clip, so the padding
  // behind a short last clip belongs to the batch too and no second buffer may begin inside it.
  uint64_t extent() const {
    uint64_t longest = 0;
    for (uint64_t i = 0; i < l->n_clips; ++i) longest = std::max(longest, len(i));
    return at(l->n_clips - 1) + occupied_by(longest);
  }
  bool same_as(const RtbLayout &o) const {
    return planes() == o.planes() && (l->n_clips <= 1 || l->clip_stride == o.l->clip_stride) &&
           (!planes() || l->channel_stride == o.l->channel_stride);
  }
  // The bytes [p, p + extent() * elem) of the batch at `p`, whose elements are `elem` bytes wide: overlap is judged on
  // BYTES, the layouts of a call may count elements of different widths.
  uintptr_t end_of(const void *p, size_t elem) const { return reinterpret_cast<uintptr_t>(p) + extent() * elem; }
};

// THE stride rule, of clip i: its planes do not run into each other, and (where there is a next slot) the clip does not
// run into it.  Judges a clip of length 0 like any other; a caller that skips lanes which bring nothing skips them
// itself.
static inline const char *stride_fault(const RtbLayout &l, uint64_t i) {
  if (l.planes() && l.l->channel_stride < l.len(i)) return "channel_stride is smaller than a plane";
  if (l.l->n_clips > 1 && l.l->clip_stride < l.occupies(i)) return "clip_stride is smaller than the clip";
  return nullptr;
}

// THE frames rule, of a clip of n_samples interleaved samples (len * channels for a clip of a layout; channels != 0):
// the encoder takes it, and its rows fit the 32-bit row index of the kernels.  *plan: plan_encode of it, fault or not.
static inline const char *frames_fault(uint64_t n_samples, uint16_t channels, glc_plan *plan) {
  *plan = glc::plan_encode(n_samples, channels);
  if (plan->n_frames == 0) return "the reference encoder panics on this input (<= 512 samples per channel, or ragged channels)";
  if (plan->n_frames * channels > 0xFFFFFFFFull) return "stream too long";
  return nullptr;
}

// What every batch call over a glc_clip_layout refuses of clip i: the frames rule, then the stride rule.
static inline const char *clip_fault(const RtbLayout &l, uint64_t i) {
  glc_plan plan;
  if (const char *bad = frames_fault(l.len(i) * l.l->channels, l.l->channels, &plan)) return bad;
  return stride_fault(l, i);
}

// prefix + ": clip i", for the message of a fault
static inline std::string clip_name(const std::string &w, uint64_t i) { return w + ": clip " + std::to_string(i); }

// ------------------------------------------------------------------------------ byte spans

// The bytes [lo, hi) an argument covers, and what a message calls it.
struct ByteSpan {
  uintptr_t lo = 0, hi = 0;
  const char *name = "";
};
static inline ByteSpan span_of(const void *p, uint64_t bytes, const char *name = "") {
  return ByteSpan{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes, name};
}
static inline ByteSpan span_of(const void *p, const RtbLayout &l, size_t elem, const char *name = "") {
  return ByteSpan{reinterpret_cast<uintptr_t>(p), l.end_of(p, elem), name};
}
static inline bool overlaps(const ByteSpan &a, const ByteSpan &b) { return a.lo < b.hi && b.lo < a.hi; }

// The first pair of a list that overlaps, in the order (0,1), (0,2), .. (1,2), ..; spans of a null pointer and empty
// spans take no part.  *a, *b: the names of the two (the list itself may be gone when the caller reports them).
// false: no two overlap.
static inline bool first_overlap(std::initializer_list<ByteSpan> spans, const char **a, const char **b) {
  auto counts = [](const ByteSpan &s) { return s.lo != 0 && s.hi != s.lo; };
  for (const ByteSpan *i = spans.begin(); i != spans.end(); ++i)
    for (const ByteSpan *j = i + 1; counts(*i) && j != spans.end(); ++j)
      if (counts(*j) && overlaps(*i, *j)) {
        *a = i->name, *b = j->name;
        return true;
      }
  return false;
}

// What the calls that fill a store from device PCM - the store encode and the device push of a streaming encode - check
// alike of where they read and write: the alignment of the four pointers, and that the input's extent lies apart from
// the arena and from the entries (one per clip of the layout).
static inline const char *store_fill_misaligned(const RtbPcm &pcm, const void *d_arena, const void *d_cursor, const void *d_entries) {
  if (!aligned(pcm.p, pcm.elem())) return "d_pcm is not aligned to its sample size";
  if (!aligned(d_arena, 64)) return "d_arena is not 64-byte aligned";
  if (!all_aligned(8, d_cursor, d_entries)) return "d_cursor and d_entries must be 8-byte aligned";
  return nullptr;
}
static inline const char *store_fill_overlap(const RtbPcm &pcm, const RtbLayout &in, const void *d_arena, uint64_t arena_bytes,
                                             const glc_store_entry *d_entries) {
  const ByteSpan input = span_of(pcm.p, in, pcm.elem());
  if (overlaps(input, span_of(d_arena, arena_bytes))) return "the arena overlaps the input";
  if (overlaps(input, span_of(d_entries, in.l->n_clips * sizeof(glc_store_entry)))) return "the entries overlap the input";
  return nullptr;
}

// THE segment rule of the join (glc_store_join_segments_device): segs ascends by (stream, first_frame); the segments of
// one stream value are one clip - consecutive, the first at frame 0, each with frames, each starting where the one
// before ends -, the clips numbered in order of appearance; a clip's frames pass the 32-bit row limit of frames_fault
// and, where lengths are given, are exactly plan_encode(lengths[c], 1).n_frames.  *clips: per clip {first segment,
// segments, frames}, fault or not; *at: the segment or (*of_clip, the last two rules) the clip the fault names.
struct JoinClipSpan {
  uint64_t seg_first, n_segs, n_frames;
};
static inline const char *join_segs_fault(const glc_stream_seg *segs, uint64_t n_segs, const uint64_t *lengths, uint16_t channels,
                                          std::vector<JoinClipSpan> *clips, uint64_t *at, bool *of_clip) {
  clips->clear();
  *of_clip = false;
  for (uint64_t j = 0; j < n_segs; ++j) {
    *at = j;
    if (segs[j].n_frames == 0) return "no frames";
    const bool fresh = j == 0 || segs[j].stream != segs[j - 1].stream;
    if (fresh) {
      if (j && segs[j].stream < segs[j - 1].stream) return "the segments do not ascend by stream and frame";
      if (segs[j].first_frame != 0) return "a clip's first segment must start at frame 0";
      clips->push_back(JoinClipSpan{j, 0, 0});
    } else if (segs[j].first_frame != clips->back().n_frames) {
      return segs[j].first_frame < clips->back().n_frames ? "the segments do not ascend by stream and frame"
                                                          : "it does not start where its clip's frames end";
    }
    JoinClipSpan &c = clips->back();
    if (segs[j].n_frames > 0xFFFFFFFFull - c.n_frames) return "stream too long";
    c.n_frames += segs[j].n_frames, c.n_segs += 1;
  }
  *of_clip = true;
  for (uint64_t c = 0; c < clips->size(); ++c) {
    *at = c;
    if ((*clips)[c].n_frames * channels > 0xFFFFFFFFull) return "stream too long";
    if (lengths && glc::plan_encode(lengths[c], 1).n_frames != (*clips)[c].n_frames)
      return "the segments' frames are not those of a clip of lengths[c] samples (glc_plan_encode)";
  }
  return nullptr;
}

// THE cut rule (glc_store_cut_device): every cut has frames, its piece's rows pass the 32-bit row limit of frames_fault
// and, where lengths are given, its frames are exactly plan_encode(lengths[i], 1).n_frames.  Which clip a cut names and
// where its window lies are judged on the device, against an index and headers the host never reads.  *at: the cut.
static inline const char *cuts_fault(const glc_store_cut *cuts, uint64_t n_cuts, const uint64_t *lengths, uint16_t channels, uint64_t *at) {
  for (uint64_t i = 0; i < n_cuts; ++i) {
    *at = i;
    if (cuts[i].n_frames == 0) return "no frames";
    if (cuts[i].n_frames > 0xFFFFFFFFull / channels) return "stream too long";
    if (lengths && glc::plan_encode(lengths[i], 1).n_frames != cuts[i].n_frames)
      return "n_frames is not the frame count of a clip of lengths[i] samples (glc_plan_encode)";
  }
  return nullptr;
}

// The one overlap of input and output the batch round trip allows: in place - the same pointer, the same layout and the
// same format, so that every sample is read before the slot it lies in is written.
static inline bool in_place(const void *in, const RtbLayout &li, glc_pcm_format fmt, const void *out, const RtbLayout &lo,
                            glc_pcm_format out_fmt) {
  return in == out && li.same_as(lo) && fmt == out_fmt;
}
