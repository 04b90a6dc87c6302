// arg_rules_check.cpp - the argument rules of the device batch, store and stream calls (csrc/glc_args.hpp) on the host
// alone: the layout view, the stride rule, the frames rule, byte spans, alignment, the format rules and the message
// texts the suite asserts.  The rules sit behind a glc_ctx in the library, where every refusal test needs a device; here
// they are held by brute force over small shapes to the properties DESIGN.md section 3 ("The argument rules") states.
// Plain C++, no HIP header: built by tests/test_arg_rules.py with
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Werror tools/arg_rules_check.cpp
// Exit status 0 and the line "arg rules ok": every check held.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../gapless-lossy-codec_amd/csrc/glc_args.hpp"

static int g_failed = 0;
static char g_what[160] = "";
#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      if (++g_failed <= 20) std::printf("line %d (%s): %s does not hold\n", __LINE__, g_what, #cond);      \
    }                                                                                                     \
  } while (0)

static bool says(const char *msg, const char *part) { return msg && std::strstr(msg, part); }
static const void *ptr(uintptr_t v) { return reinterpret_cast<const void *>(v); }

// Every property of one layout.  `lens`: the per-clip lengths (all the same where `ragged` is false).
static void check_layout(uint64_t n, uint16_t ch, int planar, const std::vector<uint64_t> &lens, bool ragged, uint64_t clip_stride,
                         uint64_t channel_stride) {
  std::snprintf(g_what, sizeof g_what, "n %llu ch %u planar %d %s lens %llu.. cs %llu chs %llu", (unsigned long long)n, ch, planar,
                ragged ? "ragged" : "uniform", (unsigned long long)lens[0], (unsigned long long)clip_stride, (unsigned long long)channel_stride);
  const glc_clip_layout lay{n, ch, planar, clip_stride, channel_stride, ragged ? 0 : lens[0], ragged ? lens.data() : nullptr};
  const RtbLayout l{&lay};
  const bool planes = planar && ch > 1;
  CHECK(l.planes() == planes);  // one channel has no planes whatever `planar` says
  uint64_t longest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    CHECK(l.len(i) == lens[i]);
    CHECK(l.at(i) == i * clip_stride);
    CHECK(l.occupies(i) == (planes ? (ch - 1) * channel_stride + lens[i] : lens[i] * ch));
    longest = std::max(longest, lens[i]);
  }
  // the extent counts the LONGEST clip in the last slot
  CHECK(l.extent() == (n - 1) * clip_stride + (planes ? (ch - 1) * channel_stride + longest : longest * ch));
  // the rule, clip by clip as the calls ask it, against the two inequalities written out
  uint64_t first_bad = n;
  for (uint64_t i = 0; i < n; ++i) {
    const bool plane_short = planes && channel_stride < lens[i];
    const bool slot_short = n > 1 && clip_stride < l.occupies(i);
    const char *bad = stride_fault(l, i);
    CHECK((bad != nullptr) == (plane_short || slot_short));
    if (plane_short) CHECK(says(bad, "channel_stride") && !says(bad, "clip_stride"));
    if (!plane_short && slot_short) CHECK(says(bad, "clip_stride") && !says(bad, "channel_stride"));
    if (bad && first_bad == n) first_bad = i;
  }
  if (first_bad != n) {
    for (uint64_t i = 0; i < first_bad; ++i) CHECK(stride_fault(l, i) == nullptr);  // a loop in clip order names the lowest faulty clip
    return;
  }
  // the rule passes: every sample has an element of its own, inside its clip's slot and below the extent
  std::set<uint64_t> seen;
  uint64_t samples = 0;
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t c = 0; c < ch; ++c)
      for (uint64_t t = 0; t < lens[i]; ++t) {
        const uint64_t e = l.at(i) + (planes ? c * channel_stride + t : t * ch + c);
        seen.insert(e), ++samples;
        CHECK(e >= l.at(i) && e < l.at(i) + l.occupies(i));
        CHECK(e < l.extent());
      }
  CHECK(seen.size() == samples);
}

static void check_layouts() {
  const uint64_t kLens[] = {0, 1, 2, 5};
  for (uint64_t n = 1; n <= 3; ++n)
    for (uint16_t ch = 1; ch <= 3; ++ch)
      for (int planar = 0; planar <= 1; ++planar)
        for (uint64_t channel_stride = 0; channel_stride <= 7; ++channel_stride) {
          // ragged: every n-tuple of lengths; uniform: every length
          uint64_t tuples = 1;
          for (uint64_t i = 0; i < n; ++i) tuples *= 4;
          for (uint64_t k = 0; k < tuples + 4; ++k) {
            const bool ragged = k < tuples;
            std::vector<uint64_t> lens(n);
            for (uint64_t i = 0, r = k; i < n; ++i, r /= 4) lens[i] = ragged ? kLens[r % 4] : kLens[k - tuples];
            uint64_t occ = 0;
            for (uint64_t len : lens) occ = std::max(occ, planar && ch > 1 ? (ch - 1) * channel_stride + len : len * ch);
            for (uint64_t clip_stride = 0; clip_stride <= occ + 2; ++clip_stride) check_layout(n, ch, planar, lens, ragged, clip_stride, channel_stride);
          }
        }
  // same_as: what decides where a sample lies, and nothing else
  std::snprintf(g_what, sizeof g_what, "same_as");
  const glc_clip_layout a{2, 2, 1, 20, 7, 5, nullptr};
  glc_clip_layout b = a;
  CHECK(RtbLayout{&a}.same_as(RtbLayout{&b}));
  b.clip_stride = 21;
  CHECK(!RtbLayout{&a}.same_as(RtbLayout{&b}));
  b = a, b.channel_stride = 8;
  CHECK(!RtbLayout{&a}.same_as(RtbLayout{&b}));
  b = a, b.planar = 0;
  CHECK(!RtbLayout{&a}.same_as(RtbLayout{&b}));
  glc_clip_layout one = a, other = a;  // one clip has no next slot, interleaved clips no planes
  one.n_clips = other.n_clips = 1, other.clip_stride = 99;
  CHECK(RtbLayout{&one}.same_as(RtbLayout{&other}));
  one = other = a, one.planar = other.planar = 0, other.channel_stride = 99;
  CHECK(RtbLayout{&one}.same_as(RtbLayout{&other}));
}

// The least samples per channel whose stream of `ch` channels has `frames` frames (plan_encode ascends with the length).
static uint64_t least_len_of(uint64_t frames, uint16_t ch) {
  uint64_t lo = 513, hi = (frames + 2) * 1024;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (glc::plan_encode(mid * ch, ch).n_frames >= frames) hi = mid; else lo = mid + 1;
  }
  return lo;
}

static void check_frames() {
  for (uint16_t ch = 1; ch <= 8; ++ch) {
    std::snprintf(g_what, sizeof g_what, "frames rule, %u channels", ch);
    glc_plan plan;
    CHECK(says(frames_fault(512ull * ch, ch, &plan), "panics") && plan.n_frames == 0);
    CHECK(frames_fault(513ull * ch, ch, &plan) == nullptr && plan.n_frames >= 1);
    CHECK(says(frames_fault(0, ch, &plan), "panics"));
    // ragged channels where the one sample more of channel 0 begins another hop (512 + 1537 > 2048): the last channel is a frame short
    if (ch > 1) CHECK(says(frames_fault(1536ull * ch + 1, ch, &plan), "panics") && frames_fault(1536ull * ch, ch, &plan) == nullptr);
    // the most frames whose rows fit 32 bits, and one more
    const uint64_t most = 0xFFFFFFFFull / ch;
    const uint64_t fits = least_len_of(most, ch), beyond = least_len_of(most + 1, ch);
    CHECK(glc::plan_encode(fits * ch, ch).n_frames == most && glc::plan_encode(beyond * ch, ch).n_frames == most + 1);
    CHECK(frames_fault(fits * ch, ch, &plan) == nullptr && plan.n_frames == most);
    CHECK(frames_fault((beyond - 1) * ch, ch, &plan) == nullptr);
    CHECK(says(frames_fault(beyond * ch, ch, &plan), "stream too long") && plan.n_frames == most + 1);
    // a clip of a layout is judged through the same rule
    const glc_clip_layout ok{1, ch, 0, 0, 0, 513, nullptr}, shrt{1, ch, 0, 0, 0, 512, nullptr};
    CHECK(clip_fault(RtbLayout{&ok}, 0) == nullptr && says(clip_fault(RtbLayout{&shrt}, 0), "panics"));
  }
  std::snprintf(g_what, sizeof g_what, "frames rule, the products 2^32 - 1 and 2^32");
  glc_plan plan;
  CHECK(frames_fault(least_len_of(0xFFFFFFFFull, 1), 1, &plan) == nullptr && plan.n_frames * 1 == 0xFFFFFFFFull);
  CHECK(says(frames_fault(least_len_of(0x100000000ull, 1), 1, &plan), "stream too long") && plan.n_frames == 0x100000000ull);
  CHECK(says(frames_fault(least_len_of(0x80000000ull, 2) * 2, 2, &plan), "stream too long") && plan.n_frames * 2 == 0x100000000ull);
  CHECK(frames_fault(least_len_of(0x55555555ull, 3) * 3, 3, &plan) == nullptr && plan.n_frames * 3 == 0xFFFFFFFFull);
  // the frames rule comes before the stride rule
  const glc_clip_layout both{2, 2, 1, 0, 0, 100, nullptr};
  CHECK(says(clip_fault(RtbLayout{&both}, 0), "panics"));
}

static void check_spans() {
  std::snprintf(g_what, sizeof g_what, "spans");
  const ByteSpan a = span_of(ptr(1000), 100), next = span_of(ptr(1100), 50), last_byte = span_of(ptr(1099), 1), before = span_of(ptr(900), 100);
  CHECK(a.lo == 1000 && a.hi == 1100);
  CHECK(!overlaps(a, next) && !overlaps(next, a) && !overlaps(a, before) && !overlaps(before, a));  // adjacent
  CHECK(overlaps(a, last_byte) && overlaps(last_byte, a));                                          // one shared byte
  CHECK(overlaps(a, span_of(ptr(901), 100)) && overlaps(a, a) && overlaps(a, span_of(ptr(1010), 5)) && overlaps(span_of(ptr(0x10), 5000), a));
  // the pairwise list: the first pair in order, null and empty spans left out
  const char *x = nullptr, *y = nullptr;
  CHECK(!first_overlap({a, next, before}, &x, &y));
  CHECK(!first_overlap({}, &x, &y) && !first_overlap({a}, &x, &y));
  const ByteSpan A = span_of(ptr(1000), 100, "A"), B = span_of(ptr(2000), 100, "B"), C = span_of(ptr(1050), 1000, "C"), D = span_of(ptr(2050), 10, "D");
  CHECK(first_overlap({A, B, C, D}, &x, &y) && !std::strcmp(x, "A") && !std::strcmp(y, "C"));
  CHECK(first_overlap({B, A, D, C}, &x, &y) && !std::strcmp(x, "B") && !std::strcmp(y, "D"));
  CHECK(first_overlap({A, B, D}, &x, &y) && !std::strcmp(x, "B") && !std::strcmp(y, "D"));
  const ByteSpan null_all = span_of(nullptr, 1ull << 40, "null"), empty_in_a = span_of(ptr(1050), 0, "empty"), dflt{};
  CHECK(!first_overlap({null_all, A, empty_in_a, B, dflt}, &x, &y));
  CHECK(first_overlap({null_all, A, empty_in_a, C}, &x, &y) && !std::strcmp(x, "A") && !std::strcmp(y, "C"));
  // the bytes of a layout scale with the element: the same layout as S16 and as F32
  const uint64_t lens[3] = {5, 9, 2};
  const glc_clip_layout lay{3, 2, 1, 40, 12, 0, lens};
  const RtbLayout l{&lay};
  CHECK(l.extent() == 2 * 40 + 12 + 9);
  const ByteSpan s16 = span_of(ptr(4096), l, pcm_elem(GLC_PCM_S16)), f32 = span_of(ptr(4096), l, pcm_elem(GLC_PCM_F32));
  CHECK(s16.lo == 4096 && f32.lo == 4096 && s16.hi == 4096 + 2 * l.extent() && f32.hi == 4096 + 4 * l.extent());
  CHECK(l.end_of(ptr(4096), 4) == f32.hi);
  CHECK(overlaps(f32, span_of(ptr(s16.hi), 1)) && !overlaps(s16, span_of(ptr(s16.hi), 1)));
  // in place: the same pointer, the same layout, the same format - and nothing less
  glc_clip_layout other = lay;
  CHECK(in_place(ptr(4096), l, GLC_PCM_F32, ptr(4096), RtbLayout{&other}, GLC_PCM_F32));
  CHECK(in_place(ptr(4096), l, GLC_PCM_S16, ptr(4096), RtbLayout{&other}, GLC_PCM_S16));
  CHECK(!in_place(ptr(4096), l, GLC_PCM_F32, ptr(4100), RtbLayout{&other}, GLC_PCM_F32));
  CHECK(!in_place(ptr(4096), l, GLC_PCM_S32, ptr(4096), RtbLayout{&other}, GLC_PCM_S16));
  CHECK(!in_place(ptr(4096), l, GLC_PCM_S16, ptr(4096), RtbLayout{&other}, GLC_PCM_F32));
  other.clip_stride = 41;
  CHECK(!in_place(ptr(4096), l, GLC_PCM_F32, ptr(4096), RtbLayout{&other}, GLC_PCM_F32));
  // the calls that fill a store: the input apart from the arena and from one entry per clip
  const RtbPcm pcm{ptr(4096), GLC_PCM_S16, 16};
  const auto *ents = reinterpret_cast<const glc_store_entry *>(ptr(s16.hi));
  CHECK(store_fill_overlap(pcm, l, ptr(1 << 20), 4096, ents) == nullptr);
  CHECK(says(store_fill_overlap(pcm, l, ptr(s16.hi - 1), 4096, ents), "the arena overlaps the input"));
  CHECK(says(store_fill_overlap(pcm, l, ptr(1 << 20), 4096, reinterpret_cast<const glc_store_entry *>(ptr(4096 - 3 * sizeof(glc_store_entry) + 1))),
             "the entries overlap the input"));
  CHECK(store_fill_overlap(pcm, l, ptr(1 << 20), 4096, reinterpret_cast<const glc_store_entry *>(ptr(4096 - 3 * sizeof(glc_store_entry)))) == nullptr);
}

static void check_alignment_and_formats() {
  std::snprintf(g_what, sizeof g_what, "alignment");
  for (size_t a : {size_t(1), size_t(2), size_t(4), size_t(8), size_t(16), size_t(64)})
    for (uintptr_t base : {uintptr_t(0), uintptr_t(4096)}) {
      CHECK(aligned(ptr(base), a) && aligned(ptr(base + a), a));
      if (a > 1) CHECK(!aligned(ptr(base + 1), a) && !aligned(ptr(base + a - 1), a) && !aligned(ptr(base + a / 2), a));
    }
  CHECK(aligned(nullptr, 64));
  const char *p8 = static_cast<const char *>(ptr(4104));
  const uint64_t *p64 = static_cast<const uint64_t *>(ptr(4160));
  CHECK(all_aligned(8, p8, p64, static_cast<const void *>(nullptr)) && !all_aligned(64, p8, p64) && !all_aligned(64, p64, p8) && all_aligned(64, p64));
  const RtbPcm s16{ptr(4098), GLC_PCM_S16, 16}, s32{ptr(4098), GLC_PCM_S32, 24}, f32{ptr(4100), GLC_PCM_F32, 32};
  CHECK(store_fill_misaligned(s16, ptr(4160), ptr(8), ptr(16)) == nullptr && store_fill_misaligned(f32, ptr(4160), ptr(8), ptr(16)) == nullptr);
  CHECK(says(store_fill_misaligned(s32, ptr(4160), ptr(8), ptr(16)), "aligned to its sample size"));
  CHECK(says(store_fill_misaligned(s16, ptr(4128), ptr(8), ptr(16)), "64-byte aligned"));
  CHECK(says(store_fill_misaligned(s16, ptr(4160), ptr(12), ptr(16)), "8-byte aligned") && says(store_fill_misaligned(s16, ptr(4160), ptr(8), ptr(20)), "8-byte aligned"));

  std::snprintf(g_what, sizeof g_what, "formats");
  CHECK(pcm_elem(GLC_PCM_S16) == 2 && pcm_elem(GLC_PCM_S32) == 4 && pcm_elem(GLC_PCM_F32) == 4);
  CHECK(s16.elem() == 2 && s32.elem() == 4 && f32.elem() == 4);
  for (uint32_t bits : {0u, 1u, 16u, 17u, 32u, 33u}) {
    CHECK((fmt_fault(GLC_PCM_S16, bits) == nullptr) == (bits >= 1 && bits <= 16));
    CHECK((fmt_fault(GLC_PCM_S32, bits) == nullptr) == (bits >= 1 && bits <= 32));
    CHECK(fmt_fault(GLC_PCM_F32, bits) == nullptr);  // floats have no width to state
    CHECK(says(fmt_fault(static_cast<glc_pcm_format>(77), bits), "unknown sample format"));
  }
  CHECK(says(fmt_fault(GLC_PCM_S16, 17), "bits must be"));
  CHECK(out_fmt_fault(GLC_PCM_F32) == nullptr && out_fmt_fault(GLC_PCM_S16) == nullptr);
  CHECK(out_fmt_fault(GLC_PCM_S32) != nullptr && out_fmt_fault(static_cast<glc_pcm_format>(77)) != nullptr);
}

// The texts the suite asserts of a refusal (tests/: `in S.err()`, `in msg`, glc_last_error), through the prefix a caller
// puts in front.
static void check_messages() {
  std::snprintf(g_what, sizeof g_what, "messages");
  const glc_clip_layout narrow{2, 2, 1, 100, 4, 5, nullptr}, tight{2, 2, 0, 9, 0, 5, nullptr};
  CHECK(says(stride_fault(RtbLayout{&narrow}, 0), "channel_stride"));
  CHECK(says(stride_fault(RtbLayout{&tight}, 0), "clip_stride"));
  const std::string w = "glc_encode_batch_device_compact";
  CHECK(clip_name(w, 1) == "glc_encode_batch_device_compact: clip 1");
  const std::string msg = clip_name(w, 1) + ": " + stride_fault(RtbLayout{&tight}, 1);
  CHECK(says(msg.c_str(), "glc_encode_batch_device_compact") && says(msg.c_str(), "clip 1") && says(msg.c_str(), "clip_stride"));
  const RtbPcm odd{ptr(4097), GLC_PCM_S16, 16}, even{ptr(4096), GLC_PCM_S16, 16};
  CHECK(says(store_fill_misaligned(odd, ptr(4160), ptr(8), ptr(16)), "aligned"));
  CHECK(says(store_fill_misaligned(even, ptr(4128), ptr(8), ptr(16)), "64-byte"));
  CHECK(says(store_fill_misaligned(even, ptr(4160), ptr(4), ptr(16)), "8-byte"));
  const glc_clip_layout lay{1, 1, 0, 0, 0, 1000, nullptr};
  CHECK(says(store_fill_overlap(even, RtbLayout{&lay}, ptr(4096 + 64), 64, static_cast<const glc_store_entry *>(ptr(8))), "overlaps"));
  CHECK(says(out_fmt_fault(GLC_PCM_S32), "GLC_PCM_F32 or GLC_PCM_S16") && says(out_fmt_fault(GLC_PCM_S32), "out_fmt"));
  glc_plan plan;
  CHECK(says(frames_fault(1024, 2, &plan), "512"));
}

int main() {
  check_layouts();
  check_frames();
  check_spans();
  check_alignment_and_formats();
  check_messages();
  if (g_failed) {
    std::printf("arg rules: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("arg rules ok\n");
  return 0;
}
