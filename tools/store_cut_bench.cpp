// store_cut_bench.cpp — what cutting stored clips into frame ranges costs: glc_store_cut_device against the plain mover,
// against the join's mover and against what a caller does without it, for a store the batch encode has just filled.
//   (a) the cut of every clip into 20 pieces                      (store 1: 512 stereo clips of 10 s)
//   (b) the cut of every clip into 100 ms pieces                  (store 2: 64 stereo clips of 60 s)
//   (c) every clip cut as ONE piece: the whole clip, source and destination co-aligned
//   (d) glc_store_compact_device out of place over the same store, every clip kept: the co-aligned gather moving the same
//       blobs - the ceiling for a mover
//   (e) glc_store_join_segments_device over the pieces of (a) / (b): the mover that searches per unit, the other way
//   (f) today's path: the entries and the used arena downloaded, glc_compact_cut per piece, the pieces and their entries
//       uploaded
// Per call and arm: the device time (two events on the context's stream around the call), the host wall time INSIDE the
// call, and the pieces' bytes per second of device time ((f): of host time, where it spends it).  All arms in one
// process and one session, interleaved after a warm-up; the cut runs twice per round and the difference of its two
// medians is the run's own A/A spread.  Before anything is timed the arena and entries of the cut are compared with
// those of (f), and the join of the pieces with the source store.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_cut_bench [reps = 10]
//        build/store_cut_bench trace [clips = 512] [seconds = 10] [pieces = 20]
//                                                    3 warm-up + 10 cuts and nothing else (for a kernel and memory-copy
//                                                    trace): clips of `seconds` in `pieces` pieces each
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glc.h"

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Stat {
  double med, p10, p90;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v[v.size() / 10], v[v.size() * 9 / 10]};
}

#define CHECK(call)                                                   \
  do {                                                                \
    if ((call) != GLC_OK) {                                           \
      std::printf("%s failed: %s\n", #call, glc_last_error(nullptr)); \
      return 1;                                                       \
    }                                                                 \
  } while (0)
#define HIPCHECK(call)                                               \
  do {                                                               \
    const hipError_t e__ = (call);                                   \
    if (e__ != hipSuccess) {                                         \
      std::printf("%s failed: %s\n", #call, hipGetErrorString(e__)); \
      return 1;                                                      \
    }                                                                \
  } while (0)

// the signal of store_compact_bench: eight partials per channel, clip i a cut at its own offset, every fourth clip noise
static std::vector<float> base_signal(uint32_t sr, uint16_t ch, uint64_t period) {
  std::vector<float> x(period * ch);
  for (uint16_t c = 0; c < ch; ++c)
    for (uint64_t t = 0; t < period; ++t) {
      double v = 0;
      for (int p = 0; p < 8; ++p) v += 0.05 * std::sin(2 * M_PI * (110.0 * (p + 1) * (1.0 + 0.37 * c) + 3.1 * p) * t / sr + 0.5 * p);
      x[t * ch + c] = static_cast<float>(v);
    }
  return x;
}
static void fill_clip(std::vector<float> &x, const std::vector<float> &base, uint16_t ch, uint64_t clip, bool noise) {
  if (noise) {
    uint32_t s = 12345u + static_cast<uint32_t>(clip);
    for (float &v : x) {
      s = 1664525u * s + 1013904223u;
      v = static_cast<float>(0.5 * (s / 2147483648.0 - 1.0));
    }
    return;
  }
  const uint64_t period = base.size() / ch, off = (997 * clip) % period;
  for (uint64_t t = 0, n = x.size() / ch; t < n; ++t) std::memcpy(&x[t * ch], &base[((t + off) % period) * ch], ch * sizeof(float));
}

constexpr uint32_t kSr = 48000;
constexpr uint16_t kCh = 2;

struct Store {
  glc_ctx *ctx = nullptr;
  hipStream_t st = nullptr;
  uint64_t n_clips = 0, clip_len = 0, frames = 0, used = 0, dst_bytes = 0;  // used: the source arena's cursor
  void *d_arena = nullptr, *d_dst = nullptr, *d_dst2 = nullptr;
  glc_store_entry *d_entries = nullptr, *d_entries_out = nullptr, *d_entries_out2 = nullptr;
  int64_t *d_lengths_out = nullptr, *d_new_index = nullptr;
  uint32_t *d_status = nullptr;
  uint8_t *d_keep = nullptr;
  uint64_t *d_counts = nullptr, *d_cursor = nullptr;
  uint64_t max_pieces = 0;
};

// n_clips clips of clip_len samples per channel through the batch encode: the store a corpus lies in
static int fill_store(Store &s, uint64_t n_clips, uint64_t clip_len, uint64_t max_pieces_per_clip) {
  const uint64_t n = clip_len * kCh;
  CHECK(glc_ctx_create(0, kSr, &s.ctx));
  s.st = static_cast<hipStream_t>(glc_ctx_stream(s.ctx));
  s.n_clips = n_clips, s.clip_len = clip_len, s.max_pieces = n_clips * max_pieces_per_clip;
  glc_plan plan{};
  CHECK(glc_plan_encode(n, kCh, &plan));
  s.frames = plan.n_frames;
  const glc_clip_layout whole{n_clips, kCh, 0, n, 0, clip_len, nullptr};
  const uint64_t arena_bytes = glc_compact_store_bound(&whole);
  s.dst_bytes = arena_bytes + s.max_pieces * 1024;  // a piece adds its header and the padding of its sections
  float *d_pcm = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&s.d_arena, arena_bytes));
  HIPCHECK(hipMalloc(&s.d_cursor, 8));
  HIPCHECK(hipMalloc(&s.d_entries, n_clips * sizeof(glc_store_entry)));
  {
    const std::vector<float> base = base_signal(kSr, kCh, 10ull * kSr);
    std::vector<float> x(n);
    for (uint64_t i = 0; i < n_clips; ++i) {
      fill_clip(x, base, kCh, i, i % 4 == 3);
      HIPCHECK(hipMemcpy(d_pcm + i * n, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIPCHECK(hipMemset(s.d_cursor, 0, 8));
  CHECK(glc_encode_batch_device_compact(s.ctx, d_pcm, &whole, s.d_arena, arena_bytes, s.d_cursor, s.d_entries));
  CHECK(glc_ctx_synchronize(s.ctx));
  HIPCHECK(hipMemcpy(&s.used, s.d_cursor, 8, hipMemcpyDeviceToHost));
  (void)hipFree(d_pcm);
  HIPCHECK(hipMalloc(&s.d_dst, s.dst_bytes));
  HIPCHECK(hipMalloc(&s.d_dst2, s.dst_bytes));
  HIPCHECK(hipMalloc(&s.d_entries_out, s.max_pieces * sizeof(glc_store_entry)));
  HIPCHECK(hipMalloc(&s.d_entries_out2, s.max_pieces * sizeof(glc_store_entry)));
  HIPCHECK(hipMalloc(&s.d_lengths_out, s.max_pieces * 8));
  HIPCHECK(hipMalloc(&s.d_status, s.max_pieces * 4));
  HIPCHECK(hipMalloc(&s.d_keep, n_clips));
  HIPCHECK(hipMemset(s.d_keep, 1, n_clips));
  HIPCHECK(hipMalloc(&s.d_new_index, n_clips * 8));
  HIPCHECK(hipMalloc(&s.d_counts, 16));
  return 0;
}

static void free_store(Store &s) {
  (void)hipFree(s.d_arena), (void)hipFree(s.d_dst), (void)hipFree(s.d_dst2), (void)hipFree(s.d_entries), (void)hipFree(s.d_entries_out);
  (void)hipFree(s.d_entries_out2), (void)hipFree(s.d_lengths_out), (void)hipFree(s.d_status), (void)hipFree(s.d_keep);
  (void)hipFree(s.d_new_index), (void)hipFree(s.d_counts), (void)hipFree(s.d_cursor);
  glc_ctx_destroy(s.ctx);
  s = Store{};
}

// every clip in `per_clip` pieces whose seams are those of equal chunks of samples (piece k starts at the frame that
// holds sample k * clip_len / per_clip): clip by clip, in frame order
static std::vector<glc_store_cut> pieces_of(const Store &s, uint64_t per_clip) {
  std::vector<glc_store_cut> cuts;
  for (uint64_t c = 0; c < s.n_clips; ++c)
    for (uint64_t k = 0; k < per_clip; ++k) {
      const uint64_t f0 = k * s.frames / per_clip, f1 = (k + 1) * s.frames / per_clip;
      if (f1 > f0) cuts.push_back(glc_store_cut{c, f0, f1 - f0});
    }
  return cuts;
}

static int call_cut(Store &s, const std::vector<glc_store_cut> &cuts) {
  HIPCHECK(hipMemsetAsync(s.d_cursor, 0, 8, s.st));  // every cut starts the destination store afresh
  return glc_store_cut_device(s.ctx, s.d_arena, s.used, s.d_entries, s.n_clips, cuts.data(), cuts.size(), nullptr, kCh, s.d_dst, s.dst_bytes,
                              s.d_cursor, s.d_entries_out, s.d_lengths_out, s.d_status);
}

static int call_gather(Store &s) {
  return glc_store_compact_device(s.ctx, s.d_arena, s.used, s.d_entries, nullptr, s.n_clips, s.d_keep, s.d_dst2, s.dst_bytes, s.d_entries_out2,
                                  nullptr, s.d_new_index, s.d_counts, s.d_counts + 1);
}

// the join of the pieces the last cut left in d_dst / d_entries_out, into d_dst2
static int call_join(Store &s, const std::vector<glc_stream_seg> &segs, uint64_t pieces_bytes) {
  HIPCHECK(hipMemsetAsync(s.d_counts, 0, 8, s.st));
  return glc_store_join_segments_device(s.ctx, s.d_dst, pieces_bytes, s.d_entries_out, segs.data(), segs.size(), nullptr, kCh, s.d_dst2,
                                        s.dst_bytes, s.d_counts, s.d_entries_out2, nullptr, s.d_status);
}

// today's path, into d_dst2 / d_entries_out2; `out`, `out_entries`: what it uploads
static int call_today(Store &s, const std::vector<glc_store_cut> &cuts, std::vector<uint8_t> &down, std::vector<glc_store_entry> &ents,
                      std::vector<uint8_t> &out, std::vector<glc_store_entry> &out_entries, uint64_t *bytes) {
  HIPCHECK(hipMemcpyAsync(ents.data(), s.d_entries, ents.size() * sizeof(glc_store_entry), hipMemcpyDeviceToHost, s.st));
  HIPCHECK(hipMemcpyAsync(down.data(), s.d_arena, s.used, hipMemcpyDeviceToHost, s.st));
  HIPCHECK(hipStreamSynchronize(s.st));
  uint64_t at = 0;
  for (size_t i = 0; i < cuts.size(); ++i) {
    const glc_store_entry &e = ents[cuts[i].clip];
    glc_compact_info info{};
    CHECK(glc_compact_cut(down.data() + e.offset, e.bytes, kCh, cuts[i].first_frame, cuts[i].n_frames, out.data() + at, out.size() - at, &info));
    out_entries[i] = glc_store_entry{at, info.bytes, info.n_pairs, static_cast<uint32_t>(info.n_raw_rows), 1u};
    at += info.bytes;
  }
  HIPCHECK(hipMemcpyAsync(s.d_dst2, out.data(), at, hipMemcpyHostToDevice, s.st));
  HIPCHECK(hipMemcpyAsync(s.d_entries_out2, out_entries.data(), cuts.size() * sizeof(glc_store_entry), hipMemcpyHostToDevice, s.st));
  if (bytes) *bytes = at;
  return 0;
}

template <typename F>
static int timed(Store &s, hipEvent_t ev0, hipEvent_t ev1, F &&fn, std::vector<double> *host, std::vector<double> *dev) {
  if (hipEventRecord(ev0, s.st) != hipSuccess) return 1;
  const double t0 = now_ms();
  const int rc = fn();
  const double t1 = now_ms();
  if (rc) return rc;
  if (hipEventRecord(ev1, s.st) != hipSuccess || hipEventSynchronize(ev1) != hipSuccess) return 1;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return 1;
  if (host) host->push_back(t1 - t0), dev->push_back(ms);
  return 0;
}

// arms of one store: the cut into `per_clip` pieces (label `cut_name`), the cut into one piece, the gather, the join, today
static int run_store(Store &s, const char *name, const char *cut_name, uint64_t per_clip, int reps) {
  const std::vector<glc_store_cut> cuts = pieces_of(s, per_clip), whole = pieces_of(s, 1);
  std::vector<glc_stream_seg> segs;
  for (const glc_store_cut &c : cuts) segs.push_back(glc_stream_seg{c.clip, c.first_frame, c.n_frames});
  std::vector<uint8_t> down(s.used), out(s.dst_bytes);
  std::vector<glc_store_entry> ents(s.n_clips), today(cuts.size()), got(cuts.size());
  // ---- before anything is timed: the cut is today's path byte for byte, and the join of the pieces is the source store
  uint64_t pieces_bytes = 0, today_bytes = 0;
  {
    if (call_today(s, cuts, down, ents, out, today, &today_bytes)) return 1;
    HIPCHECK(hipStreamSynchronize(s.st));
    if (call_cut(s, cuts)) return std::printf("the cut failed: %s\n", glc_last_error(nullptr)), 1;
    CHECK(glc_ctx_synchronize(s.ctx));
    HIPCHECK(hipMemcpy(&pieces_bytes, s.d_cursor, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(got.data(), s.d_entries_out, cuts.size() * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
    std::vector<uint8_t> x(pieces_bytes);
    HIPCHECK(hipMemcpy(x.data(), s.d_dst, pieces_bytes, hipMemcpyDeviceToHost));
    if (pieces_bytes != today_bytes || std::memcmp(got.data(), today.data(), cuts.size() * sizeof(glc_store_entry)) ||
        std::memcmp(x.data(), out.data(), pieces_bytes))
      return std::printf("%s: the cut differs from glc_compact_cut of the downloaded store\n", name), 1;
    if (call_join(s, segs, pieces_bytes)) return std::printf("the join failed: %s\n", glc_last_error(nullptr)), 1;
    CHECK(glc_ctx_synchronize(s.ctx));
    std::vector<glc_store_entry> joined(s.n_clips);
    HIPCHECK(hipMemcpy(joined.data(), s.d_entries_out2, s.n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
    std::vector<uint8_t> y(s.used);
    HIPCHECK(hipMemcpy(y.data(), s.d_dst2, s.used, hipMemcpyDeviceToHost));
    for (uint64_t c = 0; c < s.n_clips; ++c)
      if (!joined[c].stored || joined[c].bytes != ents[c].bytes || std::memcmp(y.data() + joined[c].offset, down.data() + ents[c].offset, ents[c].bytes))
        return std::printf("%s: the join of the pieces of clip %llu is not the clip\n", name, (unsigned long long)c), 1;
  }
  hipEvent_t ev0, ev1;
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  auto arm_cut = [&] { return call_cut(s, cuts); };
  auto arm_whole = [&] { return call_cut(s, whole); };
  auto arm_gather = [&] { return call_gather(s); };
  auto arm_join = [&] { return call_join(s, segs, pieces_bytes); };
  auto arm_today = [&] { return call_today(s, cuts, down, ents, out, today, nullptr); };
  std::vector<double> h[6], d[6];
  for (int i = -std::max(2, reps / 5); i < reps; ++i) {
    const bool keep_it = i >= 0;
    if (timed(s, ev0, ev1, arm_cut, keep_it ? &h[0] : nullptr, &d[0])) return 1;
    if (timed(s, ev0, ev1, arm_join, keep_it ? &h[3] : nullptr, &d[3])) return 1;  // behind the cut: its pieces lie in d_dst
    if (timed(s, ev0, ev1, arm_whole, keep_it ? &h[1] : nullptr, &d[1])) return 1;
    if (timed(s, ev0, ev1, arm_gather, keep_it ? &h[2] : nullptr, &d[2])) return 1;
    if (keep_it && i < 3 && timed(s, ev0, ev1, arm_today, &h[4], &d[4])) return 1;  // tens of milliseconds of host work: three reps
    if (timed(s, ev0, ev1, arm_cut, keep_it ? &h[5] : nullptr, &d[5])) return 1;
  }
  std::printf("%s: %llu pieces of %llu clips of %llu frames, %.1f MiB of clips cut to %.1f MiB of pieces; %d interleaved reps, 3 of (f) "
              "(ms per call: median [p10 .. p90])\n", name, (unsigned long long)cuts.size(), (unsigned long long)s.n_clips,
              (unsigned long long)s.frames, s.used / 1048576.0, pieces_bytes / 1048576.0, reps);
  std::printf("  the cut equals glc_compact_cut of the downloaded store, and the join of its pieces the source store\n");
  const Stat a1d = stat(d[0]), a2d = stat(d[5]), a1h = stat(h[0]), a2h = stat(h[5]);
  std::printf("  A/A spread of %s: device %.4f, host %.4f\n", cut_name, std::fabs(a1d.med - a2d.med), std::fabs(a1h.med - a2h.med));
  const char *names[5] = {cut_name, "(c) every clip as one piece                        ", "(d) glc_store_compact_device out of place, all kept",
                          "(e) glc_store_join_segments_device over the pieces ", "(f) download, glc_compact_cut per piece, upload    "};
  const double moved[5] = {double(pieces_bytes), double(s.used), double(s.used), double(s.used), double(pieces_bytes)};
  for (int k = 0; k < 5; ++k) {
    const Stat D = stat(d[k]), H = stat(h[k]);
    std::printf("  %s device %.4f [%.4f .. %.4f]   host %.4f [%.4f .. %.4f]   %.1f GB/s written bytes\n", names[k], D.med, D.p10, D.p90, H.med,
                H.p10, H.p90, D.med > 0 ? moved[k] / D.med / 1e6 : 0.0);
  }
  (void)hipEventDestroy(ev0), (void)hipEventDestroy(ev1);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "trace")) {
    const uint64_t n = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 512;
    const uint64_t seconds = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 10, per_clip = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 20;
    Store s;
    if (n == 0 || seconds == 0 || per_clip == 0 || fill_store(s, n, seconds * kSr, per_clip)) return 1;
    const std::vector<glc_store_cut> cuts = pieces_of(s, per_clip);
    for (int i = 0; i < 13; ++i) {
      if (call_cut(s, cuts)) return std::printf("the cut failed: %s\n", glc_last_error(nullptr)), 1;
      CHECK(glc_ctx_synchronize(s.ctx));
    }
    std::printf("trace: 3 warm-up + 10 cuts, %llu clips of %llu s in %llu pieces each\n", (unsigned long long)n, (unsigned long long)seconds,
                (unsigned long long)per_clip);
    free_store(s);
    return 0;
  }
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 10;
  const struct {
    const char *name, *cut_name;
    uint64_t clips, seconds, per_clip;
  } stores[2] = {{"512 clips of 10 s", "(a) glc_store_cut_device, 20 pieces per clip       ", 512, 10, 20},
                 {"64 clips of 60 s", "(b) glc_store_cut_device, 100 ms pieces            ", 64, 60, 600}};
  for (const auto &st : stores) {
    Store s;
    if (fill_store(s, st.clips, st.seconds * kSr, st.per_clip)) return 1;
    if (run_store(s, st.name, st.cut_name, st.per_clip, reps)) return 1;
    free_store(s);
  }
  return 0;
}
