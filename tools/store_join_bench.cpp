// store_join_bench.cpp — what joining a streamed clip's segments into one store blob costs: glc_store_join_segments_device
// against the plain mover and against what a caller does without it, for a store the streaming encoder has just filled.
//   (a) the join: the segments of every clip into one blob per clip in a second arena
//   (b) glc_store_compact_device out of place over the JOINED store, every clip kept: the co-aligned gather moving the
//       same number of bytes - the ceiling for a mover
//   (c) today's path: the entries and the used arena downloaded, per clip glc_frames_from_compact over its segments and
//       glc_frames_to_compact, the blobs and the new entries uploaded
// Per call and arm: the device time (two events on the context's stream around the call), the host wall time INSIDE the
// call, and the joined bytes per second of device time ((c): of host time, where it spends it).  All arms in one
// process and one session, interleaved a b c a' after a warm-up; a' is the join again and the difference of its two
// medians is the run's own A/A spread.  The joined arena and entries of (a) are compared with those of (c) before
// anything is timed.
// Stores, 48 kHz stereo, every fourth clip noise: 512 clips of 10 s in 20 segments each; 64 clips of 60 s in 100 ms
// segments; 512 clips of 10 s in one segment.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_join_bench [reps = 10]
//        build/store_join_bench trace [clips = 512]   3 warm-up + 10 joins and nothing else (for a kernel and memory-copy
//                                                     trace): clips of 10 s in 20 segments
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
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
  uint64_t n_clips = 0, clip_len = 0, used = 0, arena_bytes = 0, dst_bytes = 0;  // used: the segment arena's cursor
  void *d_arena = nullptr, *d_dst = nullptr, *d_dst2 = nullptr;
  glc_store_entry *d_entries = nullptr, *d_entries_out = nullptr, *d_entries_out2 = nullptr;
  uint32_t *d_status = nullptr;
  uint8_t *d_keep = nullptr;
  int64_t *d_new_index = nullptr;
  uint64_t *d_counts = nullptr, *d_cursor = nullptr;
  std::vector<glc_stream_seg> segs;       // ascending by (stream, first_frame)
  std::vector<glc_store_entry> entries;   // in that order
  std::vector<uint64_t> lengths;
  std::vector<uint8_t> ref;                // the store glc_encode_batch_device_compact fills from the same clips
  std::vector<glc_store_entry> ref_entries;
};

// n_clips lanes of clip_len samples per channel pushed in chunks of `chunk`: the store a live capture leaves
static int stream_store(Store &s, uint64_t n_clips, uint64_t clip_len, uint64_t chunk) {
  const uint64_t n = clip_len * kCh;
  CHECK(glc_ctx_create(0, kSr, &s.ctx));
  s.st = static_cast<hipStream_t>(glc_ctx_stream(s.ctx));
  s.n_clips = n_clips, s.clip_len = clip_len;
  s.lengths.assign(n_clips, clip_len);
  const uint64_t pushes = (clip_len + chunk - 1) / chunk;
  const glc_clip_layout whole{n_clips, kCh, 0, n, 0, clip_len, nullptr};
  s.dst_bytes = glc_compact_store_bound(&whole);
  s.arena_bytes = s.dst_bytes + n_clips * pushes * 1024;  // a segment adds its header and the padding of its sections
  float *d_pcm = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&s.d_arena, s.arena_bytes));
  HIPCHECK(hipMalloc(&s.d_cursor, 8));
  HIPCHECK(hipMalloc(&s.d_entries, n_clips * pushes * sizeof(glc_store_entry)));
  {
    const std::vector<float> base = base_signal(kSr, kCh, 10ull * kSr);
    std::vector<float> x(n);
    for (uint64_t i = 0; i < n_clips; ++i) {
      fill_clip(x, base, kCh, i, i % 4 == 3);
      HIPCHECK(hipMemcpy(d_pcm + i * n, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIPCHECK(hipMemset(s.d_cursor, 0, 8));
  glc_stream_enc *enc = nullptr;
  CHECK(glc_stream_enc_open(s.ctx, kCh, n_clips, &enc));
  std::vector<glc_stream_seg> segs(n_clips), all;
  const std::vector<uint8_t> fin(n_clips, 1);
  for (uint64_t p = 0; p < pushes; ++p) {
    const uint64_t t0 = p * chunk, len = std::min(chunk, clip_len - t0);
    const glc_clip_layout lay{n_clips, kCh, 0, n, 0, len, nullptr};
    uint64_t got = 0;
    CHECK(glc_stream_enc_push_device(enc, d_pcm + t0 * kCh, GLC_PCM_F32, 32, &lay, p + 1 == pushes ? fin.data() : nullptr, s.d_arena,
                                     s.arena_bytes, s.d_cursor, s.d_entries + all.size(), segs.data(), &got));
    all.insert(all.end(), segs.begin(), segs.begin() + got);
  }
  CHECK(glc_ctx_synchronize(s.ctx));
  glc_stream_enc_close(enc);
  HIPCHECK(hipMemcpy(&s.used, s.d_cursor, 8, hipMemcpyDeviceToHost));
  {  // the reference: the whole clips through the batch encode
    void *d_ref = nullptr;
    glc_store_entry *d_ref_entries = nullptr;
    uint64_t ref_bytes = 0;
    HIPCHECK(hipMalloc(&d_ref, s.dst_bytes));
    HIPCHECK(hipMalloc(&d_ref_entries, n_clips * sizeof(glc_store_entry)));
    HIPCHECK(hipMemset(s.d_cursor, 0, 8));
    CHECK(glc_encode_batch_device_compact(s.ctx, d_pcm, &whole, d_ref, s.dst_bytes, s.d_cursor, d_ref_entries));
    CHECK(glc_ctx_synchronize(s.ctx));
    HIPCHECK(hipMemcpy(&ref_bytes, s.d_cursor, 8, hipMemcpyDeviceToHost));
    s.ref.resize(ref_bytes), s.ref_entries.resize(n_clips);
    HIPCHECK(hipMemcpy(s.ref.data(), d_ref, ref_bytes, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(s.ref_entries.data(), d_ref_entries, n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
    (void)hipFree(d_ref), (void)hipFree(d_ref_entries);
  }
  (void)hipFree(d_pcm);
  // the pushes return their segments push by push: the join takes them clip by clip
  std::vector<glc_store_entry> ents(all.size());
  HIPCHECK(hipMemcpy(ents.data(), s.d_entries, all.size() * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  std::vector<size_t> order(all.size());
  std::iota(order.begin(), order.end(), size_t{0});
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return all[a].stream != all[b].stream ? all[a].stream < all[b].stream : all[a].first_frame < all[b].first_frame;
  });
  for (size_t j : order) {
    if (!ents[j].stored) return std::printf("a segment did not fit the arena\n"), 1;
    s.segs.push_back(all[j]), s.entries.push_back(ents[j]);
  }
  HIPCHECK(hipMemcpy(s.d_entries, s.entries.data(), s.entries.size() * sizeof(glc_store_entry), hipMemcpyHostToDevice));
  HIPCHECK(hipMalloc(&s.d_dst, s.dst_bytes));
  HIPCHECK(hipMalloc(&s.d_dst2, s.dst_bytes));
  HIPCHECK(hipMalloc(&s.d_entries_out, n_clips * sizeof(glc_store_entry)));
  HIPCHECK(hipMalloc(&s.d_entries_out2, n_clips * sizeof(glc_store_entry)));
  HIPCHECK(hipMalloc(&s.d_status, s.segs.size() * 4));
  HIPCHECK(hipMalloc(&s.d_keep, n_clips));
  HIPCHECK(hipMemset(s.d_keep, 1, n_clips));
  HIPCHECK(hipMalloc(&s.d_new_index, n_clips * 8));
  HIPCHECK(hipMalloc(&s.d_counts, 16));
  return 0;
}

static void free_store(Store &s) {
  (void)hipFree(s.d_arena), (void)hipFree(s.d_dst), (void)hipFree(s.d_dst2), (void)hipFree(s.d_entries), (void)hipFree(s.d_entries_out);
  (void)hipFree(s.d_entries_out2), (void)hipFree(s.d_status), (void)hipFree(s.d_keep), (void)hipFree(s.d_new_index), (void)hipFree(s.d_counts);
  (void)hipFree(s.d_cursor);
  glc_ctx_destroy(s.ctx);
  s = Store{};
}

static int call_join(Store &s) {
  HIPCHECK(hipMemsetAsync(s.d_cursor, 0, 8, s.st));  // every join starts the destination store afresh
  return glc_store_join_segments_device(s.ctx, s.d_arena, s.used, s.d_entries, s.segs.data(), s.segs.size(), nullptr, kCh, s.d_dst, s.dst_bytes,
                                        s.d_cursor, s.d_entries_out, nullptr, s.d_status);
}

static int call_gather(Store &s, uint64_t joined) {
  return glc_store_compact_device(s.ctx, s.d_dst, joined, s.d_entries_out, nullptr, s.n_clips, s.d_keep, s.d_dst2, s.dst_bytes, s.d_entries_out2,
                                  nullptr, s.d_new_index, s.d_counts, s.d_counts + 1);
}

// today's path, into d_dst2 / d_entries_out2; `out`, `out_entries`: what it uploads
static int call_today(Store &s, std::vector<uint8_t> &down, std::vector<glc_store_entry> &ents, std::vector<uint8_t> &out,
                      std::vector<glc_store_entry> &out_entries) {
  HIPCHECK(hipMemcpyAsync(ents.data(), s.d_entries, ents.size() * sizeof(glc_store_entry), hipMemcpyDeviceToHost, s.st));
  HIPCHECK(hipMemcpyAsync(down.data(), s.d_arena, s.used, hipMemcpyDeviceToHost, s.st));
  HIPCHECK(hipStreamSynchronize(s.st));
  uint64_t at = 0;
  std::vector<const void *> blobs;
  std::vector<uint64_t> sizes;
  for (size_t j = 0, c = 0; j < s.segs.size(); ++c) {
    blobs.clear(), sizes.clear();
    for (const uint64_t stream = s.segs[j].stream; j < s.segs.size() && s.segs[j].stream == stream; ++j)
      blobs.push_back(down.data() + ents[j].offset), sizes.push_back(ents[j].bytes);
    glc_frames *f = nullptr;
    CHECK(glc_frames_from_compact(kSr, s.clip_len * kCh, kCh, blobs.data(), sizes.data(), static_cast<uint32_t>(blobs.size()), &f));
    glc_compact_info info{};
    const int rc = glc_frames_to_compact(f, out.data() + at, out.size() - at, &info);
    glc_frames_free(f);
    if (rc != GLC_OK) return std::printf("glc_frames_to_compact failed: %s\n", glc_last_error(nullptr)), 1;
    out_entries[c] = glc_store_entry{at, info.bytes, info.n_pairs, static_cast<uint32_t>(info.n_raw_rows), 1u};
    at += info.bytes;
  }
  HIPCHECK(hipMemcpyAsync(s.d_dst2, out.data(), at, hipMemcpyHostToDevice, s.st));
  HIPCHECK(hipMemcpyAsync(s.d_entries_out2, out_entries.data(), s.n_clips * sizeof(glc_store_entry), hipMemcpyHostToDevice, s.st));
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

static int run_store(Store &s, const char *name, int reps) {
  std::vector<uint8_t> down(s.used), out(s.dst_bytes);
  std::vector<glc_store_entry> ents(s.entries.size()), today(s.n_clips), got(s.n_clips);
  // ---- the join gives the bytes and entries of the batch encode of the whole clips, before anything is timed.  (The host
  // path gives the same blobs except for the scale words of the rows of raw frames, which glc_frames_to_compact writes as
  // 0: a stream keeps no scale of a raw frame.  The count of differing bytes is printed.)
  uint64_t joined = 0, host_differs = 0;
  {
    if (call_today(s, down, ents, out, today)) return 1;
    HIPCHECK(hipStreamSynchronize(s.st));
    HIPCHECK(hipMemset(s.d_dst, 0, s.dst_bytes));
    if (call_join(s)) return std::printf("the join failed: %s\n", glc_last_error(nullptr)), 1;
    CHECK(glc_ctx_synchronize(s.ctx));
    HIPCHECK(hipMemcpy(&joined, s.d_cursor, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(got.data(), s.d_entries_out, s.n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
    std::vector<uint8_t> x(joined);
    HIPCHECK(hipMemcpy(x.data(), s.d_dst, joined, hipMemcpyDeviceToHost));
    if (joined != s.ref.size() || std::memcmp(got.data(), s.ref_entries.data(), s.n_clips * sizeof(glc_store_entry)) ||
        std::memcmp(x.data(), s.ref.data(), joined))
      return std::printf("%s: the join differs from the batch encode\n", name), 1;
    if (std::memcmp(got.data(), today.data(), s.n_clips * sizeof(glc_store_entry)))
      return std::printf("%s: the entries of the host path differ from the join's\n", name), 1;
    for (uint64_t i = 0; i < joined; ++i) host_differs += x[i] != out[i];
  }
  hipEvent_t ev0, ev1;
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  auto arm_a = [&] { return call_join(s); };
  auto arm_b = [&] { return call_gather(s, joined); };
  auto arm_c = [&] { return call_today(s, down, ents, out, today); };
  std::vector<double> h[4], d[4];
  for (int i = -std::max(2, reps / 5); i < reps; ++i) {
    const bool keep_it = i >= 0;
    if (timed(s, ev0, ev1, arm_a, keep_it ? &h[0] : nullptr, &d[0])) return 1;
    if (timed(s, ev0, ev1, arm_b, keep_it ? &h[1] : nullptr, &d[1])) return 1;
    if (keep_it && i < 3 && timed(s, ev0, ev1, arm_c, &h[2], &d[2])) return 1;  // seconds of host work: three reps
    if (timed(s, ev0, ev1, arm_a, keep_it ? &h[3] : nullptr, &d[3])) return 1;
  }
  std::printf("%s: %llu segments of %llu clips, %.1f MiB of segments joined to %.1f MiB; %d interleaved reps, 3 of (c) "
              "(ms per call: median [p10 .. p90])\n", name, (unsigned long long)s.segs.size(), (unsigned long long)s.n_clips, s.used / 1048576.0,
              joined / 1048576.0, reps);
  std::printf("  the join equals the batch encode of the whole clips; the host path differs from both in %llu bytes (scales of raw rows)\n",
              (unsigned long long)host_differs);
  const Stat a1d = stat(d[0]), a2d = stat(d[3]), a1h = stat(h[0]), a2h = stat(h[3]);
  std::printf("  A/A spread of (a): device %.4f, host %.4f\n", std::fabs(a1d.med - a2d.med), std::fabs(a1h.med - a2h.med));
  const char *names[3] = {"(a) glc_store_join_segments_device                 ", "(b) glc_store_compact_device out of place, all kept",
                          "(c) download, frames from / to compact, upload     "};
  for (int k = 0; k < 3; ++k) {
    const Stat D = stat(d[k]), H = stat(h[k]);
    std::printf("  %s device %.4f [%.4f .. %.4f]   host %.4f [%.4f .. %.4f]   %.1f GB/s joined bytes\n", names[k], D.med, D.p10, D.p90, H.med, H.p10,
                H.p90, D.med > 0 ? joined / D.med / 1e6 : 0.0);
  }
  (void)hipEventDestroy(ev0), (void)hipEventDestroy(ev1);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "trace")) {
    const uint64_t n = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 512;
    Store s;
    if (n == 0 || stream_store(s, n, 10ull * kSr, kSr / 2)) return 1;
    for (int i = 0; i < 13; ++i) {
      if (call_join(s)) return std::printf("the join failed: %s\n", glc_last_error(nullptr)), 1;
      CHECK(glc_ctx_synchronize(s.ctx));
    }
    std::printf("trace: 3 warm-up + 10 joins, %llu clips of 10 s in 20 segments each\n", (unsigned long long)n);
    free_store(s);
    return 0;
  }
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 10;
  const struct {
    const char *name;
    uint64_t clips, seconds, chunk;
  } stores[3] = {{"512 clips of 10 s in 20 segments", 512, 10, kSr / 2},
                 {"64 clips of 60 s in 100 ms segments", 64, 60, kSr / 10},
                 {"512 clips of 10 s in one segment", 512, 10, 10ull * kSr}};
  for (const auto &st : stores) {
    Store s;
    if (stream_store(s, st.clips, st.seconds * kSr, st.chunk)) return 1;
    if (run_store(s, st.name, reps)) return 1;
    free_store(s);
  }
  return 0;
}
