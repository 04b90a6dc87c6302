// store_compact_bench.cpp — what evicting clips from the compact store costs: glc_store_compact_device against what a caller
// does without it, for a store the encoder has just filled.
//   (a) the new call in place (the arena is restored from a pristine copy before every call, outside the timing)
//   (b) the new call out of place, into a second arena
//   (c) today's path: the entries downloaded and the stream synchronised, the plan made on the host, one
//       hipMemcpyAsync device-to-device per kept blob into a second arena, the new entries uploaded
//   (d) ONE hipMemcpyAsync device-to-device of as many bytes as the kept blobs hold: the bandwidth yardstick
// Per call and arm: the device time (two events on the context's stream around the call), the host wall time INSIDE the
// call, and the kept bytes per second of device time.  All arms in one process, interleaved c a b d c' after a warm-up;
// c' is today's path again and the difference of its two medians is the run's own A/A spread.  The arenas and entries
// of (a) and (b) are compared with those of (c) before anything is timed.  arena_bytes is the store's cursor - the
// bound on the bytes in use a caller has who read it once.
// Stores, 48 kHz stereo: 512 clips of 10 s, 64 clips of 60 s.  Keep patterns: every other clip, the last three quarters,
// all, none.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_compact_bench [reps = 10]
//        build/store_compact_bench rounds [reps = 10]     (a) at in-place rounds of 2 .. 256 MiB, 512 clips of 10 s, every other
//        build/store_compact_bench trace [entries = 512]  3 warm-up + 10 in-place calls and nothing else (for a kernel and
//                                                         memory-copy trace): a host-made store of 256 MiB, every other kept
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glc.h"
#include "glc_debug.h"

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

// the signal of store_draw_bench: eight partials per channel, clip i a cut at its own offset, every fourth clip noise
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

struct Store {
  glc_ctx *ctx = nullptr;
  hipStream_t st = nullptr;
  uint64_t n = 0, bytes = 0;           // entries; the cursor: bytes in use
  void *d_pristine = nullptr, *d_work = nullptr, *d_dst = nullptr;
  glc_store_entry *d_entries = nullptr, *d_entries_out = nullptr;
  uint8_t *d_keep = nullptr;
  int64_t *d_new_index = nullptr;
  uint64_t *d_counts = nullptr;
  std::vector<glc_store_entry> entries;
};

static int make_buffers(Store &s) {
  HIPCHECK(hipMalloc(&s.d_work, std::max<uint64_t>(s.bytes, 64)));
  HIPCHECK(hipMalloc(&s.d_dst, std::max<uint64_t>(s.bytes, 64)));
  HIPCHECK(hipMalloc(&s.d_entries_out, s.n * sizeof(glc_store_entry)));
  HIPCHECK(hipMalloc(&s.d_keep, s.n));
  HIPCHECK(hipMalloc(&s.d_new_index, s.n * 8));
  HIPCHECK(hipMalloc(&s.d_counts, 16));
  return 0;
}

static int encode_store(Store &s, uint64_t n_clips, uint64_t clip_len) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = clip_len * ch;
  CHECK(glc_ctx_create(0, sr, &s.ctx));
  s.st = static_cast<hipStream_t>(glc_ctx_stream(s.ctx));
  s.n = n_clips;
  const glc_clip_layout in_lay{n_clips, ch, 0, n, 0, clip_len, nullptr};
  const uint64_t bound = glc_compact_store_bound(&in_lay);
  float *d_pcm = nullptr;
  uint64_t *d_cursor = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&s.d_pristine, bound));
  HIPCHECK(hipMalloc(&d_cursor, 8));
  HIPCHECK(hipMalloc(&s.d_entries, n_clips * sizeof(glc_store_entry)));
  {
    const std::vector<float> base = base_signal(sr, ch, 10ull * sr);
    std::vector<float> x(n);
    for (uint64_t i = 0; i < n_clips; ++i) {
      fill_clip(x, base, ch, i, i % 4 == 3);
      HIPCHECK(hipMemcpy(d_pcm + i * n, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIPCHECK(hipMemset(d_cursor, 0, 8));
  CHECK(glc_encode_batch_device_compact(s.ctx, d_pcm, &in_lay, s.d_pristine, bound, d_cursor, s.d_entries));
  CHECK(glc_ctx_synchronize(s.ctx));
  HIPCHECK(hipMemcpy(&s.bytes, d_cursor, 8, hipMemcpyDeviceToHost));
  (void)hipFree(d_pcm), (void)hipFree(d_cursor);
  s.entries.resize(n_clips);
  HIPCHECK(hipMemcpy(s.entries.data(), s.d_entries, n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  for (const glc_store_entry &e : s.entries)
    if (!e.stored) return std::printf("a clip did not fit the arena\n"), 1;
  return make_buffers(s);
}

// a store nobody encoded: n equal blobs of arbitrary bytes in `bytes` bytes (the mover does not look into a blob)
static int host_store(Store &s, uint64_t n, uint64_t bytes) {
  CHECK(glc_ctx_create(0, 48000, &s.ctx));
  s.st = static_cast<hipStream_t>(glc_ctx_stream(s.ctx));
  s.n = n, s.bytes = bytes;
  const uint64_t each = bytes / n / 64 * 64;
  s.entries.resize(n);
  for (uint64_t i = 0; i < n; ++i) s.entries[i] = glc_store_entry{i * each, each, 0, 0, 1};
  HIPCHECK(hipMalloc(&s.d_pristine, bytes));
  HIPCHECK(hipMemset(s.d_pristine, 0x5A, bytes));
  HIPCHECK(hipMalloc(&s.d_entries, n * sizeof(glc_store_entry)));
  HIPCHECK(hipMemcpy(s.d_entries, s.entries.data(), n * sizeof(glc_store_entry), hipMemcpyHostToDevice));
  return make_buffers(s);
}

static void free_store(Store &s) {
  (void)hipFree(s.d_pristine), (void)hipFree(s.d_work), (void)hipFree(s.d_dst), (void)hipFree(s.d_entries), (void)hipFree(s.d_entries_out);
  (void)hipFree(s.d_keep), (void)hipFree(s.d_new_index), (void)hipFree(s.d_counts);
  glc_ctx_destroy(s.ctx);
  s = Store{};
}

static int call_new(Store &s, bool in_place) {
  void *src = in_place ? s.d_work : s.d_pristine, *dst = in_place ? s.d_work : s.d_dst;
  return glc_store_compact_device(s.ctx, src, s.bytes, s.d_entries, nullptr, s.n, s.d_keep, dst, s.bytes, s.d_entries_out, nullptr,
                                  s.d_new_index, s.d_counts, s.d_counts + 1);
}

// today's path; `out` receives the entries it uploads
static int call_today(Store &s, std::vector<glc_store_entry> &down, std::vector<uint8_t> &keep, std::vector<glc_store_entry> &out) {
  HIPCHECK(hipMemcpyAsync(down.data(), s.d_entries, s.n * sizeof(glc_store_entry), hipMemcpyDeviceToHost, s.st));
  HIPCHECK(hipMemcpyAsync(keep.data(), s.d_keep, s.n, hipMemcpyDeviceToHost, s.st));
  HIPCHECK(hipStreamSynchronize(s.st));
  uint64_t at = 0, k = 0;
  std::fill(out.begin(), out.end(), glc_store_entry{});
  for (uint64_t i = 0; i < s.n; ++i) {
    if (!keep[i] || !down[i].stored) continue;
    HIPCHECK(hipMemcpyAsync(static_cast<uint8_t *>(s.d_dst) + at, static_cast<const uint8_t *>(s.d_pristine) + down[i].offset, down[i].bytes,
                            hipMemcpyDeviceToDevice, s.st));
    out[k] = down[i];
    out[k++].offset = at;
    at += down[i].bytes;
  }
  HIPCHECK(hipMemcpyAsync(s.d_entries_out, out.data(), s.n * sizeof(glc_store_entry), hipMemcpyHostToDevice, s.st));
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

static int restore(Store &s) {  // the arena of the in-place arm as the encoder left it; not timed
  HIPCHECK(hipMemcpyAsync(s.d_work, s.d_pristine, s.bytes, hipMemcpyDeviceToDevice, s.st));
  HIPCHECK(hipStreamSynchronize(s.st));
  return 0;
}

static int run_pattern(Store &s, const char *store_name, const char *pat_name, const std::vector<uint8_t> &keep_h, int reps) {
  HIPCHECK(hipMemcpy(s.d_keep, keep_h.data(), s.n, hipMemcpyHostToDevice));
  uint64_t moved = 0, kept = 0;
  for (uint64_t i = 0; i < s.n; ++i)
    if (keep_h[i]) moved += s.entries[i].bytes, ++kept;
  std::vector<glc_store_entry> down(s.n), out(s.n), got(s.n);
  std::vector<uint8_t> keep(s.n);
  // ---- the same bytes and entries from all three, before anything is timed
  {
    std::vector<uint8_t> ref(moved), x(moved);
    if (call_today(s, down, keep, out)) return 1;
    HIPCHECK(hipStreamSynchronize(s.st));
    HIPCHECK(hipMemcpy(ref.data(), s.d_dst, moved, hipMemcpyDeviceToHost));
    for (int in_place = 0; in_place < 2; ++in_place) {
      if (restore(s)) return 1;
      HIPCHECK(hipMemset(s.d_dst, 0, std::max<uint64_t>(s.bytes, 64)));
      CHECK(call_new(s, in_place != 0));
      CHECK(glc_ctx_synchronize(s.ctx));
      uint64_t counts[2];
      HIPCHECK(hipMemcpy(counts, s.d_counts, 16, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(got.data(), s.d_entries_out, s.n * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(x.data(), in_place ? s.d_work : s.d_dst, moved, hipMemcpyDeviceToHost));
      if (counts[0] != kept || counts[1] != moved || std::memcmp(got.data(), out.data(), s.n * sizeof(glc_store_entry)) ||
          std::memcmp(x.data(), ref.data(), moved))
        return std::printf("%s, %s: the %s call differs from the host path\n", store_name, pat_name, in_place ? "in-place" : "out-of-place"), 1;
    }
  }
  hipEvent_t ev0, ev1;
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  auto arm_a = [&] { return call_new(s, true); };
  auto arm_b = [&] { return call_new(s, false); };
  auto arm_c = [&] { return call_today(s, down, keep, out); };
  auto arm_d = [&] {
    return moved && hipMemcpyAsync(s.d_dst, s.d_pristine, moved, hipMemcpyDeviceToDevice, s.st) != hipSuccess ? 1 : 0;
  };
  std::vector<double> h[5], d[5];
  for (int i = -std::max(2, reps / 5); i < reps; ++i) {
    const bool keep_it = i >= 0;
    if (timed(s, ev0, ev1, arm_c, keep_it ? &h[2] : nullptr, &d[2])) return 1;
    if (restore(s)) return 1;
    if (timed(s, ev0, ev1, arm_a, keep_it ? &h[0] : nullptr, &d[0])) return 1;
    if (timed(s, ev0, ev1, arm_b, keep_it ? &h[1] : nullptr, &d[1])) return 1;
    if (timed(s, ev0, ev1, arm_d, keep_it ? &h[3] : nullptr, &d[3])) return 1;
    if (timed(s, ev0, ev1, arm_c, keep_it ? &h[4] : nullptr, &d[4])) return 1;
  }
  std::printf("%s, keep %s: %llu of %llu entries kept, %.1f of %.1f MiB; %d interleaved reps (ms per call: median [p10 .. p90])\n", store_name,
              pat_name, (unsigned long long)kept, (unsigned long long)s.n, moved / 1048576.0, s.bytes / 1048576.0, reps);
  const char *names[4] = {"(a) glc_store_compact_device in place              ", "(b) glc_store_compact_device out of place          ",
                          "(c) download, host plan, one copy per blob, upload ", "(d) one device-to-device copy of the kept bytes    "};
  const Stat c1d = stat(d[2]), c2d = stat(d[4]), c1h = stat(h[2]), c2h = stat(h[4]);
  std::printf("  A/A spread of (c): device %.4f, host %.4f\n", std::fabs(c1d.med - c2d.med), std::fabs(c1h.med - c2h.med));
  for (int k = 0; k < 4; ++k) {
    const Stat D = stat(d[k]), H = stat(h[k]);
    std::printf("  %s device %.4f [%.4f .. %.4f]   host %.4f [%.4f .. %.4f]   %.1f GB/s kept bytes\n", names[k], D.med, D.p10, D.p90, H.med, H.p10,
                H.p90, D.med > 0 ? moved / D.med / 1e6 : 0.0);
  }
  (void)hipEventDestroy(ev0), (void)hipEventDestroy(ev1);
  return 0;
}

static std::vector<uint8_t> pattern(int which, uint64_t n) {
  std::vector<uint8_t> k(n);
  for (uint64_t i = 0; i < n; ++i) k[i] = which == 0 ? i % 2 : which == 1 ? i >= n / 4 : which == 2 ? 1 : 0;
  return k;
}

int main(int argc, char **argv) {
  const uint64_t sr = 48000;
  if (argc > 1 && !std::strcmp(argv[1], "trace")) {
    const uint64_t n = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 512;
    Store s;
    if (n == 0 || host_store(s, n, 256ull << 20)) return 1;
    const std::vector<uint8_t> keep = pattern(0, n);
    HIPCHECK(hipMemcpy(s.d_keep, keep.data(), n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(s.d_work, s.d_pristine, s.bytes, hipMemcpyDeviceToDevice));
    HIPCHECK(hipDeviceSynchronize());
    for (int i = 0; i < 13; ++i) {
      CHECK(call_new(s, true));
      CHECK(glc_ctx_synchronize(s.ctx));
    }
    std::printf("trace: 3 warm-up + 10 in-place calls, %llu entries in an arena of 256 MiB, every other kept\n", (unsigned long long)n);
    free_store(s);
    return 0;
  }
  if (argc > 1 && !std::strcmp(argv[1], "rounds")) {
    const int reps = argc > 2 ? std::max(5, std::atoi(argv[2])) : 10;
    Store s;
    if (encode_store(s, 512, 10 * sr)) return 1;
    const std::vector<uint8_t> keep = pattern(0, s.n);
    HIPCHECK(hipMemcpy(s.d_keep, keep.data(), s.n, hipMemcpyHostToDevice));
    uint64_t moved = 0;
    for (uint64_t i = 0; i < s.n; ++i)
      if (keep[i]) moved += s.entries[i].bytes;
    hipEvent_t ev0, ev1;
    HIPCHECK(hipEventCreate(&ev0));
    HIPCHECK(hipEventCreate(&ev1));
    std::printf("in-place rounds, 512 clips of 10 s, every other kept: %.1f of %.1f MiB; %d reps per round size, two passes "
                "(ms per call: median [p10 .. p90])\n", moved / 1048576.0, s.bytes / 1048576.0, reps);
    for (int pass = 0; pass < 2; ++pass)
      for (uint64_t mib = 2; mib <= 256; mib *= 2) {
        CHECK(glc_debug_set_store_compact_round(s.ctx, mib << 20));
        std::vector<double> h, d;
        for (int i = -2; i < reps; ++i) {
          if (restore(s)) return 1;
          if (timed(s, ev0, ev1, [&] { return call_new(s, true); }, i >= 0 ? &h : nullptr, &d)) return 1;
        }
        const Stat D = stat(d), H = stat(h);
        std::printf("  pass %d  round %3llu MiB  staging %3llu MiB  launches %3llu  device %.4f [%.4f .. %.4f]  host %.4f [%.4f .. %.4f]  %.1f GB/s\n",
                    pass, (unsigned long long)mib, (unsigned long long)(2 * std::min<uint64_t>(mib << 20, s.bytes) >> 20),
                    (unsigned long long)((s.bytes + (mib << 20) - 1) / (mib << 20) + 3), D.med, D.p10, D.p90, H.med, H.p10, H.p90,
                    moved / D.med / 1e6);
      }
    free_store(s);
    return 0;
  }
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 10;
  const char *pats[4] = {"every other", "the last three quarters", "all", "none"};
  const struct {
    const char *name;
    uint64_t clips, seconds;
  } stores[2] = {{"512 clips of 10 s", 512, 10}, {"64 clips of 60 s", 64, 60}};
  for (const auto &st : stores) {
    Store s;
    if (encode_store(s, st.clips, st.seconds * sr)) return 1;
    for (int p = 0; p < 4; ++p)
      if (run_pattern(s, st.name, pats[p], pattern(p, s.n), reps)) return 1;
    free_store(s);
  }
  return 0;
}
