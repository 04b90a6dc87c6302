// store_encode_bench.cpp — what filling the compact store in one call saves: glc_encode_batch_device_compact against
// the loop a caller needs without it, for clips that are already in HBM.
//   (a) the new call: one glc_encode_batch_device_compact into an arena, one glc_ctx_synchronize
//   (b) the parent's path: per clip glc_encode_range_device + glc_compact_device_records (which synchronises: the
//       sizes come back through `info`) into a blob buffer of glc_compact_bound bytes
// Shapes: 64 clips of 2 s, 512 of 0.25 s, 4 of 60 s, all 48 kHz stereo.  Both arms on one context in one process,
// interleaved b a b' a after a warm-up; b' is the parent's path again and the difference of its two medians is the
// run's own A/A spread.  Every blob of the arena is compared with the parent's byte for byte before anything is
// timed.  The footprint line is arithmetic: the bytes the arena holds against the sum of glc_compact_bound.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_encode_bench [reps = 20]
//        build/store_encode_bench trace [clips = 64] [seconds = 2] [tonal]   3 warm-up + 10 calls of the new call and
//                                                      nothing else (for a kernel trace); `tonal`: no noise clips, the
//                                                      content of `batch_bench trace`
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

// eight partials per channel, a different cut per clip; every fourth clip uniform noise (raw frames)
static std::vector<float> signal(uint32_t sr, uint16_t ch, uint64_t per_ch, uint64_t clip, bool tonal) {
  std::vector<float> x(per_ch * ch);
  if (clip % 4 == 3 && !tonal) {
    uint32_t s = 12345u + static_cast<uint32_t>(clip);
    for (float &v : x) {
      s = 1664525u * s + 1013904223u;
      v = static_cast<float>(0.5 * (s / 2147483648.0 - 1.0));
    }
    return x;
  }
  const uint64_t period = std::min<uint64_t>(per_ch, 10ull * sr);
  for (uint16_t c = 0; c < ch; ++c)
    for (uint64_t t = 0; t < period; ++t) {
      double v = 0;
      for (int p = 0; p < 8; ++p)
        v += 0.05 * std::sin(2 * M_PI * (110.0 * (p + 1) * (1.0 + 0.37 * c) + 3.1 * p) * (t + 997 * clip) / sr + 0.5 * p);
      x[t * ch + c] = static_cast<float>(v);
    }
  for (uint64_t i = period * ch; i < x.size(); ++i) x[i] = x[i - period * ch];
  return x;
}

static const char *verdict(double a, double b, double b2, double spread) {
  return a < std::min(b, b2) - spread ? "FASTER" : a <= std::max(b, b2) + spread ? "not slower" : "SLOWER";
}

static int run(const char *name, uint64_t n_clips, uint64_t per_ch, int reps, bool trace, bool tonal = false) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = per_ch * ch;
  glc_plan plan;
  CHECK(glc_plan_encode(n, ch, &plan));
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  const uint64_t rec_bytes = plan.n_frames * glc_record_bytes(ch), bound = glc_compact_bound(ch, plan.n_frames);
  const glc_clip_layout lay{n_clips, ch, 0, n, 0, per_ch, nullptr};
  const uint64_t store_bound = glc_compact_store_bound(&lay);
  float *d_pcm = nullptr;
  void *d_rec = nullptr, *d_blob = nullptr, *d_arena = nullptr;
  uint64_t *d_cursor = nullptr;
  glc_store_entry *d_entries = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&d_rec, rec_bytes));
  HIPCHECK(hipMalloc(&d_blob, bound));
  HIPCHECK(hipMalloc(&d_arena, store_bound));
  HIPCHECK(hipMalloc(&d_cursor, sizeof(uint64_t)));
  HIPCHECK(hipMalloc(&d_entries, n_clips * sizeof(glc_store_entry)));
  for (uint64_t i = 0; i < n_clips; ++i) {
    const std::vector<float> x = signal(sr, ch, per_ch, i, tonal);
    HIPCHECK(hipMemcpy(d_pcm + i * n, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
  }
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  auto arm_new = [&] {
    if (hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st) != hipSuccess) return 1;  // every call fills the arena from its start
    const int rc = glc_encode_batch_device_compact(ctx, d_pcm, &lay, d_arena, store_bound, d_cursor, d_entries);
    return rc ? rc : glc_ctx_synchronize(ctx);
  };
  if (trace) {
    for (int i = 0; i < 13; ++i) CHECK(arm_new());
    std::printf("trace: 3 warm-up + 10 calls, %llu clip(s) x %llu frames x %u ch\n", (unsigned long long)n_clips,
                (unsigned long long)plan.n_frames, ch);
    return 0;
  }
  glc_compact_info info{};
  auto arm_parent = [&] {
    for (uint64_t i = 0; i < n_clips; ++i) {
      int rc = glc_encode_range_device(ctx, d_pcm + i * n, 0, per_ch, n, ch, 0, plan.n_frames, d_rec, nullptr);
      if (!rc) rc = glc_compact_device_records(ctx, d_rec, plan.n_frames, ch, d_blob, bound, &info);
      if (rc) return rc;
    }
    return 0;
  };
  // the same bytes, before anything is timed
  CHECK(arm_new());
  std::vector<glc_store_entry> entries(n_clips);
  HIPCHECK(hipMemcpy(entries.data(), d_entries, n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  uint64_t cursor = 0, held = 0;
  HIPCHECK(hipMemcpy(&cursor, d_cursor, sizeof cursor, hipMemcpyDeviceToHost));
  std::vector<uint8_t> want(bound), have(bound);
  for (uint64_t i = 0; i < n_clips; ++i) {
    CHECK(glc_encode_range_device(ctx, d_pcm + i * n, 0, per_ch, n, ch, 0, plan.n_frames, d_rec, nullptr));
    CHECK(glc_compact_device_records(ctx, d_rec, plan.n_frames, ch, d_blob, bound, &info));
    const glc_store_entry &e = entries[i];
    if (!e.stored || e.bytes != info.bytes || e.n_pairs != info.n_pairs || e.n_raw_rows != info.n_raw_rows || e.offset != held)
      return std::printf("%s: the entry of clip %llu differs from the parent's sizes\n", name, (unsigned long long)i), 1;
    HIPCHECK(hipMemcpy(want.data(), d_blob, info.bytes, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(have.data(), static_cast<const uint8_t *>(d_arena) + e.offset, e.bytes, hipMemcpyDeviceToHost));
    if (std::memcmp(want.data(), have.data(), info.bytes))
      return std::printf("%s: the blob of clip %llu differs from the parent's\n", name, (unsigned long long)i), 1;
    held += e.bytes;
  }
  if (cursor != held) return std::printf("%s: the cursor is not the sum of the sizes\n", name), 1;

  auto timed = [&](auto &&fn, std::vector<double> &into) {
    const double t0 = now_ms();
    const int rc = fn();
    into.push_back(now_ms() - t0);
    return rc;
  };
  const int warm = std::max(3, reps / 5);
  for (int i = 0; i < warm; ++i) { CHECK(arm_parent()); CHECK(arm_new()); }
  std::vector<double> tb, tb2, ta;
  for (int i = 0; i < reps; ++i) {
    CHECK(timed(arm_parent, tb)); CHECK(timed(arm_new, ta)); CHECK(timed(arm_parent, tb2)); CHECK(timed(arm_new, ta));
  }
  const Stat A = stat(ta), B = stat(tb), B2 = stat(tb2);
  const double spread = std::fabs(B.med - B2.med);
  std::printf("%s: %llu clip(s) x %llu frames x %u ch at %u Hz; %d interleaved reps (ms per call: median [p10 .. p90])\n", name,
              (unsigned long long)n_clips, (unsigned long long)plan.n_frames, ch, sr, reps);
  std::printf("  (b) loop of glc_encode_range_device + glc_compact_device_records   %.4f [%.4f .. %.4f]   again %.4f   A/A spread %.4f\n",
              B.med, B.p10, B.p90, B2.med, spread);
  std::printf("  (a) glc_encode_batch_device_compact + glc_ctx_synchronize          %.4f [%.4f .. %.4f]   new - parent %+.4f   parent / new %.2f  -> %s\n",
              A.med, A.p10, A.p90, A.med - std::min(B.med, B2.med), std::min(B.med, B2.med) / A.med, verdict(A.med, B.med, B2.med, spread));
  std::printf("  footprint: the arena holds %llu bytes; blob buffers of glc_compact_bound each hold %llu (%.2f x); records %llu\n",
              (unsigned long long)held, (unsigned long long)store_bound, double(store_bound) / double(held),
              (unsigned long long)(rec_bytes * n_clips));
  (void)hipFree(d_pcm), (void)hipFree(d_rec), (void)hipFree(d_blob), (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "trace"))
    return run("trace", argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 64, static_cast<uint64_t>((argc > 3 ? std::atof(argv[3]) : 2.0) * 48000), 0,
               true, argc > 4 && !std::strcmp(argv[4], "tonal"));
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 20;
  if (run("64 clips of 2 s", 64, 2ull * 48000, reps, false)) return 1;
  if (run("512 clips of 0.25 s", 512, 12000, reps, false)) return 1;
  if (run("4 clips of 60 s", 4, 60ull * 48000, reps, false)) return 1;
  return 0;
}
