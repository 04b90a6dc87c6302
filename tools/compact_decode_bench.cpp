// compact_decode_bench.cpp — what decoding a compact blob where it lies saves: glc_decode_device_compact /
// glc_decode_batch_device_compact against what a caller needs without them for a blob that is already in HBM,
// and against the decode of the same stream's (8.9 x larger) frame records.
//   (a) the new call
//   (b) the parent's path: copy the blob to the host, glc_frames_from_compact, glc_decode_device of a stream the
//       context has not seen (per clip, for the batch)
//   (c) glc_decode_device_records of the same stream's records (a loop over the clips, for the batch)
// Shapes: BASELINE config 2 (48 kHz stereo, 4096 frames), and 64 clips of 2 s.  All arms end in
// glc_ctx_synchronize.  Interleaved b a b' a c after a warm-up; b' is the parent's path again and the difference
// of its two medians is the run's own A/A spread.  Every arm's samples are compared bit for bit before anything
// is timed.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/compact_decode_bench [reps = 20]
//        build/compact_decode_bench trace single|batch [clips = 64]   3 warm-up + 10 calls of the new call and nothing
//                                                                     else (for a kernel + memory-copy trace)
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
static std::vector<float> signal(uint32_t sr, uint16_t ch, uint64_t per_ch, uint64_t clip) {
  std::vector<float> x(per_ch * ch);
  if (clip % 4 == 3) {
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

static const char *verdict(double b, double a, double a2, double spread) {
  return b < std::min(a, a2) - spread ? "FASTER" : b <= std::max(a, a2) + spread ? "not slower" : "SLOWER";
}

static int run(const char *name, uint64_t n_clips, uint64_t per_ch, int reps, bool trace) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = per_ch * ch;
  glc_plan plan;
  CHECK(glc_plan_encode(n, ch, &plan));
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  const uint64_t rec_bytes = plan.n_frames * glc_record_bytes(ch), bound = glc_compact_bound(ch, plan.n_frames);
  const uint64_t cap_all = (plan.n_frames + 1) * 1024ull * ch;
  float *d_pcm = nullptr, *d_out = nullptr, *d_all = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, n * sizeof(float)));
  HIPCHECK(hipMalloc(&d_out, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&d_all, cap_all * sizeof(float)));
  std::vector<void *> d_rec(n_clips), d_blob(n_clips);
  std::vector<const void *> blobs(n_clips);
  std::vector<uint64_t> blob_bytes(n_clips), n_samples(n_clips, n);
  uint64_t total_blob = 0;
  for (uint64_t i = 0; i < n_clips; ++i) {  // the store: every clip's records (for arm c) and its blob, trimmed to its bytes
    const std::vector<float> x = signal(sr, ch, per_ch, i);
    HIPCHECK(hipMemcpy(d_pcm, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(hipMalloc(&d_rec[i], rec_bytes));
    void *tmp = nullptr;
    HIPCHECK(hipMalloc(&tmp, bound));
    CHECK(glc_encode_range_device(ctx, d_pcm, 0, per_ch, n, ch, 0, plan.n_frames, d_rec[i], nullptr));
    glc_compact_info info;
    CHECK(glc_compact_device_records(ctx, d_rec[i], plan.n_frames, ch, tmp, bound, &info));
    HIPCHECK(hipMalloc(&d_blob[i], info.bytes));
    HIPCHECK(hipMemcpy(d_blob[i], tmp, info.bytes, hipMemcpyDeviceToDevice));
    (void)hipFree(tmp);
    blobs[i] = d_blob[i], blob_bytes[i] = info.bytes, total_blob += info.bytes;
  }
  const glc_clip_layout lay{n_clips, ch, 0, n, 0, per_ch, nullptr};
  uint64_t got = 0, start = 0;
  auto arm_new = [&] {
    const int rc = n_clips == 1 ? glc_decode_device_compact(ctx, blobs[0], blob_bytes[0], n, ch, d_out, n, &got)
                                : glc_decode_batch_device_compact(ctx, blobs.data(), blob_bytes.data(), n_samples.data(), d_out, &lay);
    return rc ? rc : glc_ctx_synchronize(ctx);
  };
  if (trace) {
    for (int i = 0; i < 13; ++i) CHECK(arm_new());
    std::printf("trace (%s): 3 warm-up + 10 calls, %llu clip(s) x %llu frames x %u ch\n", name, (unsigned long long)n_clips,
                (unsigned long long)plan.n_frames, ch);
    return 0;
  }
  std::vector<uint64_t> host(*std::max_element(blob_bytes.begin(), blob_bytes.end()) / 8 + 1);
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  auto arm_parent = [&] {  // per clip: the blob comes down, a stream is assembled, its rows go up, it is decoded
    for (uint64_t i = 0; i < n_clips; ++i) {
      if (hipMemcpy(host.data(), d_blob[i], blob_bytes[i], hipMemcpyDeviceToHost) != hipSuccess) return 1;
      const void *p[1] = {host.data()};
      glc_frames *F = nullptr;
      int rc = glc_frames_from_compact(sr, n, ch, p, &blob_bytes[i], 1, &F);
      if (!rc) rc = glc_decode_device(ctx, F, d_all, cap_all, &start, &got);
      if (!rc && hipMemcpyAsync(d_out + i * n, d_all + start, got * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = 1;
      if (!rc) rc = glc_ctx_synchronize(ctx);  // F's rows are in flight until here
      glc_frames_free(F);
      if (rc) return rc;
    }
    return 0;
  };
  auto arm_records = [&] {
    for (uint64_t i = 0; i < n_clips; ++i)
      if (const int rc = glc_decode_device_records(ctx, d_rec[i], plan.n_frames, n, ch, d_out + i * n, n, &got)) return rc;
    return glc_ctx_synchronize(ctx);
  };
  // the same bits, before anything is timed
  std::vector<float> ya(n_clips * n), yb(n_clips * n);
  CHECK(arm_parent());
  HIPCHECK(hipMemcpy(ya.data(), d_out, ya.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemset(d_out, 0xFF, ya.size() * sizeof(float)));
  CHECK(arm_new());
  HIPCHECK(hipMemcpy(yb.data(), d_out, yb.size() * sizeof(float), hipMemcpyDeviceToHost));
  if (std::memcmp(ya.data(), yb.data(), ya.size() * sizeof(float))) return std::printf("%s: the compact decode differs from the parent's path\n", name), 1;
  std::vector<glc_compact_status> status(n_clips);
  CHECK(glc_decode_compact_last_status(ctx, status.data(), n_clips));
  for (const glc_compact_status &s : status)
    if (s.flags || s.n_bad_rows) return std::printf("%s: the device check refused part of an encoder's blob\n", name), 1;
  CHECK(arm_records());
  HIPCHECK(hipMemcpy(yb.data(), d_out, yb.size() * sizeof(float), hipMemcpyDeviceToHost));
  if (std::memcmp(ya.data(), yb.data(), ya.size() * sizeof(float))) return std::printf("%s: the records decode differs from the parent's path\n", name), 1;

  auto timed = [&](auto &&fn, std::vector<double> &into) {
    const double t0 = now_ms();
    const int rc = fn();
    into.push_back(now_ms() - t0);
    return rc;
  };
  const int warm = std::max(3, reps / 5);
  for (int i = 0; i < warm; ++i) { CHECK(arm_parent()); CHECK(arm_new()); CHECK(arm_records()); }
  std::vector<double> tb, tb2, ta, tc;
  for (int i = 0; i < reps; ++i) {
    CHECK(timed(arm_parent, tb)); CHECK(timed(arm_new, ta)); CHECK(timed(arm_parent, tb2)); CHECK(timed(arm_new, ta)); CHECK(timed(arm_records, tc));
  }
  const Stat A = stat(ta), B = stat(tb), B2 = stat(tb2), Cs = stat(tc);
  const double spread = std::fabs(B.med - B2.med);
  std::printf("%s: %llu clip(s) x %llu frames x %u ch at %u Hz; blobs %llu bytes, records %llu bytes; %d interleaved reps "
              "(ms per call: median [p10 .. p90])\n", name, (unsigned long long)n_clips, (unsigned long long)plan.n_frames, ch, sr,
              (unsigned long long)total_blob, (unsigned long long)(rec_bytes * n_clips), reps);
  std::printf("  (b) blob to host + glc_frames_from_compact + glc_decode_device   %.4f [%.4f .. %.4f]   again %.4f   A/A spread %.4f\n",
              B.med, B.p10, B.p90, B2.med, spread);
  std::printf("  (a) %-61s %.4f [%.4f .. %.4f]   new - parent %+.4f   parent / new %.2f  -> %s\n",
              n_clips == 1 ? "glc_decode_device_compact" : "glc_decode_batch_device_compact", A.med, A.p10, A.p90,
              A.med - std::min(B.med, B2.med), std::min(B.med, B2.med) / A.med, verdict(A.med, B.med, B2.med, spread));
  std::printf("  (c) glc_decode_device_records of the same stream's records       %.4f [%.4f .. %.4f]   (a) - (c) %+.4f\n", Cs.med, Cs.p10,
              Cs.p90, A.med - Cs.med);
  for (uint64_t i = 0; i < n_clips; ++i) (void)hipFree(d_rec[i]), (void)hipFree(d_blob[i]);
  (void)hipFree(d_pcm), (void)hipFree(d_out), (void)hipFree(d_all);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 2 && !std::strcmp(argv[1], "trace")) {
    if (!std::strcmp(argv[2], "single")) return run("single", 1, 4096ull * 1024, 0, true);
    return run("batch", argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 64, 2ull * 48000, 0, true);
  }
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 20;
  if (run("config 2 (4096 frames)", 1, 4096ull * 1024, reps, false)) return 1;
  if (run("64 clips of 2 s", 64, 2ull * 48000, reps, false)) return 1;
  return 0;
}
