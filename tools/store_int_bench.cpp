// store_int_bench.cpp — what integer PCM on the device batch and store paths costs and saves.
// Encode legs (the workloads of store_encode_bench: 64 stereo clips of 2 s, 512 of 0.25 s), int16 clips in HBM:
//   (a) the calls a caller had: glc_pcm_widen_device into a float scratch batch twice the size, then
//       glc_encode_batch_device_compact of that
//   (b) glc_encode_batch_device_compact_int: the gather widens
// Draw legs (the workloads of store_draw_bench: 512 crops of 0.25 s from 512 clips of 10 s, 64 crops of 1 s from 64 clips
// of 60 s):
//   (a) glc_decode_crops_device_store (float crops)
//   (b) glc_decode_crops_device_store_i16 (half the bytes written)
// Per call and arm: the device time (two events on the context's stream around the call) and the host wall time INSIDE
// the call.  Both arms on one context in one process, interleaved a b a' b after a warm-up; a' is arm (a) again and the
// difference of its two medians is the run's own A/A spread.  Before anything is timed the two arenas are compared
// byte for byte (encode) and the int16 crops with the narrowed float crops (draw).
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_int_bench [reps = 20]
//        build/store_int_bench trace [clips = 64]   3 warm-up + 10 calls of each of the two new calls and nothing else (for a
//                                                   kernel and memory-copy trace): `clips` stereo int16 clips of 0.25 s into
//                                                   the store, then as many int16 crops of 0.125 s drawn from it
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

// the base signal of store_draw_bench: eight partials per channel over a period of 10 s; clip i is a cut of it at its
// own offset, every fourth clip uniform noise (raw frames)
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
// the 16-bit file a user would have
static void quantise(const std::vector<float> &x, std::vector<int16_t> &q) {
  q.resize(x.size());
  for (size_t i = 0; i < x.size(); ++i) q[i] = static_cast<int16_t>(std::max(-32768.0, std::min(32767.0, std::nearbyint(x[i] * 32767.0))));
}
// convert_f32_to_i16 of the reference (src/audio.rs:11-16)
static int16_t narrow(float s) {
  const float v = s * 32767.0f;
  if (v != v) return 0;
  return static_cast<int16_t>(std::max(-32768.0f, std::min(32767.0f, v)));
}

static const char *verdict(double b, double a, double a2, double spread) {
  return b < std::min(a, a2) - spread ? "FASTER" : b <= std::max(a, a2) + spread ? "not slower" : "SLOWER";
}

struct Timer {
  hipStream_t st;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int init(hipStream_t s) {
    st = s;
    return hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess;
  }
  template <typename F>
  int operator()(F &&fn, std::vector<double> *host, std::vector<double> *dev) {
    if (hipEventRecord(ev0, st) != hipSuccess) return 1;
    const double t0 = now_ms();
    const int rc = fn();
    const double t1 = now_ms();
    if (rc) return rc;
    if (hipEventRecord(ev1, st) != hipSuccess || hipEventSynchronize(ev1) != hipSuccess) return 1;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return 1;
    if (host) host->push_back(t1 - t0), dev->push_back(ms);
    return 0;
  }
  ~Timer() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

template <typename FA, typename FB>
static int race(Timer &timed, FA &&arm_a, FB &&arm_b, int reps, const char *name_a, const char *name_b) {
  const int warm = std::max(3, reps / 5);
  for (int i = 0; i < warm; ++i) {
    if (timed(arm_a, nullptr, nullptr) || timed(arm_b, nullptr, nullptr)) return 1;
  }
  std::vector<double> ha, ha2, hb, da, da2, db;
  for (int i = 0; i < reps; ++i) {
    if (timed(arm_a, &ha, &da) || timed(arm_b, &hb, &db) || timed(arm_a, &ha2, &da2) || timed(arm_b, &hb, &db)) return 1;
  }
  const char *what[2] = {"device time (events around the call)", "host wall time inside the call     "};
  std::vector<double> *ta[2] = {&da, &ha}, *ta2[2] = {&da2, &ha2}, *tb[2] = {&db, &hb};
  for (int k = 0; k < 2; ++k) {
    const Stat A = stat(*ta[k]), A2 = stat(*ta2[k]), B = stat(*tb[k]);
    const double spread = std::fabs(A.med - A2.med);
    std::printf("  %s\n", what[k]);
    std::printf("    (a) %s   %.4f [%.4f .. %.4f]   again %.4f   A/A spread %.4f\n", name_a, A.med, A.p10, A.p90, A2.med, spread);
    std::printf("    (b) %s   %.4f [%.4f .. %.4f]   b - a %+.4f   a / b %.2f  -> %s\n", name_b, B.med, B.p10, B.p90,
                B.med - std::min(A.med, A2.med), std::min(A.med, A2.med) / B.med, verdict(B.med, A.med, A2.med, spread));
  }
  return 0;
}

// ---- encode: n_clips int16 stereo clips of per_ch samples per channel
static int run_encode(const char *name, uint64_t n_clips, uint64_t per_ch, int reps) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = per_ch * ch;
  glc_plan plan;
  CHECK(glc_plan_encode(n, ch, &plan));
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  const glc_clip_layout lay{n_clips, ch, 0, n, 0, per_ch, nullptr};
  const uint64_t store_bound = glc_compact_store_bound(&lay);
  int16_t *d_int = nullptr;
  float *d_scratch = nullptr;
  void *d_arena[2] = {nullptr, nullptr};
  uint64_t *d_cursor = nullptr;
  glc_store_entry *d_entries[2] = {nullptr, nullptr};
  HIPCHECK(hipMalloc(&d_int, n_clips * n * sizeof(int16_t)));
  HIPCHECK(hipMalloc(&d_scratch, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&d_cursor, sizeof(uint64_t)));
  for (int k = 0; k < 2; ++k) {
    HIPCHECK(hipMalloc(&d_arena[k], store_bound));
    HIPCHECK(hipMemset(d_arena[k], 0, store_bound));
    HIPCHECK(hipMalloc(&d_entries[k], n_clips * sizeof(glc_store_entry)));
  }
  {
    const std::vector<float> base = base_signal(sr, ch, 10ull * sr);
    std::vector<float> x(n);
    std::vector<int16_t> q;
    for (uint64_t i = 0; i < n_clips; ++i) {
      fill_clip(x, base, ch, i, i % 4 == 3);
      quantise(x, q);
      HIPCHECK(hipMemcpy(d_int + i * n, q.data(), n * sizeof(int16_t), hipMemcpyHostToDevice));
    }
  }
  auto arm_a = [&] {  // every call fills its arena from the start
    if (hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st) != hipSuccess) return 1;
    const int rc = glc_pcm_widen_device(ctx, d_int, GLC_PCM_S16, 16, n_clips * n, d_scratch);
    return rc ? rc : glc_encode_batch_device_compact(ctx, d_scratch, &lay, d_arena[0], store_bound, d_cursor, d_entries[0]);
  };
  auto arm_b = [&] {
    if (hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st) != hipSuccess) return 1;
    return glc_encode_batch_device_compact_int(ctx, d_int, GLC_PCM_S16, 16, &lay, d_arena[1], store_bound, d_cursor, d_entries[1]);
  };
  // the same bytes, before anything is timed
  uint64_t held = 0;
  {
    uint64_t cur[2];
    CHECK(arm_a());
    CHECK(glc_ctx_synchronize(ctx));
    HIPCHECK(hipMemcpy(&cur[0], d_cursor, 8, hipMemcpyDeviceToHost));
    CHECK(arm_b());
    CHECK(glc_ctx_synchronize(ctx));
    HIPCHECK(hipMemcpy(&cur[1], d_cursor, 8, hipMemcpyDeviceToHost));
    if (cur[0] != cur[1] || cur[0] > store_bound) return std::printf("%s: the cursors differ\n", name), 1;
    held = cur[0];
    std::vector<uint8_t> a(held), b(held);
    std::vector<glc_store_entry> ea(n_clips), eb(n_clips);
    HIPCHECK(hipMemcpy(a.data(), d_arena[0], held, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b.data(), d_arena[1], held, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(ea.data(), d_entries[0], n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(eb.data(), d_entries[1], n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
    if (std::memcmp(a.data(), b.data(), held)) return std::printf("%s: the arenas differ\n", name), 1;
    if (std::memcmp(ea.data(), eb.data(), n_clips * sizeof(glc_store_entry))) return std::printf("%s: the entries differ\n", name), 1;
  }
  Timer timed;
  if (timed.init(st)) return 1;
  std::printf("encode, %s: %llu clip(s) x %llu frames x %u ch at %u Hz, int16; %d interleaved reps (ms per call: median [p10 .. p90])\n", name,
              (unsigned long long)n_clips, (unsigned long long)plan.n_frames, ch, sr, reps);
  if (race(timed, arm_a, arm_b, reps, "glc_pcm_widen_device + glc_encode_batch_device_compact", "glc_encode_batch_device_compact_int                   "))
    return std::printf("%s: a timed call failed: %s\n", name, glc_last_error(nullptr)), 1;
  std::printf("  bytes: input %llu (int16); (a) also writes and reads a float scratch batch of %llu; the arena holds %llu, identical in both arms\n",
              (unsigned long long)(n_clips * n * 2), (unsigned long long)(n_clips * n * 4), (unsigned long long)held);
  (void)hipFree(d_int), (void)hipFree(d_scratch), (void)hipFree(d_cursor);
  for (int k = 0; k < 2; ++k) (void)hipFree(d_arena[k]), (void)hipFree(d_entries[k]);
  glc_ctx_destroy(ctx);
  return 0;
}

// ---- draw: n_crops windows of crop_len samples per channel, crop i from clip i % n_clips (clips of clip_len samples per channel)
static int run_draw(const char *name, uint64_t n_clips, uint64_t clip_len, uint64_t n_crops, uint64_t crop_len, int reps) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = clip_len * ch;
  glc_plan plan;
  CHECK(glc_plan_encode(n, ch, &plan));
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  const glc_clip_layout in_lay{n_clips, ch, 0, n, 0, clip_len, nullptr};
  const uint64_t store_bound = glc_compact_store_bound(&in_lay);
  float *d_pcm = nullptr;
  void *d_arena = nullptr;
  uint64_t *d_cursor = nullptr;
  glc_store_entry *d_entries = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, n_clips * n * sizeof(float)));
  HIPCHECK(hipMalloc(&d_arena, store_bound));
  HIPCHECK(hipMalloc(&d_cursor, sizeof(uint64_t)));
  HIPCHECK(hipMalloc(&d_entries, n_clips * sizeof(glc_store_entry)));
  {
    const std::vector<float> base = base_signal(sr, ch, 10ull * sr);
    std::vector<float> x(n);
    for (uint64_t i = 0; i < n_clips; ++i) {
      fill_clip(x, base, ch, i, i % 4 == 3);
      HIPCHECK(hipMemcpy(d_pcm + i * n, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIPCHECK(hipMemset(d_cursor, 0, sizeof(uint64_t)));
  CHECK(glc_encode_batch_device_compact(ctx, d_pcm, &in_lay, d_arena, store_bound, d_cursor, d_entries));
  CHECK(glc_ctx_synchronize(ctx));
  (void)hipFree(d_pcm);
  std::vector<int64_t> clips(n_crops), starts(n_crops), lengths(n_clips, static_cast<int64_t>(clip_len));
  uint32_t s = 2463534242u;
  for (uint64_t i = 0; i < n_crops; ++i) {
    s = 1664525u * s + 1013904223u;
    clips[i] = static_cast<int64_t>(i % n_clips);
    starts[i] = static_cast<int64_t>((static_cast<uint64_t>(s) * 2654435761ull) % (clip_len - crop_len + 1));
  }
  int64_t *d_clips = nullptr, *d_starts = nullptr, *d_lengths = nullptr;
  HIPCHECK(hipMalloc(&d_clips, n_crops * 8));
  HIPCHECK(hipMalloc(&d_starts, n_crops * 8));
  HIPCHECK(hipMalloc(&d_lengths, n_clips * 8));
  HIPCHECK(hipMemcpy(d_clips, clips.data(), n_crops * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_starts, starts.data(), n_crops * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_lengths, lengths.data(), n_clips * 8, hipMemcpyHostToDevice));
  const glc_clip_layout out_lay{n_crops, ch, 0, crop_len * ch, 0, crop_len, nullptr};
  const uint64_t out_elems = n_crops * crop_len * ch;
  float *d_out = nullptr;
  int16_t *d_out16 = nullptr;
  HIPCHECK(hipMalloc(&d_out, out_elems * sizeof(float)));
  HIPCHECK(hipMalloc(&d_out16, out_elems * sizeof(int16_t)));
  auto arm_a = [&] {
    return glc_decode_crops_device_store(ctx, d_arena, store_bound, d_entries, d_lengths, n_clips, clip_len, d_clips, d_starts, crop_len, d_out,
                                         &out_lay);
  };
  auto arm_b = [&] {
    return glc_decode_crops_device_store_i16(ctx, d_arena, store_bound, d_entries, d_lengths, n_clips, clip_len, d_clips, d_starts, crop_len,
                                             d_out16, &out_lay);
  };
  {
    std::vector<glc_compact_status> sa(n_crops), sb(n_crops);
    CHECK(arm_a());
    CHECK(glc_decode_compact_last_status(ctx, sa.data(), n_crops));
    CHECK(arm_b());
    CHECK(glc_decode_compact_last_status(ctx, sb.data(), n_crops));
    std::vector<float> a(out_elems);
    std::vector<int16_t> b(out_elems);
    HIPCHECK(hipMemcpy(a.data(), d_out, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b.data(), d_out16, out_elems * sizeof(int16_t), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < out_elems; ++i)
      if (narrow(a[i]) != b[i]) return std::printf("%s: sample %llu of the int16 draw is not the narrowed float one\n", name, (unsigned long long)i), 1;
    if (std::memcmp(sa.data(), sb.data(), n_crops * sizeof(glc_compact_status))) return std::printf("%s: the status words differ\n", name), 1;
  }
  Timer timed;
  if (timed.init(st)) return 1;
  std::printf("draw, %s: %llu crop(s) of %llu samples from %llu clip(s) of %llu frames x %u ch at %u Hz; %d interleaved reps "
              "(ms per call: median [p10 .. p90])\n", name, (unsigned long long)n_crops, (unsigned long long)crop_len, (unsigned long long)n_clips,
              (unsigned long long)plan.n_frames, ch, sr, reps);
  if (race(timed, arm_a, arm_b, reps, "glc_decode_crops_device_store    ", "glc_decode_crops_device_store_i16"))
    return std::printf("%s: a timed call failed: %s\n", name, glc_last_error(nullptr)), 1;
  std::printf("  bytes written per call: (a) %llu, (b) %llu\n", (unsigned long long)(out_elems * 4), (unsigned long long)(out_elems * 2));
  (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries), (void)hipFree(d_out), (void)hipFree(d_out16);
  (void)hipFree(d_clips), (void)hipFree(d_starts), (void)hipFree(d_lengths);
  glc_ctx_destroy(ctx);
  return 0;
}

// ---- trace: the two new calls and nothing else
static int run_trace(uint64_t n_clips) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t per_ch = sr / 4, n = per_ch * ch, crop_len = sr / 8;
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  const glc_clip_layout lay{n_clips, ch, 0, n, 0, per_ch, nullptr};
  const uint64_t store_bound = glc_compact_store_bound(&lay);
  int16_t *d_int = nullptr, *d_out16 = nullptr;
  void *d_arena = nullptr;
  uint64_t *d_cursor = nullptr;
  glc_store_entry *d_entries = nullptr;
  int64_t *d_clips = nullptr, *d_starts = nullptr, *d_lengths = nullptr;
  HIPCHECK(hipMalloc(&d_int, n_clips * n * sizeof(int16_t)));
  HIPCHECK(hipMalloc(&d_arena, store_bound));
  HIPCHECK(hipMalloc(&d_cursor, sizeof(uint64_t)));
  HIPCHECK(hipMalloc(&d_entries, n_clips * sizeof(glc_store_entry)));
  HIPCHECK(hipMalloc(&d_out16, n_clips * crop_len * ch * sizeof(int16_t)));
  HIPCHECK(hipMalloc(&d_clips, n_clips * 8));
  HIPCHECK(hipMalloc(&d_starts, n_clips * 8));
  HIPCHECK(hipMalloc(&d_lengths, n_clips * 8));
  // what is uploaded here happens before the first traced call: a trace shows these copies in front of the kernels
  {
    const std::vector<float> base = base_signal(sr, ch, 10ull * sr);
    std::vector<float> x(n);
    std::vector<int16_t> q;
    std::vector<int64_t> clips(n_clips), starts(n_clips), lengths(n_clips, static_cast<int64_t>(per_ch));
    for (uint64_t i = 0; i < n_clips; ++i) {
      fill_clip(x, base, ch, i, i % 4 == 3);
      quantise(x, q);
      HIPCHECK(hipMemcpy(d_int + i * n, q.data(), n * sizeof(int16_t), hipMemcpyHostToDevice));
      clips[i] = static_cast<int64_t>((i * 7) % n_clips), starts[i] = static_cast<int64_t>((i * 977) % (per_ch - crop_len + 1));
    }
    HIPCHECK(hipMemcpy(d_clips, clips.data(), n_clips * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_starts, starts.data(), n_clips * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_lengths, lengths.data(), n_clips * 8, hipMemcpyHostToDevice));
  }
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  for (int i = 0; i < 13; ++i) {
    HIPCHECK(hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st));
    CHECK(glc_encode_batch_device_compact_int(ctx, d_int, GLC_PCM_S16, 16, &lay, d_arena, store_bound, d_cursor, d_entries));
    CHECK(glc_ctx_synchronize(ctx));
  }
  const glc_clip_layout out_lay{n_clips, ch, 0, crop_len * ch, 0, crop_len, nullptr};
  for (int i = 0; i < 13; ++i) {
    CHECK(glc_decode_crops_device_store_i16(ctx, d_arena, store_bound, d_entries, d_lengths, n_clips, per_ch, d_clips, d_starts, crop_len, d_out16,
                                            &out_lay));
    CHECK(glc_ctx_synchronize(ctx));
  }
  std::printf("trace: 3 warm-up + 10 calls each of glc_encode_batch_device_compact_int and glc_decode_crops_device_store_i16, %llu clip(s) of "
              "%llu samples x %u ch, crops of %llu\n", (unsigned long long)n_clips, (unsigned long long)per_ch, ch, (unsigned long long)crop_len);
  (void)hipFree(d_int), (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries), (void)hipFree(d_out16);
  (void)hipFree(d_clips), (void)hipFree(d_starts), (void)hipFree(d_lengths);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  const uint64_t sr = 48000;
  if (argc > 1 && !std::strcmp(argv[1], "trace")) return run_trace(argc > 2 ? std::max<uint64_t>(1, std::strtoull(argv[2], nullptr, 10)) : 64);
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 20;
  if (run_encode("64 clips of 2 s", 64, 2 * sr, reps)) return 1;
  if (run_encode("512 clips of 0.25 s", 512, sr / 4, reps)) return 1;
  if (run_draw("512 crops of 0.25 s from 512 clips of 10 s", 512, 10 * sr, 512, sr / 4, reps)) return 1;
  if (run_draw("64 crops of 1 s from 64 clips of 60 s", 64, 60 * sr, 64, sr, reps)) return 1;
  return 0;
}
