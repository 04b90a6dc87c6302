// store_draw_bench.cpp — what drawing crops from the store by DEVICE-side index and start costs and saves:
// glc_decode_crops_device_store against the path a caller had without it, for a store the encoder has just filled.
//   (a) the new call: arena + entries as the write side left them, clip indices and starts in device arrays; the call
//       uploads nothing
//   (b) the parent's path: glc_decode_crops_device_compact with the SAME selections resolved on the host - the entries
//       downloaded once outside the timing, then per call four host arrays of B values (blob pointer, size, n_samples,
//       crop) built from them, as a training step would build them for a fresh draw
// Per call and arm: the device time (two events on the context's stream around the call) and the host wall time INSIDE
// the call (it returns without synchronising); the host arrays of (b) are built inside its wall time, because the
// step cannot skip that work.  Both arms on one context in one process, interleaved b a b' a after a warm-up; b' is
// the parent's path again and the difference of its two medians is the run's own A/A spread.  The two outputs and
// the status words are compared before anything is timed.
// Shapes, 48 kHz stereo (those of store_crop_bench): 64 crops of 1 s from 64 clips of 60 s; 512 crops of 0.25 s from 512
// clips of 10 s; 64 crops of 1 s from ONE clip of 10 minutes.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_draw_bench [reps = 20]
//        build/store_draw_bench trace [crops = 64]    3 warm-up + 10 calls of the new call and nothing else (for a kernel
//                                                     and memory-copy trace): crops of 1 s from as many clips of 10 s
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

// the base signal: eight partials per channel over a period of 10 s; clip i is a cut of it at its own offset, every
// fourth clip uniform noise (raw frames)
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

static const char *verdict(double a, double b, double b2, double spread) {
  return a < std::min(b, b2) - spread ? "FASTER" : a <= std::max(b, b2) + spread ? "not slower" : "SLOWER";
}

// n_crops windows of crop_len samples per channel, crop i from clip i % n_clips (clips of clip_len samples per channel)
static int run(const char *name, uint64_t n_clips, uint64_t clip_len, uint64_t n_crops, uint64_t crop_len, int reps, bool trace) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = clip_len * ch;
  glc_plan plan;
  CHECK(glc_plan_encode(n, ch, &plan));
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  // ---- the store: every clip encoded into an arena
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
  // ---- the selection (a fixed draw), on the device for (a); the lengths of the stored clips likewise
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
  float *d_out = nullptr, *d_out_parent = nullptr;
  HIPCHECK(hipMalloc(&d_out, out_elems * sizeof(float)));
  HIPCHECK(hipMalloc(&d_out_parent, out_elems * sizeof(float)));
  uint64_t max_hops = 0, max_frames = 0;
  CHECK(glc_store_crop_slots(crop_len, ch, &max_hops, &max_frames));
  auto call_new = [&] {
    return glc_decode_crops_device_store(ctx, d_arena, store_bound, d_entries, d_lengths, n_clips, clip_len, d_clips, d_starts, crop_len,
                                         d_out, &out_lay);
  };
  if (trace) {
    for (int i = 0; i < 13; ++i) {
      CHECK(call_new());
      CHECK(glc_ctx_synchronize(ctx));
    }
    std::printf("trace: 3 warm-up + 10 calls, %llu crop(s) in slots of %llu frames, %llu per round, from clips of %llu frames x %u ch\n",
                (unsigned long long)n_crops, (unsigned long long)max_frames, (unsigned long long)(4097 / (max_frames + 1)),
                (unsigned long long)plan.n_frames, ch);
    return 0;
  }
  // ---- the parent's path: the entries come down once, outside the timing
  std::vector<glc_store_entry> entries(n_clips);
  HIPCHECK(hipMemcpy(entries.data(), d_entries, n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  uint64_t store_bytes = 0;
  for (const glc_store_entry &e : entries) {
    if (!e.stored) return std::printf("%s: a clip did not fit the arena\n", name), 1;
    store_bytes += e.bytes;
  }
  std::vector<const void *> crop_blob(n_crops);
  std::vector<uint64_t> crop_bytes(n_crops), crop_ns(n_crops);
  std::vector<glc_crop> crops(n_crops);
  auto call_parent = [&] {  // the step's host work: four arrays of B values from the selection
    for (uint64_t i = 0; i < n_crops; ++i) {
      const glc_store_entry &e = entries[static_cast<size_t>(clips[i])];
      crop_blob[i] = static_cast<const uint8_t *>(d_arena) + e.offset, crop_bytes[i] = e.bytes;
      crop_ns[i] = static_cast<uint64_t>(lengths[static_cast<size_t>(clips[i])]) * ch;
      crops[i] = glc_crop{static_cast<uint64_t>(starts[i]), crop_len};
    }
    return glc_decode_crops_device_compact(ctx, crop_blob.data(), crop_bytes.data(), crop_ns.data(), crops.data(), d_out_parent, &out_lay);
  };
  // the same bytes and the same status words, before anything is timed
  {
    std::vector<glc_compact_status> sa(n_crops), sb(n_crops);
    CHECK(call_new());
    CHECK(glc_decode_compact_last_status(ctx, sa.data(), n_crops));
    CHECK(call_parent());
    CHECK(glc_decode_compact_last_status(ctx, sb.data(), n_crops));
    std::vector<float> a(out_elems), b(out_elems);
    HIPCHECK(hipMemcpy(a.data(), d_out, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b.data(), d_out_parent, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    if (std::memcmp(a.data(), b.data(), out_elems * sizeof(float))) return std::printf("%s: the draws differ from the pointer call's crops\n", name), 1;
    for (uint64_t i = 0; i < n_crops; ++i)
      if (sa[i].flags || sa[i].n_bad_rows || sb[i].flags || sb[i].n_bad_rows) return std::printf("%s: a crop's status is not clean\n", name), 1;
  }
  hipEvent_t ev0, ev1;
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  auto timed = [&](auto &&fn, std::vector<double> *host, std::vector<double> *dev) {
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
  };
  const int warm = std::max(3, reps / 5);
  for (int i = 0; i < warm; ++i) { CHECK(timed(call_parent, nullptr, nullptr)); CHECK(timed(call_new, nullptr, nullptr)); }
  std::vector<double> hb, hb2, ha, db, db2, da;
  for (int i = 0; i < reps; ++i) {
    CHECK(timed(call_parent, &hb, &db)); CHECK(timed(call_new, &ha, &da)); CHECK(timed(call_parent, &hb2, &db2)); CHECK(timed(call_new, &ha, &da));
  }
  glc_crop_plan cp;
  uint64_t win_frames = 0;
  for (uint64_t i = 0; i < n_crops; ++i) {
    const glc_crop c{static_cast<uint64_t>(starts[i]), crop_len};
    CHECK(glc_plan_crop(n, ch, &c, &cp));
    win_frames += cp.n_frames;
  }
  std::printf("%s: %llu crop(s) of %llu samples from %llu clip(s) of %llu frames x %u ch at %u Hz; %d interleaved reps "
              "(ms per call: median [p10 .. p90])\n", name, (unsigned long long)n_crops, (unsigned long long)crop_len,
              (unsigned long long)n_clips, (unsigned long long)plan.n_frames, ch, sr, reps);
  const char *what[2] = {"device time (events around the call)", "host wall time inside the call     "};
  std::vector<double> *tb[2] = {&db, &hb}, *tb2[2] = {&db2, &hb2}, *ta[2] = {&da, &ha};
  for (int k = 0; k < 2; ++k) {
    const Stat A = stat(*ta[k]), B = stat(*tb[k]), B2 = stat(*tb2[k]);
    const double spread = std::fabs(B.med - B2.med);
    std::printf("  %s\n", what[k]);
    std::printf("    (b) glc_decode_crops_device_compact, selection resolved on the host   %.4f [%.4f .. %.4f]   again %.4f   A/A spread %.4f\n",
                B.med, B.p10, B.p90, B2.med, spread);
    std::printf("    (a) glc_decode_crops_device_store                                     %.4f [%.4f .. %.4f]   new - parent %+.4f   parent / new %.2f  -> %s\n",
                A.med, A.p10, A.p90, A.med - std::min(B.med, B2.med), std::min(B.med, B2.med) / A.med, verdict(A.med, B.med, B2.med, spread));
  }
  const uint64_t per_round = 4097 / (max_frames + 1), rounds = (n_crops + per_round - 1) / per_round;
  std::printf("  geometry: slots of %llu frames and %llu hops, %llu crop(s) per round, %llu round(s); frames through the inverse transform "
              "(b) %llu, (a) %llu; host-to-device bytes per call (b) the table image, (a) 0; the store holds %llu bytes\n",
              (unsigned long long)max_frames, (unsigned long long)max_hops, (unsigned long long)per_round, (unsigned long long)rounds,
              (unsigned long long)win_frames, (unsigned long long)(n_crops * max_frames), (unsigned long long)store_bytes);
  (void)hipEventDestroy(ev0), (void)hipEventDestroy(ev1);
  (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries), (void)hipFree(d_out), (void)hipFree(d_out_parent);
  (void)hipFree(d_clips), (void)hipFree(d_starts), (void)hipFree(d_lengths);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  const uint64_t sr = 48000;
  if (argc > 1 && !std::strcmp(argv[1], "trace")) {
    const uint64_t crops = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 64;
    return run("trace", crops, 10 * sr, crops, sr, 0, true);
  }
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 20;
  if (run("64 crops of 1 s from 64 clips of 60 s", 64, 60 * sr, 64, sr, reps, false)) return 1;
  if (run("512 crops of 0.25 s from 512 clips of 10 s", 512, 10 * sr, 512, sr / 4, reps, false)) return 1;
  if (run("64 crops of 1 s from ONE clip of 10 min", 1, 600 * sr, 64, sr, reps, false)) return 1;
  return 0;
}
