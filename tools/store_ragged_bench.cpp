// store_ragged_bench.cpp — what drawing RAGGED crops from the store costs and saves (glc_decode_ragged_crops_device_store).
//   1. the cost of the new call on a selection the fixed draw accepts: every crop inside its clip, d_want == NULL,
//      (a) glc_decode_ragged_crops_device_store against (b) glc_decode_crops_device_store on the same selection - the
//      launches differ by at most one descriptor per crop
//   2. the case the call exists for: a store in which a third of the clips are shorter than the crop (with a single
//      clip: a third of the starts lie in its last `length` samples), (a) the new call, d_valid written, against (b)
//      the path a caller has without it: download the selection and the lengths (three copies that synchronise),
//      work out the valid lengths on the host, zero the output, glc_decode_crops_device_compact with ragged lengths
//      (the entries are downloaded once, outside the timing)
// Per call and arm: the device time (two events on the context's stream around the arm) and the host wall time INSIDE
// the arm (the calls return without synchronising; the downloads of (b) are inside its wall time, because the step
// cannot skip them).  Both arms on one context in one process, interleaved b a b' a after a warm-up; b' is (b)
// again and the difference of its two medians is the run's own A/A spread.  Outputs, valid lengths and status words
// of the two arms are compared before anything is timed.
// Shapes, 48 kHz stereo (those of store_draw_bench): 64 crops of 1 s from 64 clips of 60 s; 512 crops of 0.25 s from 512
// clips of 10 s; 64 crops of 1 s from ONE clip of 10 minutes.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_ragged_bench [reps = 20]
//        build/store_ragged_bench trace [crops = 64]   3 warm-up + 10 calls of the new call on the store of measurement 2
//                                                      and nothing else (for a kernel and memory-copy trace): crops of 1 s
//                                                      from as many clips of 10 s, a third of them shorter
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

// n_crops rows of crop_len samples per channel, crop i from clip i % n_clips (clips of clip_len samples per channel; with
// `ragged` every third clip is shorter than the row, or - one clip - every third start lies in its last crop_len samples)
static int run(const char *name, uint64_t n_clips, uint64_t clip_len, uint64_t n_crops, uint64_t crop_len, int reps, bool ragged, bool trace) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t n = clip_len * ch;
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  // ---- the store: every clip encoded into an arena; the short clips are the first samples of their slot
  std::vector<uint64_t> clip_lens(n_clips, clip_len);
  std::vector<int64_t> lengths(n_clips);
  uint64_t n_short = 0;
  for (uint64_t i = 0; i < n_clips; ++i) {
    if (ragged && n_clips >= 3 && i % 3 == 2) clip_lens[i] = crop_len * (2 + i % 5) / 8, ++n_short;  // 0.25 .. 0.75 of the row
    lengths[i] = static_cast<int64_t>(clip_lens[i]);
  }
  const glc_clip_layout in_lay{n_clips, ch, 0, n, 0, clip_len, clip_lens.data()};
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
  // ---- the selection (a fixed draw), on the device
  std::vector<int64_t> clips(n_crops), starts(n_crops);
  uint32_t s = 2463534242u;
  uint64_t n_cut = 0;
  for (uint64_t i = 0; i < n_crops; ++i) {
    s = 1664525u * s + 1013904223u;
    const uint64_t c = i % n_clips, len = clip_lens[c], r = static_cast<uint64_t>(s) * 2654435761ull;
    clips[i] = static_cast<int64_t>(c);
    if (!ragged) starts[i] = static_cast<int64_t>(r % (len - crop_len + 1));
    else if (len < crop_len) starts[i] = static_cast<int64_t>(r % (len / 2));                                  // a short clip
    else if (n_clips < 3 && i % 3 == 2) starts[i] = static_cast<int64_t>(len - crop_len + 1 + r % (crop_len - 1));  // cut by the end
    else starts[i] = static_cast<int64_t>(r % (len - crop_len + 1));
    n_cut += static_cast<uint64_t>(starts[i]) + crop_len > len;
  }
  int64_t *d_clips = nullptr, *d_starts = nullptr, *d_lengths = nullptr, *d_valid = nullptr;
  HIPCHECK(hipMalloc(&d_clips, n_crops * 8));
  HIPCHECK(hipMalloc(&d_starts, n_crops * 8));
  HIPCHECK(hipMalloc(&d_lengths, n_clips * 8));
  HIPCHECK(hipMalloc(&d_valid, n_crops * 8));
  HIPCHECK(hipMemcpy(d_clips, clips.data(), n_crops * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_starts, starts.data(), n_crops * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_lengths, lengths.data(), n_clips * 8, hipMemcpyHostToDevice));
  const glc_clip_layout out_lay{n_crops, ch, 0, crop_len * ch, 0, crop_len, nullptr};
  const uint64_t out_elems = n_crops * crop_len * ch;
  float *d_out = nullptr, *d_out_parent = nullptr;
  HIPCHECK(hipMalloc(&d_out, out_elems * sizeof(float)));
  HIPCHECK(hipMalloc(&d_out_parent, out_elems * sizeof(float)));
  uint64_t max_hops = 0, max_descs = 0, max_frames = 0;
  CHECK(glc_store_crop_slots(crop_len, ch, &max_hops, &max_frames));
  CHECK(glc_store_ragged_slots(crop_len, ch, &max_descs, &max_frames));
  auto call_new = [&] {
    return glc_decode_ragged_crops_device_store(ctx, d_arena, store_bound, d_entries, d_lengths, n_clips, clip_len, d_clips, d_starts,
                                                nullptr, crop_len, d_out, &out_lay, ragged ? d_valid : nullptr);
  };
  if (trace) {
    for (int i = 0; i < 13; ++i) {
      CHECK(call_new());
      CHECK(glc_ctx_synchronize(ctx));
    }
    std::printf("trace: 3 warm-up + 10 calls, %llu crop(s) in slots of %llu frames and %llu descriptors, %llu per round; %llu of %llu "
                "clips are shorter than the row\n", (unsigned long long)n_crops, (unsigned long long)max_frames, (unsigned long long)max_descs,
                (unsigned long long)(4097 / (max_frames + 1)), (unsigned long long)n_short, (unsigned long long)n_clips);
    return 0;
  }
  // ---- the other arm.  1: the fixed draw.  2: the caller's path today; the entries come down once, outside the timing
  std::vector<glc_store_entry> entries(n_clips);
  HIPCHECK(hipMemcpy(entries.data(), d_entries, n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  for (const glc_store_entry &e : entries)
    if (!e.stored) return std::printf("%s: a clip did not fit the arena\n", name), 1;
  std::vector<const void *> crop_blob(n_crops);
  std::vector<uint64_t> crop_bytes(n_crops), crop_ns(n_crops), valid(n_crops);
  std::vector<glc_crop> crops(n_crops);
  std::vector<int64_t> h_clips(n_crops), h_starts(n_crops), h_lengths(n_clips);
  glc_clip_layout host_lay = out_lay;
  host_lay.lengths = valid.data();
  auto call_fixed = [&] {
    return glc_decode_crops_device_store(ctx, d_arena, store_bound, d_entries, d_lengths, n_clips, clip_len, d_clips, d_starts, crop_len,
                                         d_out_parent, &out_lay);
  };
  auto call_host = [&]() -> int {  // selection and lengths come down (each copy synchronises), v on the host, zeros, the pointer call
    if (hipMemcpyAsync(h_clips.data(), d_clips, n_crops * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h_starts.data(), d_starts, n_crops * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h_lengths.data(), d_lengths, n_clips * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return 1;
    for (uint64_t i = 0; i < n_crops; ++i) {
      const size_t c = static_cast<size_t>(h_clips[i]);
      const glc_store_entry &e = entries[c];
      const uint64_t len = static_cast<uint64_t>(h_lengths[c]), at = static_cast<uint64_t>(h_starts[i]);
      valid[i] = std::min(crop_len, len - at);
      crop_blob[i] = static_cast<const uint8_t *>(d_arena) + e.offset, crop_bytes[i] = e.bytes;
      crop_ns[i] = len * ch;
      crops[i] = glc_crop{at, valid[i]};
    }
    if (hipMemsetAsync(d_out_parent, 0, out_elems * sizeof(float), st) != hipSuccess) return 1;
    return glc_decode_crops_device_compact(ctx, crop_blob.data(), crop_bytes.data(), crop_ns.data(), crops.data(), d_out_parent, &host_lay);
  };
  auto call_parent = [&]() -> int { return ragged ? call_host() : call_fixed(); };
  // the same bytes, valid lengths and status words, before anything is timed
  {
    std::vector<glc_compact_status> sa(n_crops), sb(n_crops);
    CHECK(call_new());
    CHECK(glc_decode_compact_last_status(ctx, sa.data(), n_crops));
    CHECK(call_parent());
    CHECK(glc_decode_compact_last_status(ctx, sb.data(), n_crops));
    std::vector<float> a(out_elems), b(out_elems);
    HIPCHECK(hipMemcpy(a.data(), d_out, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b.data(), d_out_parent, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    if (std::memcmp(a.data(), b.data(), out_elems * sizeof(float))) return std::printf("%s: the two arms' crops differ\n", name), 1;
    for (uint64_t i = 0; i < n_crops; ++i)
      if (sa[i].flags || sa[i].n_bad_rows || sb[i].flags || sb[i].n_bad_rows) return std::printf("%s: a crop's status is not clean\n", name), 1;
    if (ragged) {
      std::vector<int64_t> v(n_crops);
      HIPCHECK(hipMemcpy(v.data(), d_valid, n_crops * 8, hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n_crops; ++i)
        if (static_cast<uint64_t>(v[i]) != valid[i]) return std::printf("%s: a valid length differs from the host's\n", name), 1;
    }
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
  std::printf("%s, measurement %d: %llu row(s) of %llu samples from %llu clip(s) of %llu samples x %u ch at %u Hz, %llu clip(s) shorter than "
              "the row, %llu crop(s) cut by their clip's end; %d interleaved reps (ms per call: median [p10 .. p90])\n", name, ragged ? 2 : 1,
              (unsigned long long)n_crops, (unsigned long long)crop_len, (unsigned long long)n_clips, (unsigned long long)clip_len, ch, sr,
              (unsigned long long)n_short, (unsigned long long)n_cut, reps);
  const char *what[2] = {"device time (events around the arm)", "host wall time inside the arm     "};
  const char *parent = ragged ? "(b) download selection + lengths, v on the host, memset, glc_decode_crops_device_compact"
                              : "(b) glc_decode_crops_device_store                                                       ";
  std::vector<double> *tb[2] = {&db, &hb}, *tb2[2] = {&db2, &hb2}, *ta[2] = {&da, &ha};
  for (int k = 0; k < 2; ++k) {
    const Stat A = stat(*ta[k]), B = stat(*tb[k]), B2 = stat(*tb2[k]);
    const double spread = std::fabs(B.med - B2.med);
    std::printf("  %s\n", what[k]);
    std::printf("    %s   %.4f [%.4f .. %.4f]   again %.4f   A/A spread %.4f\n", parent, B.med, B.p10, B.p90, B2.med, spread);
    std::printf("    (a) glc_decode_ragged_crops_device_store                                                   %.4f [%.4f .. %.4f]   "
                "new - parent %+.4f   parent / new %.2f  -> %s\n",
                A.med, A.p10, A.p90, A.med - std::min(B.med, B2.med), std::min(B.med, B2.med) / A.med, verdict(A.med, B.med, B2.med, spread));
  }
  const uint64_t per_round = 4097 / (max_frames + 1), rounds = (n_crops + per_round - 1) / per_round;
  std::printf("  geometry: slots of %llu frames, %llu descriptors (fixed draw: %llu), %llu crop(s) per round, %llu round(s); copies per call: "
              "(a) none; (b) %s\n", (unsigned long long)max_frames, (unsigned long long)max_descs, (unsigned long long)max_hops,
              (unsigned long long)per_round, (unsigned long long)rounds,
              ragged ? "3 device-to-host (clips, starts, lengths), 1 host-to-device (the table image), 1 memset of the output" : "none");
  (void)hipEventDestroy(ev0), (void)hipEventDestroy(ev1);
  (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries), (void)hipFree(d_out), (void)hipFree(d_out_parent);
  (void)hipFree(d_clips), (void)hipFree(d_starts), (void)hipFree(d_lengths), (void)hipFree(d_valid);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  const uint64_t sr = 48000;
  if (argc > 1 && !std::strcmp(argv[1], "trace")) {
    const uint64_t crops = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 64;
    return run("trace", crops, 10 * sr, crops, sr, 0, true, true);
  }
  const int reps = argc > 1 ? std::max(5, std::atoi(argv[1])) : 20;
  for (int ragged = 0; ragged < 2; ++ragged) {
    if (run("64 crops of 1 s from 64 clips of 60 s", 64, 60 * sr, 64, sr, reps, ragged, false)) return 1;
    if (run("512 crops of 0.25 s from 512 clips of 10 s", 512, 10 * sr, 512, sr / 4, reps, ragged, false)) return 1;
    if (run("64 crops of 1 s from ONE clip of 10 min", 1, 600 * sr, 64, sr, reps, ragged, false)) return 1;
  }
  return 0;
}
