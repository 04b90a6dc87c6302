// stream_encode_bench.cpp — what a streaming push costs: glc_stream_enc_push_device against the call that sends the same
// rows through the same transform and pack, glc_encode_batch_device_compact, for samples that are already in HBM.
//   (a) the push: `lanes` live streams each receive a chunk of 20 ms / 100 ms / 1 s per call, P calls in a row, nothing
//       synchronised between them; every call stages [what was held back | what arrived], encodes the frames that
//       became final and packs one blob per lane
//   (b) the yardstick: for every one of those P calls one glc_encode_batch_device_compact over `lanes` clips of exactly
//       the frames that push completed per lane (a clip of n * 1024 + 512 samples has n frames; a push that completes
//       nothing has no call).  It is not a stream - every clip starts from silence and is zero-padded - so it is what
//       the rows cost, not an alternative.
// Per arm: device time (events around the P calls on the context's stream) and host time (wall clock until the last of
// the P calls has returned, before any synchronisation).  Arms interleaved b a b' a; |b - b'| is the run's own A/A
// spread.  Before anything is timed lane 0 and the last lane are pushed to their end and their segments, assembled by
// glc_frames_from_compact, are compared with glc_encode of the same samples byte for byte.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/stream_encode_bench [reps = 10]
//        build/stream_encode_bench trace <lanes> <chunk samples>     3 warm-up + 10 pushes and nothing else (kernel trace)
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

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
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

// eight partials per channel, a different cut of one long signal per lane; every fourth lane uniform noise (raw frames)
static std::vector<float> tonal_base(uint32_t sr, uint16_t ch, uint64_t per_ch) {
  std::vector<float> x(per_ch * ch);
  for (uint16_t c = 0; c < ch; ++c)
    for (uint64_t t = 0; t < per_ch; ++t) {
      double v = 0;
      for (int p = 0; p < 8; ++p) v += 0.05 * std::sin(2 * M_PI * (110.0 * (p + 1) * (1.0 + 0.37 * c) + 3.1 * p) * t / sr + 0.5 * p);
      x[t * ch + c] = static_cast<float>(v);
    }
  return x;
}
static std::vector<float> signal(const std::vector<float> &base, uint16_t ch, uint64_t per_ch, uint64_t lane) {
  std::vector<float> x(per_ch * ch);
  if (lane % 4 == 3) {
    uint32_t s = 12345u + static_cast<uint32_t>(lane);
    for (float &v : x) {
      s = 1664525u * s + 1013904223u;
      v = static_cast<float>(0.5 * (s / 2147483648.0 - 1.0));
    }
    return x;
  }
  std::memcpy(x.data(), base.data() + 997 * lane * ch, x.size() * sizeof(float));
  return x;
}

static int run(uint64_t lanes, uint64_t chunk, uint64_t P, int reps, bool trace) {
  const uint32_t sr = 48000;
  const uint16_t ch = 2;
  const uint64_t per_lane = P * chunk, stride = per_lane * ch;
  glc_ctx *ctx = nullptr;
  CHECK(glc_ctx_create(0, sr, &ctx));
  glc_stream_enc *se = nullptr;
  CHECK(glc_stream_enc_open(ctx, ch, lanes, &se));
  // the frames every push completes (the lanes run in lock step)
  std::vector<uint64_t> frames(P);
  uint64_t max_frames = 1, total_frames = 0;
  for (uint64_t p = 0; p < P; ++p) {
    glc_stream_push_plan plan;
    CHECK(glc_plan_stream_push(p * chunk, chunk, 0, &plan));
    frames[p] = plan.n_frames, max_frames = std::max(max_frames, plan.n_frames), total_frames += plan.n_frames;
  }
  glc_stream_push_plan last;
  CHECK(glc_plan_stream_push(per_lane, 0, 1, &last));
  max_frames = std::max(max_frames, last.n_frames);
  const uint64_t arena_bytes = lanes * ((glc_compact_bound(ch, max_frames) + 63) / 64 * 64) + 64;
  float *d_pcm = nullptr;
  void *d_arena = nullptr;
  uint64_t *d_cursor = nullptr;
  glc_store_entry *d_entries = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, lanes * stride * sizeof(float)));
  HIPCHECK(hipMalloc(&d_arena, arena_bytes));
  HIPCHECK(hipMalloc(&d_cursor, sizeof(uint64_t)));
  HIPCHECK(hipMalloc(&d_entries, lanes * sizeof(glc_store_entry)));
  std::vector<float> first, final_lane;
  const std::vector<float> base = tonal_base(sr, ch, per_lane + 997 * lanes);
  for (uint64_t i = 0; i < lanes; ++i) {
    const std::vector<float> x = signal(base, ch, per_lane, i);
    HIPCHECK(hipMemcpy(d_pcm + i * stride, x.data(), stride * sizeof(float), hipMemcpyHostToDevice));
    if (i == 0) first = x;
    if (i == lanes - 1) final_lane = x;
  }
  hipStream_t st = static_cast<hipStream_t>(glc_ctx_stream(ctx));
  std::vector<glc_stream_seg> segs(lanes);
  uint64_t n_segs = 0;
  const glc_clip_layout lay{lanes, ch, 0, stride, 0, chunk, nullptr};
  auto push = [&](uint64_t p) {
    if (hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st) != hipSuccess) return 1;  // every call fills the arena from its start
    return glc_stream_enc_push_device(se, d_pcm + p * chunk * ch, GLC_PCM_F32, 32, &lay, nullptr, d_arena, arena_bytes, d_cursor, d_entries,
                                      segs.data(), &n_segs);
  };
  auto reset = [&] {
    for (uint64_t i = 0; i < lanes; ++i) glc_stream_enc_reset(se, i);
  };
  if (trace) {
    for (uint64_t i = 0; i < 13; ++i) CHECK(push(i % P));
    CHECK(glc_ctx_synchronize(ctx));
    std::printf("trace: 3 warm-up + 10 pushes, %llu lane(s) x %llu samples x %u ch\n", (unsigned long long)lanes, (unsigned long long)chunk, ch);
    glc_stream_enc_close(se);
    glc_ctx_destroy(ctx);
    return 0;
  }
  // the same bytes, before anything is timed: lane 0 and the last lane to their end
  {
    std::vector<std::vector<uint64_t>> blobs[2];
    const uint64_t watch[2] = {0, lanes - 1};
    std::vector<uint8_t> fin(lanes, 1);
    const glc_clip_layout none{lanes, ch, 0, stride, 0, 0, nullptr};
    for (uint64_t p = 0; p <= P; ++p) {
      if (p < P) {
        CHECK(push(p));
      } else {
        HIPCHECK(hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st));
        CHECK(glc_stream_enc_push_device(se, d_pcm, GLC_PCM_F32, 32, &none, fin.data(), d_arena, arena_bytes, d_cursor, d_entries, segs.data(),
                                         &n_segs));
      }
      CHECK(glc_ctx_synchronize(ctx));
      const uint64_t want = p < P ? frames[p] : last.n_frames;
      if (n_segs != (want ? lanes : 0)) return std::printf("push %llu: %llu segments\n", (unsigned long long)p, (unsigned long long)n_segs), 1;
      std::vector<glc_store_entry> ent(n_segs);
      if (n_segs) HIPCHECK(hipMemcpy(ent.data(), d_entries, n_segs * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
      for (uint64_t j = 0; j < n_segs; ++j)
        for (int w = 0; w < 2; ++w)
          if (segs[j].stream == watch[w]) {
            if (!ent[j].stored || segs[j].n_frames != want) return std::printf("push %llu: a segment is not stored or not the plan's\n", (unsigned long long)p), 1;
            std::vector<uint64_t> b(ent[j].bytes / 8);
            HIPCHECK(hipMemcpy(b.data(), static_cast<const uint8_t *>(d_arena) + ent[j].offset, ent[j].bytes, hipMemcpyDeviceToHost));
            blobs[w].push_back(std::move(b));
          }
    }
    for (int w = 0; w < 2; ++w) {
      std::vector<const void *> ptr;
      std::vector<uint64_t> len;
      for (const auto &b : blobs[w]) ptr.push_back(b.data()), len.push_back(b.size() * 8);
      glc_frames *streamed = nullptr, *whole = nullptr;
      CHECK(glc_frames_from_compact(sr, stride, ch, ptr.data(), len.data(), static_cast<uint32_t>(ptr.size()), &streamed));
      CHECK(glc_encode(ctx, (w ? final_lane : first).data(), stride, ch, &whole));
      std::vector<uint8_t> a(glc_serialized_size(streamed)), b(glc_serialized_size(whole));
      uint64_t na = 0, nb = 0;
      CHECK(glc_serialize(streamed, a.data(), a.size(), &na));
      CHECK(glc_serialize(whole, b.data(), b.size(), &nb));
      glc_frames_free(streamed), glc_frames_free(whole);
      if (a != b) return std::printf("lane %llu: the streamed bytes differ from glc_encode\n", (unsigned long long)watch[w]), 1;
    }
  }
  // the yardstick's clips: lanes clips of n frames for every n a push completes, cut from the same samples
  auto ref = [&](uint64_t p) {
    if (!frames[p]) return 0;
    if (hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st) != hipSuccess) return 1;
    const glc_clip_layout cl{lanes, ch, 0, stride, 0, frames[p] * 1024 + 512, nullptr};
    return glc_encode_batch_device_compact(ctx, d_pcm, &cl, d_arena, arena_bytes, d_cursor, d_entries);
  };
  for (uint64_t p = 0; p < P; ++p)
    if (frames[p] && (frames[p] * 1024 + 512 > per_lane)) return std::printf("the yardstick's clip does not fit the lane's samples\n"), 1;
  struct T {
    std::vector<double> dev, host;
  };
  auto timed = [&](auto &&fn, T &into) {
    if (glc_ctx_synchronize(ctx) != GLC_OK || glc_ctx_timer_begin(ctx) != GLC_OK) return 1;
    const double t0 = now_ms();
    for (uint64_t p = 0; p < P; ++p)
      if (fn(p)) return 1;
    const double host = now_ms() - t0;
    float ms = 0;
    if (glc_ctx_timer_end(ctx, &ms) != GLC_OK) return 1;
    into.dev.push_back(ms / P), into.host.push_back(host / P);
    return 0;
  };
  T tb, tb2, ta;
  for (int i = 0; i < 2; ++i) {
    T warm;
    CHECK(timed(ref, warm));
    reset();
    CHECK(timed(push, warm));
  }
  for (int i = 0; i < reps; ++i) {
    CHECK(timed(ref, tb));
    reset();
    CHECK(timed(push, ta));
    CHECK(timed(ref, tb2));
    reset();
    CHECK(timed(push, ta));
  }
  const double b = median(tb.dev), b2 = median(tb2.dev), a = median(ta.dev), spread = std::fabs(b - b2);
  std::printf("%4llu lane(s), chunks of %6llu samples (%4.0f ms), %2llu pushes, %.2f frames per lane and push; %d reps, ms per call (median)\n",
              (unsigned long long)lanes, (unsigned long long)chunk, 1000.0 * chunk / sr, (unsigned long long)P, double(total_frames) / P, reps);
  std::printf("  (b) glc_encode_batch_device_compact   device %.4f  again %.4f  A/A spread %.4f   host %.4f\n", b, b2, spread,
              std::min(median(tb.host), median(tb2.host)));
  std::printf("  (a) glc_stream_enc_push_device        device %.4f  push - yardstick %+.4f  push / yardstick %.3f   host %.4f\n", a,
              a - std::min(b, b2), a / std::min(b, b2), median(ta.host));
  (void)hipFree(d_pcm), (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries);
  glc_stream_enc_close(se);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 3 && !std::strcmp(argv[1], "trace")) return run(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), 16, 0, true);
  const int reps = argc > 1 ? std::max(3, std::atoi(argv[1])) : 10;
  const uint64_t lanes[3] = {1, 64, 512}, chunks[3] = {960, 4800, 48000}, pushes[3] = {32, 16, 4};
  for (uint64_t l : lanes)
    for (int c = 0; c < 3; ++c)
      if (run(l, chunks[c], pushes[c], reps, false)) return 1;
  return 0;
}
