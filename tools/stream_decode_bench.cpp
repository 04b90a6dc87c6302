// stream_decode_bench.cpp — what a streaming decode push costs: glc_stream_dec_push_device against the call that sends
// the same rows through the same row tables, inverse transform and overlap-add, glc_decode_batch_device_compact, for
// segments that are already in HBM.
//   setup   `lanes` live streams are encoded by glc_stream_enc_push_device in P chunks of 20 ms / 100 ms / 1 s into ONE
//           arena; the entries and segment lists of every push are kept as they came
//   (a) the push: P calls in a row, call p decoding what encoder push p stored, nothing synchronised between them;
//       every call resolves its entries on the device, builds the row tables, loads and saves the lanes' carry
//   (b) the yardstick: for every one of those P calls one glc_decode_batch_device_compact over `lanes` clips that are
//       the SAME blobs, each read as a clip of its own of n * 1024 samples per channel (n frames: the header passes).
//       It is not a stream - every clip starts from silence and ends with its bare tail - so it is what the rows cost,
//       not an alternative.  A push that brought no frames has no call.
// Per arm: device time (events around the P calls on the context's stream) and host time (wall clock until the last of
// the P calls has returned, before any synchronisation).  Arms interleaved b a b' a; |b - b'| is the run's own A/A
// spread.  Before anything is timed lane 0 and the last lane are pushed to their end and their samples compared bit for
// bit with glc_decode of glc_frames_from_compact of their segments.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/stream_decode_bench [reps = 10]
//        build/stream_decode_bench trace <lanes> <chunk samples>     the encoder's pushes, then 3 warm-up + 10 decode pushes,
//                                                                    and no copy to the host anywhere (kernel and copy trace)
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
  glc_stream_dec *sd = nullptr;
  CHECK(glc_stream_enc_open(ctx, ch, lanes, &se));
  CHECK(glc_stream_dec_open(ctx, ch, lanes, &sd));
  // the frames every push completes and the samples it emits (the lanes run in lock step); push P is the finish
  std::vector<uint64_t> frames(P + 1), emits(P + 1);
  uint64_t arena_bytes = 64, total_frames = 0, done = 0, max_emit = 1;
  for (uint64_t p = 0; p <= P; ++p) {
    glc_stream_push_plan plan;
    CHECK(glc_plan_stream_push(p * chunk, p < P ? chunk : 0, p == P, &plan));
    glc_stream_dec_plan dp;
    CHECK(glc_plan_stream_dec_push(done, plan.n_frames, p == P, p == P ? per_lane : 0, &dp));
    frames[p] = plan.n_frames, emits[p] = dp.n_samples, done += plan.n_frames;
    if (p < P) total_frames += plan.n_frames;
    max_emit = std::max({max_emit, dp.n_samples, plan.n_frames * 1024});
    if (plan.n_frames) arena_bytes += lanes * ((glc_compact_bound(ch, plan.n_frames) + 63) / 64 * 64);
  }
  const uint64_t out_stride = max_emit * ch;
  float *d_pcm = nullptr, *d_out = nullptr;
  void *d_arena = nullptr;
  uint64_t *d_cursor = nullptr;
  glc_store_entry *d_entries = nullptr;
  HIPCHECK(hipMalloc(&d_pcm, lanes * stride * sizeof(float)));
  HIPCHECK(hipMalloc(&d_out, lanes * out_stride * sizeof(float)));
  HIPCHECK(hipMalloc(&d_arena, arena_bytes));
  HIPCHECK(hipMalloc(&d_cursor, sizeof(uint64_t)));
  HIPCHECK(hipMalloc(&d_entries, (P + 1) * lanes * sizeof(glc_store_entry)));
  HIPCHECK(hipMemset(d_cursor, 0, sizeof(uint64_t)));
  const std::vector<float> base = tonal_base(sr, ch, per_lane + 997 * lanes);
  for (uint64_t i = 0; i < lanes; ++i) {
    const std::vector<float> x = signal(base, ch, per_lane, i);
    HIPCHECK(hipMemcpy(d_pcm + i * stride, x.data(), stride * sizeof(float), hipMemcpyHostToDevice));
  }
  // the sending half: P pushes and the finish, appended to one arena
  std::vector<std::vector<glc_stream_seg>> segs(P + 1, std::vector<glc_stream_seg>(lanes));
  const std::vector<uint8_t> fin(lanes, 1);
  for (uint64_t p = 0; p <= P; ++p) {
    const glc_clip_layout lay{lanes, ch, 0, stride, 0, p < P ? chunk : 0, nullptr};
    uint64_t n = 0;
    CHECK(glc_stream_enc_push_device(se, d_pcm + (p < P ? p * chunk * ch : 0), GLC_PCM_F32, 32, &lay, p < P ? nullptr : fin.data(), d_arena,
                                     arena_bytes, d_cursor, d_entries + p * lanes, segs[p].data(), &n));
    if (n != (frames[p] ? lanes : 0)) return std::printf("encoder push %llu: %llu segments\n", (unsigned long long)p, (unsigned long long)n), 1;
    segs[p].resize(n);
  }
  const std::vector<uint64_t> totals(lanes, per_lane);
  auto push = [&](uint64_t p) {
    const glc_clip_layout lay{lanes, ch, 0, out_stride, 0, emits[p], nullptr};
    return glc_stream_dec_push_device(sd, d_arena, arena_bytes, d_entries + p * lanes, segs[p].data(), segs[p].size(), p < P ? nullptr : fin.data(),
                                      p < P ? nullptr : totals.data(), d_out, GLC_PCM_F32, &lay);
  };
  auto reset = [&] {
    for (uint64_t i = 0; i < lanes; ++i) glc_stream_dec_reset(sd, i);
  };
  if (trace) {
    for (uint64_t i = 0; i < 13; ++i) {
      if (i % P == 0) reset();
      CHECK(push(i % P));
    }
    CHECK(glc_ctx_synchronize(ctx));
    std::printf("trace: %llu encoder pushes, then 3 warm-up + 10 decode pushes, %llu lane(s) x %llu samples x %u ch\n", (unsigned long long)(P + 1),
                (unsigned long long)lanes, (unsigned long long)chunk, ch);
    glc_stream_dec_close(sd);
    glc_stream_enc_close(se);
    glc_ctx_destroy(ctx);
    return 0;
  }
  CHECK(glc_ctx_synchronize(ctx));
  std::vector<glc_store_entry> ent((P + 1) * lanes);
  HIPCHECK(hipMemcpy(ent.data(), d_entries, ent.size() * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  for (uint64_t p = 0; p <= P; ++p)
    for (uint64_t j = 0; j < segs[p].size(); ++j)
      if (!ent[p * lanes + j].stored || segs[p][j].stream != j) return std::printf("push %llu: a segment is not stored or not its lane's\n", (unsigned long long)p), 1;
  // the same samples, before anything is timed: lane 0 and the last lane to their end
  {
    const uint64_t watch[2] = {0, lanes - 1};
    std::vector<float> got[2];
    for (uint64_t p = 0; p <= P; ++p) {
      CHECK(push(p));
      CHECK(glc_ctx_synchronize(ctx));
      for (int w = 0; w < 2; ++w) {
        const size_t at = got[w].size();
        got[w].resize(at + emits[p] * ch);
        if (emits[p]) HIPCHECK(hipMemcpy(got[w].data() + at, d_out + watch[w] * out_stride, emits[p] * ch * sizeof(float), hipMemcpyDeviceToHost));
      }
    }
    for (int w = 0; w < 2; ++w) {
      std::vector<std::vector<uint64_t>> blobs;
      for (uint64_t p = 0; p <= P; ++p)
        if (!segs[p].empty()) {
          const glc_store_entry &e = ent[p * lanes + watch[w]];
          blobs.emplace_back((e.bytes + 7) / 8);
          HIPCHECK(hipMemcpy(blobs.back().data(), static_cast<const uint8_t *>(d_arena) + e.offset, e.bytes, hipMemcpyDeviceToHost));
        }
      std::vector<const void *> ptr;
      std::vector<uint64_t> len;
      for (uint64_t p = 0, k = 0; p <= P; ++p)
        if (!segs[p].empty()) ptr.push_back(blobs[k].data()), len.push_back(ent[p * lanes + watch[w]].bytes), ++k;
      glc_frames *f = nullptr;
      CHECK(glc_frames_from_compact(sr, stride, ch, ptr.data(), len.data(), static_cast<uint32_t>(ptr.size()), &f));
      std::vector<float> want(stride);
      uint64_t n = 0;
      CHECK(glc_decode(ctx, f, want.data(), want.size(), &n));
      glc_frames_free(f);
      if (n != got[w].size() || std::memcmp(want.data(), got[w].data(), n * sizeof(float)))
        return std::printf("lane %llu: the streamed samples differ from glc_decode\n", (unsigned long long)watch[w]), 1;
    }
  }
  // the yardstick's clips: the blobs of push p, each a clip of its own of frames[p] * 1024 samples per channel
  std::vector<std::vector<const void *>> ref_blob(P);
  std::vector<std::vector<uint64_t>> ref_bytes(P), ref_samples(P);
  for (uint64_t p = 0; p < P; ++p)
    for (uint64_t j = 0; j < segs[p].size(); ++j) {
      ref_blob[p].push_back(static_cast<const uint8_t *>(d_arena) + ent[p * lanes + j].offset);
      ref_bytes[p].push_back(ent[p * lanes + j].bytes);
      ref_samples[p].push_back(frames[p] * 1024 * ch);
    }
  auto ref = [&](uint64_t p) {
    if (!frames[p]) return 0;
    const glc_clip_layout cl{lanes, ch, 0, out_stride, 0, frames[p] * 1024, nullptr};
    return glc_decode_batch_device_compact(ctx, ref_blob[p].data(), ref_bytes[p].data(), ref_samples[p].data(), d_out, &cl);
  };
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
  std::printf("%4llu lane(s), segments of %6llu samples (%4.0f ms), %2llu pushes, %.2f frames per lane and push; %d reps, ms per call (median)\n",
              (unsigned long long)lanes, (unsigned long long)chunk, 1000.0 * chunk / sr, (unsigned long long)P, double(total_frames) / P, reps);
  std::printf("  (b) glc_decode_batch_device_compact   device %.4f  again %.4f  A/A spread %.4f   host %.4f\n", b, b2, spread,
              std::min(median(tb.host), median(tb2.host)));
  std::printf("  (a) glc_stream_dec_push_device        device %.4f  push - yardstick %+.4f  push / yardstick %.3f   host %.4f\n", a,
              a - std::min(b, b2), a / std::min(b, b2), median(ta.host));
  std::printf("      carry: %llu bytes read and %llu written per active lane and push\n", (unsigned long long)(2ull * 1024 * ch * 4),
              (unsigned long long)(2ull * 1024 * ch * 4));
  (void)hipFree(d_pcm), (void)hipFree(d_out), (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries);
  glc_stream_dec_close(sd);
  glc_stream_enc_close(se);
  glc_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 3 && !std::strcmp(argv[1], "trace")) return run(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), 16, 0, true);
  const int reps = argc > 1 ? std::max(3, std::atoi(argv[1])) : 10;
  const uint64_t lanes[4] = {64, 512, 512, 512}, chunks[4] = {4800, 960, 4800, 48000}, pushes[4] = {16, 32, 16, 4};
  for (int c = 0; c < 4; ++c)
    if (run(lanes[c], chunks[c], pushes[c], reps, false)) return 1;
  return 0;
}
