// encode_edge_bench.cpp — what the edge path of the screened encode is worth (csrc/glc_kernels.h EdgeLaunch): the frames
// whose window reaches into the stream's zero padding go to a side stream beside K1 and K2 instead of through the
// serial repair behind them.  The workload is the benchmark's (bench.py: 4096 stereo frames of the 16-tone chord at
// 48 kHz, one glc_encode_range_device per step), timed as the benchmark times it: wall clock over `steps` calls queued
// back to back, the stream waited for once at the end.  Arms, a fresh context each:
//   chord        the whole stream (rank 0 of 1): frames 0 and 4095 are edge frames; edge kind automatic / off / forced with
//                the latency transform (2) / forced with the capped one (3)
//   middle       rank 1 of 3 of the chord (frames 4096 .. 8191): no edge frame, no row fails - the yardstick: what the
//                step costs when nothing is repaired and nothing is queued on the side stream
//   noise        4096 stereo frames of full-scale noise, automatic mode: every row fails, the guard holds the screened
//                path off after the first launch
// Per arm: ms per step of every pass, the rows that failed the screen per launch, the serial repairs by kind and the
// edge launches / rows.  The edge hooks are looked up at run time, so the same source builds and runs against a library
// that does not have them (the parent of the change): their arms are then reported as absent.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/encode_edge_bench [steps = 200] [passes = 3] [warm = 70]
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "glc.h"
#include "glc_debug.h"

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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

constexpr uint32_t kSr = 48000;
constexpr uint16_t kCh = 2;
constexpr uint64_t kHop = 1024, kFrame = 2048, kFrames = 4096;

// bench.py chord(): numpy RandomState(7) - the Mersenne twister seeded as std::mt19937 is, a double from two draws -
// per channel 16 frequencies in [80, 8000) then 16 phases in [0, 2 pi); per-channel samples [t0, t0 + t_count)
static std::vector<float> chord(uint64_t t0, uint64_t t_count) {
  std::mt19937 mt(7);
  auto uniform = [&](double lo, double hi) {
    const uint32_t a = mt() >> 5, b = mt() >> 6;
    return lo + (hi - lo) * ((a * 67108864.0 + b) / 9007199254740992.0);
  };
  std::vector<double> acc(t_count * kCh, 0.0);
  for (uint16_t c = 0; c < kCh; ++c) {
    double f[16], p[16];
    for (double &v : f) v = uniform(80.0, 8000.0);
    for (double &v : p) v = uniform(0.0, 2.0 * M_PI);
    for (int k = 0; k < 16; ++k)
      for (uint64_t i = 0; i < t_count; ++i)
        acc[i * kCh + c] += 0.05 * std::sin(2.0 * M_PI * f[k] * (static_cast<double>(t0 + i) / kSr) + p[k]);
  }
  return std::vector<float>(acc.begin(), acc.end());
}

static std::vector<float> noise(uint64_t t_count) {
  std::vector<float> x(t_count * kCh);
  uint32_t s = 12345;
  for (float &v : x) {
    s = (1103515245u * s + 12345u) & 0x7FFFFFFFu;
    v = static_cast<float>((s / 1073741824.0 - 1.0) * 0.9);
  }
  return x;
}

struct Shard {
  const char *name;
  std::vector<float> pcm;
  uint64_t t0, t_count, n_samples, f0, f1;
};

// rank `rank` of `world` of a stream of kFrames * world frames: the samples its frames read
static Shard shard_of(const char *name, uint64_t rank, uint64_t world, bool is_noise) {
  const uint64_t per = kFrames * world * kHop, f0 = kFrames * rank, f1 = f0 + kFrames;
  const uint64_t lo = f0 * kHop > kHop / 2 ? f0 * kHop - kHop / 2 : 0;
  const uint64_t hi = std::min<uint64_t>(per, (f1 - 1) * kHop + kFrame - kHop / 2);
  return {name, is_noise ? noise(hi - lo) : chord(lo, hi - lo), lo, hi - lo, per * kCh, f0, f1};
}

using SetEdge = int (*)(glc_ctx *, int);
using EdgeStats = int (*)(glc_ctx *, uint64_t *, uint64_t *);

int main(int argc, char **argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 200, passes = argc > 2 ? std::atoi(argv[2]) : 3;
  const int warm = argc > 3 ? std::atoi(argv[3]) : 70;
  const SetEdge set_edge = reinterpret_cast<SetEdge>(dlsym(RTLD_DEFAULT, "glc_debug_set_encode_edge"));
  const EdgeStats edge_stats = reinterpret_cast<EdgeStats>(dlsym(RTLD_DEFAULT, "glc_debug_encode_edge_stats"));
  std::printf("encode_edge_bench: %d x %d steps after %d untimed, edge hooks %s\n", passes, steps, warm,
              set_edge && edge_stats ? "present" : "ABSENT (a library without the edge path)");

  const Shard shards[3] = {shard_of("chord", 0, 1, false), shard_of("middle shard", 1, 3, false), shard_of("noise", 0, 1, true)};
  float *d_pcm[3];
  for (int i = 0; i < 3; ++i) {
    HIPCHECK(hipMalloc(&d_pcm[i], shards[i].pcm.size() * sizeof(float)));
    HIPCHECK(hipMemcpy(d_pcm[i], shards[i].pcm.data(), shards[i].pcm.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  void *d_rec = nullptr;
  HIPCHECK(hipMalloc(&d_rec, kFrames * glc_record_bytes(kCh)));

  struct Arm {
    int shard, kind;  // kind: glc_debug_set_encode_edge (-1: leave the context alone)
    const char *label;
  };
  const Arm arms[] = {{0, -1, "edge automatic"}, {0, 1, "edge off"}, {0, 2, "edge forced (2)"}, {0, 3, "edge capped (3)"}, {1, -1, "edge automatic"},
                      {2, -1, "edge automatic"}, {0, 3, "edge capped (3)"}, {0, 2, "edge forced (2)"}, {0, -1, "edge automatic"},
                      {1, -1, "edge automatic"}};
  for (const Arm &arm : arms) {
    const Shard &sh = shards[arm.shard];
    if (arm.kind >= 0 && !set_edge) {
      std::printf("%-13s %-17s absent from this library\n", sh.name, arm.label);
      continue;
    }
    glc_ctx *ctx = nullptr;
    CHECK(glc_ctx_create(0, kSr, &ctx));
    if (arm.kind >= 0) CHECK(set_edge(ctx, arm.kind));
    auto step = [&]() {
      return glc_encode_range_device(ctx, d_pcm[arm.shard], sh.t0, sh.t_count, sh.n_samples, kCh, sh.f0, sh.f1, d_rec, nullptr);
    };
    for (int i = 0; i < warm; ++i) CHECK(step());
    CHECK(glc_ctx_synchronize(ctx));
    std::printf("%-13s %-17s [", sh.name, arm.label);
    for (int p = 0; p < passes; ++p) {
      const double t = now_ms();
      for (int i = 0; i < steps; ++i) CHECK(step());
      CHECK(glc_ctx_synchronize(ctx));
      std::printf("%s%.4f", p ? ", " : "", (now_ms() - t) / steps);
    }
    uint64_t screened = 0, repaired = 0, tiles = 0, latency = 0, el = 0, er = 0;
    CHECK(glc_debug_encode_screen_stats(ctx, &screened, &repaired));
    CHECK(glc_debug_encode_repair_stats(ctx, &tiles, &latency));
    if (edge_stats) CHECK(edge_stats(ctx, &el, &er));
    const uint64_t launches = tiles + latency;
    std::printf("] ms/step   screened launches %llu, failed rows per launch %.2f, repairs tiles/latency %llu/%llu, edge launches/rows %llu/%llu\n",
                static_cast<unsigned long long>(launches), launches ? static_cast<double>(repaired) / launches : 0.0,
                static_cast<unsigned long long>(tiles), static_cast<unsigned long long>(latency),
                static_cast<unsigned long long>(el), static_cast<unsigned long long>(er));
    glc_ctx_destroy(ctx);
  }
  for (float *p : d_pcm) (void)hipFree(p);
  (void)hipFree(d_rec);
  return 0;
}
