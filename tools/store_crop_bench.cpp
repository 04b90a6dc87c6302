// store_crop_bench.cpp — what decoding WINDOWS of stored clips in one call saves: glc_decode_crops_device_compact
// against the only path a caller had without it, for compact blobs that are already in HBM.
//   (a) the new call: one glc_decode_crops_device_compact into a (B, L, C) tensor, one glc_ctx_synchronize
//   (b) the parent's path: glc_decode_batch_device_compact of the whole clips the crops are cut from (each clip once)
//       into a scratch tensor, then one strided device copy of the windows (offset table + gather kernel) into
//       (B, L, C), one glc_ctx_synchronize
// Shapes, 48 kHz stereo: 64 crops of 1 s from 64 clips of 60 s; 512 crops of 0.25 s from 512 clips of 10 s; 64 crops of
// 1 s from ONE clip of 10 minutes; and the control - 64 windows that are the whole of 64 clips of 2 s, where (b) is
// the existing call straight into the tensor (no scratch, no copy) and the new call must not be slower than it by more
// than the run's A/A spread.  Both arms on one context in one process, interleaved b a b' a after a warm-up of every
// shape; b' is the parent's path again and the difference of its two medians is the run's own A/A spread.  The two
// outputs are compared byte for byte before anything is timed.  The footprint lines are arithmetic from the shapes.
// Build: make -C gapless-lossy-codec_amd/csrc tools
// Usage: build/store_crop_bench [reps = 20]
//        build/store_crop_bench trace [crops = 64]    3 warm-up + 10 calls of the new call and nothing else (for a kernel
//                                                     trace): crops of 1 s from as many clips of 10 s, one round
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

// The parent's copy of the windows: crop i is the `len` contiguous elements from src[i] of the scratch, which go to
// out + i * len.  blockIdx.y = crop, consecutive threads copy consecutive elements.
__global__ __launch_bounds__(256) void k_gather_windows(const float *__restrict__ scratch, const unsigned long long *__restrict__ src,
                                                         unsigned long long len, float *__restrict__ out) {
  const float *s = scratch + src[blockIdx.y];
  float *d = out + blockIdx.y * len;
  for (unsigned long long j = blockIdx.x * 256ull + threadIdx.x; j < len; j += gridDim.x * 256ull) d[j] = s[j];
}

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
  const bool control = crop_len == clip_len;  // whole clips: the parent is the existing call straight into the tensor
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
  std::vector<glc_store_entry> entries(n_clips);
  HIPCHECK(hipMemcpy(entries.data(), d_entries, n_clips * sizeof(glc_store_entry), hipMemcpyDeviceToHost));
  (void)hipFree(d_pcm);
  uint64_t store_bytes = 0;
  for (const glc_store_entry &e : entries) {
    if (!e.stored) return std::printf("%s: a clip did not fit the arena\n", name), 1;
    store_bytes += e.bytes;
  }
  // ---- the crops (a fixed draw), and both arms' arguments
  std::vector<const void *> crop_blob(n_crops), clip_blob(n_clips);
  std::vector<uint64_t> crop_bytes(n_crops), crop_ns(n_crops, n), clip_bytes(n_clips), clip_ns(n_clips, n), src(n_crops);
  std::vector<glc_crop> crops(n_crops);
  for (uint64_t i = 0; i < n_clips; ++i) clip_blob[i] = static_cast<const uint8_t *>(d_arena) + entries[i].offset, clip_bytes[i] = entries[i].bytes;
  uint32_t s = 2463534242u;
  uint64_t win_rows = 0, win_frames = 0;
  for (uint64_t i = 0; i < n_crops; ++i) {
    const uint64_t k = i % n_clips;
    s = 1664525u * s + 1013904223u;
    crops[i] = glc_crop{control ? 0 : (static_cast<uint64_t>(s) * 2654435761ull) % (clip_len - crop_len + 1), crop_len};
    crop_blob[i] = clip_blob[k], crop_bytes[i] = clip_bytes[k];
    src[i] = k * n + crops[i].start * ch;
    glc_crop_plan cp;
    CHECK(glc_plan_crop(n, ch, &crops[i], &cp));
    win_frames += cp.n_frames, win_rows += cp.n_frames * ch;
  }
  const glc_clip_layout out_lay{n_crops, ch, 0, crop_len * ch, 0, crop_len, nullptr};
  const glc_clip_layout scratch_lay{n_clips, ch, 0, n, 0, clip_len, nullptr};
  const uint64_t out_elems = n_crops * crop_len * ch, scratch_elems = control ? 0 : n_clips * n;
  float *d_out = nullptr, *d_out_parent = nullptr, *d_scratch = nullptr;
  unsigned long long *d_src = nullptr;
  HIPCHECK(hipMalloc(&d_out, out_elems * sizeof(float)));
  HIPCHECK(hipMalloc(&d_out_parent, out_elems * sizeof(float)));
  if (scratch_elems) HIPCHECK(hipMalloc(&d_scratch, scratch_elems * sizeof(float)));
  HIPCHECK(hipMalloc(&d_src, n_crops * sizeof(unsigned long long)));
  auto arm_new = [&] {
    const int rc = glc_decode_crops_device_compact(ctx, crop_blob.data(), crop_bytes.data(), crop_ns.data(), crops.data(), d_out, &out_lay);
    return rc ? rc : glc_ctx_synchronize(ctx);
  };
  if (trace) {
    for (int i = 0; i < 13; ++i) CHECK(arm_new());
    std::printf("trace: 3 warm-up + 10 calls, %llu crop(s) of %llu frames from clips of %llu frames x %u ch\n", (unsigned long long)n_crops,
                (unsigned long long)(win_frames / n_crops), (unsigned long long)plan.n_frames, ch);
    return 0;
  }
  auto arm_parent = [&] {
    if (control) {
      const int rc = glc_decode_batch_device_compact(ctx, clip_blob.data(), clip_bytes.data(), clip_ns.data(), d_out_parent, &out_lay);
      return rc ? rc : glc_ctx_synchronize(ctx);
    }
    int rc = glc_decode_batch_device_compact(ctx, clip_blob.data(), clip_bytes.data(), clip_ns.data(), d_scratch, &scratch_lay);
    if (rc) return rc;
    if (hipMemcpyAsync(d_src, src.data(), n_crops * sizeof(unsigned long long), hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    const unsigned bx = static_cast<unsigned>(std::min<uint64_t>(64, (crop_len * ch + 255) / 256));
    hipLaunchKernelGGL(k_gather_windows, dim3(bx, static_cast<unsigned>(n_crops)), dim3(256), 0, st, d_scratch, d_src,
                       static_cast<unsigned long long>(crop_len * ch), d_out_parent);
    if (hipGetLastError() != hipSuccess) return 1;
    return glc_ctx_synchronize(ctx);
  };
  // the same bytes, before anything is timed
  CHECK(arm_new());
  CHECK(arm_parent());
  {
    std::vector<float> a(out_elems), b(out_elems);
    HIPCHECK(hipMemcpy(a.data(), d_out, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b.data(), d_out_parent, out_elems * sizeof(float), hipMemcpyDeviceToHost));
    if (std::memcmp(a.data(), b.data(), out_elems * sizeof(float))) return std::printf("%s: the crops differ from the slices of the whole decode\n", name), 1;
    std::vector<glc_compact_status> status(n_crops);
    CHECK(glc_decode_crops_device_compact(ctx, crop_blob.data(), crop_bytes.data(), crop_ns.data(), crops.data(), d_out, &out_lay));
    CHECK(glc_decode_compact_last_status(ctx, status.data(), n_crops));
    for (const glc_compact_status &c : status)
      if (c.flags || c.n_bad_rows) return std::printf("%s: a crop's status is not clean\n", name), 1;
  }
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
  std::printf("%s: %llu crop(s) of %llu samples (%llu window frames each) from %llu clip(s) of %llu frames x %u ch at %u Hz; %d interleaved reps "
              "(ms per call: median [p10 .. p90])\n", name, (unsigned long long)n_crops, (unsigned long long)crop_len,
              (unsigned long long)(win_frames / n_crops), (unsigned long long)n_clips, (unsigned long long)plan.n_frames, ch, sr, reps);
  std::printf("  (b) %s   %.4f [%.4f .. %.4f]   again %.4f   A/A spread %.4f\n",
              control ? "glc_decode_batch_device_compact straight into the tensor            " : "glc_decode_batch_device_compact of the whole clips + copy of the windows",
              B.med, B.p10, B.p90, B2.med, spread);
  std::printf("  (a) glc_decode_crops_device_compact                                       %.4f [%.4f .. %.4f]   new - parent %+.4f   parent / new %.2f  -> %s\n",
              A.med, A.p10, A.p90, A.med - std::min(B.med, B2.med), std::min(B.med, B2.med) / A.med, verdict(A.med, B.med, B2.med, spread));
  const uint64_t clip_rows = n_clips * plan.n_frames * ch;
  std::printf("  footprint (from the shapes): scratch tensor (b) %llu bytes, (a) 0; rows tabulated per call at 32 B each (b) %llu = %llu bytes, "
              "(a) %llu = %llu bytes; frames through the inverse transform (b) %llu, (a) %llu; the store holds %llu bytes\n",
              (unsigned long long)(scratch_elems * sizeof(float)), (unsigned long long)clip_rows, (unsigned long long)(clip_rows * 32),
              (unsigned long long)win_rows, (unsigned long long)(win_rows * 32), (unsigned long long)(n_clips * plan.n_frames),
              (unsigned long long)win_frames, (unsigned long long)store_bytes);
  (void)hipFree(d_arena), (void)hipFree(d_cursor), (void)hipFree(d_entries), (void)hipFree(d_out), (void)hipFree(d_out_parent);
  (void)hipFree(d_scratch), (void)hipFree(d_src);
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
  if (run("control: 64 whole clips of 2 s", 64, 2 * sr, 64, 2 * sr, reps, false)) return 1;
  return 0;
}
