// h2d_probe.cpp — what does it cost to get a caller-owned (pageable) PCM buffer onto the device?
// Decides the staging strategy of glc_encode / glc_decode: plain hipMemcpy from pageable
// memory, hipHostRegister + async copy + unregister, or a copy through a pinned ring.
// Build: hipcc -O2 tools/h2d_probe.cpp -o build/h2d_probe        Usage: build/h2d_probe [MiB = 32]
//        build/h2d_probe clips N KiB    the staging of glc_encode_batch: N pageable clips of KiB each, one copy per
//                                       clip straight into its slot against packing them on the host + one copy
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define OK(x)                                                                          \
  do {                                                                                 \
    hipError_t e = (x);                                                                \
    if (e != hipSuccess) {                                                             \
      std::printf("%s: %s\n", #x, hipGetErrorString(e));                               \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// N clips of `bytes` each, every one a buffer of its own (as a caller's files are), to N slots of one
// device buffer: per-clip copies from pageable memory, or memcpy into one pinned image and one copy.
static int clips_mode(size_t n_clips, size_t bytes) {
  const size_t slot = (bytes + 4095) / 4096 * 4096 + 4096, total = n_clips * slot;
  void *d = nullptr, *pin = nullptr;
  OK(hipMalloc(&d, total));
  OK(hipHostMalloc(&pin, total, hipHostMallocDefault));
  std::memset(pin, 0, total);
  std::vector<std::vector<char>> clips(n_clips);
  for (size_t i = 0; i < n_clips; ++i) clips[i].assign(bytes, static_cast<char>(i + 1));
  hipStream_t s;
  OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  auto median = [&](const char *name, auto fn) {
    std::vector<double> t;
    for (int i = 0; i < 15; ++i) {
      const double t0 = now_ms();
      fn();
      t.push_back(now_ms() - t0);
    }
    std::sort(t.begin(), t.end());
    std::printf("%-62s %8.3f ms [%.3f .. %.3f]\n", name, t[7], t[1], t[13]);
  };
  std::printf("%zu clips of %zu KiB (%.1f MB)\n", n_clips, bytes >> 10, n_clips * bytes / 1e6);
  for (int rep = 0; rep < 2; ++rep) {  // twice: the second pass shows what order and warm pages do to the pair
    median("one hipMemcpyAsync per clip from pageable + memset + sync", [&] {
      OK(hipMemsetAsync(d, 0, total, s));
      for (size_t i = 0; i < n_clips; ++i)
        OK(hipMemcpyAsync(static_cast<char *>(d) + i * slot, clips[i].data(), bytes, hipMemcpyHostToDevice, s));
      OK(hipStreamSynchronize(s));
    });
    median("memcpy per clip into a pinned image + one copy + sync", [&] {
      for (size_t i = 0; i < n_clips; ++i) std::memcpy(static_cast<char *>(pin) + i * slot, clips[i].data(), bytes);
      OK(hipMemcpyAsync(d, pin, total, hipMemcpyHostToDevice, s));
      OK(hipStreamSynchronize(s));
    });
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 3 && !std::strcmp(argv[1], "clips")) return clips_mode(std::atoi(argv[2]), static_cast<size_t>(std::atoi(argv[3])) << 10);
  const size_t mib = argc > 1 ? std::atoi(argv[1]) : 32;
  const size_t n = mib << 20;
  void *d = nullptr;
  OK(hipMalloc(&d, n));
  std::vector<char> page(n, 1);  // pageable, touched
  void *pin = nullptr;
  OK(hipHostMalloc(&pin, n, hipHostMallocDefault));
  std::memset(pin, 2, n);
  hipStream_t s;
  OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  size_t bytes_moved = n;  // what the GB/s column divides by
  auto best = [&](const char *name, auto fn) {
    double b = 1e30;
    for (int i = 0; i < 7; ++i) {
      const double t0 = now_ms();
      fn();
      const double t = now_ms() - t0;
      if (t < b) b = t;
    }
    std::printf("%-58s %8.3f ms  %7.1f GB/s\n", name, b, bytes_moved / (b * 1e-3) / 1e9);
  };
  best("H2D hipMemcpy from pageable", [&] { OK(hipMemcpy(d, page.data(), n, hipMemcpyHostToDevice)); });
  best("H2D hipMemcpyAsync from pageable + sync", [&] {
    OK(hipMemcpyAsync(d, page.data(), n, hipMemcpyHostToDevice, s));
    OK(hipStreamSynchronize(s));
  });
  best("H2D hipMemcpyAsync from pinned + sync", [&] {
    OK(hipMemcpyAsync(d, pin, n, hipMemcpyHostToDevice, s));
    OK(hipStreamSynchronize(s));
  });
  best("hipHostRegister + H2D async + sync + hipHostUnregister", [&] {
    OK(hipHostRegister(page.data(), n, hipHostRegisterDefault));
    OK(hipMemcpyAsync(d, page.data(), n, hipMemcpyHostToDevice, s));
    OK(hipStreamSynchronize(s));
    OK(hipHostUnregister(page.data()));
  });
  best("  hipHostRegister alone (+ unregister)", [&] {
    OK(hipHostRegister(page.data(), n, hipHostRegisterDefault));
    OK(hipHostUnregister(page.data()));
  });
  best("memcpy pageable -> pinned (1 thread)", [&] { std::memcpy(pin, page.data(), n); });
  for (int nt : {2, 4, 8}) {
    char name[96];
    std::snprintf(name, sizeof name, "memcpy pageable -> pinned (%d threads)", nt);
    best(name, [&] {
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
          const size_t a = n * t / nt, b = n * (t + 1) / nt;
          std::memcpy(static_cast<char *>(pin) + a, page.data() + a, b - a);
        });
      for (auto &x : th) x.join();
    });
  }
  best("staged: 4 chunks memcpy(4 thr) -> pinned -> H2D async, pipelined", [&] {
    const int chunks = 4, nt = 4;
    for (int c = 0; c < chunks; ++c) {
      const size_t a = n * c / chunks, b = n * (c + 1) / chunks;
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
          const size_t x = a + (b - a) * t / nt, y = a + (b - a) * (t + 1) / nt;
          std::memcpy(static_cast<char *>(pin) + x, page.data() + x, y - x);
        });
      for (auto &x : th) x.join();
      OK(hipMemcpyAsync(static_cast<char *>(d) + a, static_cast<char *>(pin) + a, b - a, hipMemcpyHostToDevice, s));
    }
    OK(hipStreamSynchronize(s));
  });
  // The figures above are best-of-7 on ONE buffer: the runtime remembers the pages it has pinned for a
  // copy (and a registration), so repeats are cheap.  A caller that hands over a new buffer for every
  // file pays for the pinning once per buffer:
  {
    double t_copy = 1e30, t_reg = 1e30;
    for (int i = 0; i < 5; ++i) {
      std::vector<char> fresh(n, static_cast<char>(i + 3));  // touched, never seen by the runtime
      double t0 = now_ms();
      OK(hipMemcpy(d, fresh.data(), n, hipMemcpyHostToDevice));
      t_copy = std::min(t_copy, now_ms() - t0);
      std::vector<char> fresh2(n, static_cast<char>(i + 5));
      t0 = now_ms();
      OK(hipHostRegister(fresh2.data(), n, hipHostRegisterDefault));
      t_reg = std::min(t_reg, now_ms() - t0);
      OK(hipHostUnregister(fresh2.data()));
    }
    std::printf("%-58s %8.3f ms  %7.1f GB/s\n", "H2D hipMemcpy from a pageable buffer never seen before", t_copy, n / (t_copy * 1e-3) / 1e9);
    std::printf("%-58s %8.3f ms\n", "hipHostRegister of a buffer never seen before", t_reg);
  }
  bytes_moved = 4 << 20;
  best("D2H hipMemcpy to pageable (4 MiB)", [&] { OK(hipMemcpy(page.data(), d, 4 << 20, hipMemcpyDeviceToHost)); });
  best("D2H hipMemcpyAsync to pinned + sync (4 MiB)", [&] {
    OK(hipMemcpyAsync(pin, d, 4 << 20, hipMemcpyDeviceToHost, s));
    OK(hipStreamSynchronize(s));
  });
  return 0;
}
