// stage_check.cpp - the thread protocol of the pipelined host calls (csrc/glc_stages.hpp: Worker, StageGate,
// run_stages) on the host alone, with fake stages: a stage is a loop over rounds that waits for the stage before it,
// optionally sleeps, and advances its own counter.  Two helpers and a body, as glc_encode runs them:
//   stage 0 (helper)  advances counter 0                  - the uploader
//   stage 1 (helper)  waits for counter 0, advances 1     - the launcher
//   stage 2 (body)    waits for counter 1                 - the collector
// Plain C++, no HIP header: built by tests/test_stages.py, once with -fsanitize=address,undefined and once with
// -fsanitize=thread, as
//   g++ -std=c++17 -pthread -fsanitize=... -fno-sanitize-recover=all -Wall -Werror tools/stage_check.cpp
// Exit status 0 and the line "stages ok": every check held.  A protocol that hangs ends as status 2 after a minute.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>

#include "../gapless-lossy-codec_amd/csrc/glc_stages.hpp"

static std::atomic<int> g_failed{0};
static char g_what[128] = "";  // written by the main thread between runs only
#define CHECK(cond)                                                                                             \
  do {                                                                                                          \
    if (!(cond)) {                                                                                              \
      if (g_failed.fetch_add(1) < 20) std::printf("line %d (%s): %s does not hold\n", __LINE__, g_what, #cond); \
    }                                                                                                           \
  } while (0)

static void nap(int us) {
  if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
}

// clears its flag when the helper's job ends, however it ends
struct Running {
  std::atomic<bool> &flag;
  explicit Running(std::atomic<bool> &f) : flag(f) { flag.store(true); }
  ~Running() {
    nap(200);  // a runner that does not wait returns well before this
    flag.store(false);
  }
};

constexpr int kStages = 3, kNobody = -1;
constexpr int kInjected = -100, kLater = -7;  // error codes no stage of the library uses

struct Run {
  size_t n = 0;                 // rounds
  int sleep_us[kStages] = {};   // per round, per stage
  int fail_stage = kNobody;     // this stage fails ...
  size_t fail_round = 0;        // ... instead of finishing this round
  // observed
  std::atomic<size_t> done[kStages];   // rounds a stage has finished, stored BEFORE it advances its counter
  std::atomic<size_t> begun[kStages];  // rounds a stage has begun
  size_t begun_at_failure[kStages] = {};
  std::atomic<bool> running[2];
  Run() {
    for (auto &d : done) d.store(0);
    for (auto &b : begun) b.store(0);
    for (auto &r : running) r.store(false);
  }
};

// One fake stage.  A stage that finds the pipeline stopped tries to put an error of its own in the gate, as a stage of
// the library may fail on its own account after another has: the first error must stay.
static void stage(Run &r, StageGate &gate, int s) {
  for (size_t i = 0; i < r.n; ++i) {
    r.begun[s].store(i + 1);
    if (s > 0) {
      if (!gate.wait_for(s - 1, i)) return gate.set_error(kLater, "a later error");
      CHECK(r.done[s - 1].load() > i);  // round i is seen only after its producer advanced past i
    }
    nap(r.sleep_us[s]);
    if (s == r.fail_stage && i == r.fail_round) {
      gate.set_error(kInjected, "injected: stage " + std::to_string(s) + ", round " + std::to_string(i));
      for (int o = 0; o < kStages; ++o) r.begun_at_failure[o] = r.begun[o].load();
      return;
    }
    r.done[s].store(i + 1);
    if (s < 2 && !gate.advance(s)) return gate.set_error(kLater, "a later error");
  }
}

static void run(Run &r, Worker (&workers)[2], StageGate &gate) {
  auto h0 = [&] {
    Running g(r.running[0]);
    stage(r, gate, 0);
  };
  auto h1 = [&] {
    Running g(r.running[1]);
    stage(r, gate, 1);
  };
  run_stages(gate, "stage_check", {{workers[0], std::ref(h0)}, {workers[1], std::ref(h1)}}, [&] { stage(r, gate, 2); });
  CHECK(!r.running[0].load() && !r.running[1].load());  // the runner never returns while a helper runs
}

int main() {
  std::atomic<bool> finished{false};
  std::thread watchdog([&] {
    for (int t = 0; t < 600 && !finished.load(); ++t) nap(100000);
    if (finished.load()) return;
    std::printf("stages: no end after a minute (%s)\n", g_what);
    std::fflush(stdout);
    std::_Exit(2);
  });
  Worker workers[2];  // started by the first run, parked between the runs as a context parks them

  // ordering: every stage finishes every round, nobody fails; equal stages, a slow producer, a slow consumer
  const int speeds[][kStages] = {{0, 0, 0}, {300, 0, 0}, {0, 300, 0}, {0, 0, 300}, {50, 100, 20}};
  for (size_t n : {size_t(1), size_t(2), size_t(50)})
    for (const auto &sp : speeds) {
      std::snprintf(g_what, sizeof g_what, "ordering, %zu rounds, sleeps %d %d %d", n, sp[0], sp[1], sp[2]);
      Run r;
      r.n = n;
      for (int s = 0; s < kStages; ++s) r.sleep_us[s] = n > 2 ? sp[s] / 10 : sp[s];
      StageGate gate;
      run(r, workers, gate);
      CHECK(!gate.failed() && gate.code() == GLC_OK && gate.message().empty());
      for (int s = 0; s < kStages; ++s) CHECK(r.done[s].load() == n);
      CHECK(gate.passed(0, n - 1) && gate.passed(1, n - 1) && !gate.passed(0, n) && !gate.passed(1, n));
    }

  // failure: in every stage, at the first, a middle and the last round
  for (int fs = 0; fs < kStages; ++fs)
    for (size_t fr : {size_t(0), size_t(25), size_t(49)})
      for (const auto &sp : speeds) {
        std::snprintf(g_what, sizeof g_what, "failure in stage %d at round %zu, sleeps %d %d %d", fs, fr, sp[0], sp[1], sp[2]);
        Run r;
        r.n = 50;
        for (int s = 0; s < kStages; ++s) r.sleep_us[s] = sp[s] / 10;
        r.fail_stage = fs, r.fail_round = fr;
        StageGate gate;
        run(r, workers, gate);
        // the first error comes back, not one a stage raised when it found the pipeline stopped
        CHECK(gate.failed() && gate.code() == kInjected);
        CHECK(gate.message() == "injected: stage " + std::to_string(fs) + ", round " + std::to_string(fr));
        CHECK(!gate.wait_for(0, 0));  // ... and every wait says so from then on, whatever the counter holds
        for (int s = 0; s < kStages; ++s) {
          // a stage behind the failed one never sees the round that failed; one in front of it ends within the round it
          // was in when the error was set (at most: it had just finished one and begins the next before it looks)
          if (s > fs) CHECK(r.done[s].load() <= fr);
          if (s != fs) CHECK(r.begun[s].load() <= r.begun_at_failure[s] + 1);
          if (s == fs) CHECK(r.done[s].load() == fr);
        }
      }

  // stop() from the body releases a helper blocked in wait_for: nobody ever advances counter 0
  for (int who_stops = 0; who_stops < 2; ++who_stops) {
    std::snprintf(g_what, sizeof g_what, "stop, %s", who_stops ? "by the body" : "by the runner behind an empty body");
    StageGate gate;
    std::atomic<bool> running{false}, released{false};
    auto blocked = [&] {
      Running g(running);
      released.store(!gate.wait_for(0, 0));
    };
    run_stages(gate, "stage_check", {{workers[0], std::ref(blocked)}}, [&] {
      nap(2000);  // let it block first
      if (who_stops) gate.stop();
    });
    CHECK(released.load() && !running.load());
    CHECK(!gate.failed() && gate.code() == GLC_OK);  // stopping is not failing
    CHECK(!gate.advance(0) && !gate.wait_for(0, 0));  // the counter has passed 0 now, and the gate stays stopped
  }

  // a job that throws comes back as GLC_ENOMEM "<who>: host allocation failed": a helper's, then the body's; the
  // other stage is released either way
  for (int thrower = 0; thrower < 2; ++thrower) {
    std::snprintf(g_what, sizeof g_what, "an exception in %s", thrower ? "the body" : "a helper");
    StageGate gate;
    std::atomic<bool> running{false};
    bool body_released = false;
    auto helper = [&] {
      Running g(running);
      if (thrower == 0) throw std::bad_alloc();
      (void)gate.wait_for(1, 0);
    };
    run_stages(gate, "stage_check", {{workers[1], std::ref(helper)}}, [&] {
      if (thrower == 1) throw std::runtime_error("anything");
      body_released = !gate.wait_for(0, 0);
    });
    CHECK(!running.load() && (thrower == 1 || body_released));
    CHECK(gate.failed() && gate.code() == GLC_ENOMEM && gate.message() == "stage_check: host allocation failed");
  }

  // no helpers at all (a stream of a single round): the body runs on the caller, its exceptions are caught as well
  {
    std::snprintf(g_what, sizeof g_what, "no helpers");
    StageGate gate;
    bool ran = false;
    run_stages(gate, "stage_check", {}, [&] { ran = true; });
    CHECK(ran && !gate.failed());
    StageGate gate2;
    run_stages(gate2, "stage_check", {}, [&] { throw std::bad_alloc(); });
    CHECK(gate2.code() == GLC_ENOMEM && gate2.message() == "stage_check: host allocation failed");
  }

  // a Worker runs its jobs back to back on ONE thread, which is not the caller's
  {
    std::snprintf(g_what, sizeof g_what, "Worker, 1000 jobs");
    Worker w;
    int count = 0;  // written by the jobs, read behind wait(): the Worker's mutex orders them
    std::thread::id first, now;
    for (int k = 0; k < 1000; ++k) {
      w.submit([&] {
        ++count;
        now = std::this_thread::get_id();
      });
      w.wait();
      if (k == 0) first = now;
      CHECK(count == k + 1 && now == first);
    }
    CHECK(first != std::this_thread::get_id());
  }
  // ... and one that never got a job has no thread to join
  {
    std::snprintf(g_what, sizeof g_what, "Worker, no job");
    Worker w;
    CHECK(!w.th.joinable());
  }

  finished.store(true);
  watchdog.join();
  if (g_failed.load()) {
    std::printf("stages: %d checks failed\n", g_failed.load());
    return 1;
  }
  std::printf("stages ok\n");
  return 0;
}
