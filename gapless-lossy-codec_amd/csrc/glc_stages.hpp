// glc_stages.hpp — how the host threads of a pipelined call (glc_encode*, glc_roundtrip in glc_api.hip) hand rounds to
// each other: the parked helper thread, the gate the stages meet at, and the runner that starts the helpers beside a
// body on the calling thread.  Plain C++17 without a HIP type: a host program can include it alone
// (tools/stage_check.cpp, built under the address and the thread sanitizer).
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>

#include "../../include/glc.h"

// A parked host thread that runs one job at a time (glc_encode's uploader and launcher): started on
// first use and kept for the life of the context, because a fresh std::thread costs ~50 us before its
// first HIP call returns (thread start + the runtime's per-thread state) - 5 % of a config-2 call.
struct Worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, idle = true, quit = false;
  void submit(std::function<void()> j) {  // may throw std::system_error / std::bad_alloc on first use
    if (!th.joinable())
      th = std::thread([this] {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
          cv.wait(lk, [&] { return has_job || quit; });
          if (quit) return;
          std::function<void()> j2 = std::move(job);
          has_job = false;
          lk.unlock();
          j2();  // jobs do not throw (run_stages wraps them)
          lk.lock();
          idle = true;
          cv.notify_all();
        }
      });
    std::lock_guard<std::mutex> lk(mu);
    job = std::move(j);
    has_job = true;
    idle = false;
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return idle; });
  }
  ~Worker() {
    if (!th.joinable()) return;
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
      cv.notify_all();
    }
    th.join();
  }
};

// Where the stages of a call meet.  A stage that has finished round i advances its counter (counters only grow); the
// stage that consumes the round waits for the counter to pass i.  An error anywhere stops all of them: the FIRST one
// is kept, as a code and a message, and every wait returns false from then on - as it does once the consumer, done
// with the call, has said stop().
class StageGate {
 public:
  void set_error(int code, const std::string &m) {
    std::lock_guard<std::mutex> lk(mu_);
    if (code_ != GLC_OK) return;
    code_ = code;
    cv_.notify_all();
    try {
      msg_ = m;
    } catch (...) {  // a failure without its text is still a failure
    }
    failed_.store(true, std::memory_order_release);
  }
  void stop() {
    std::lock_guard<std::mutex> lk(mu_);
    stopped_ = true;
    cv_.notify_all();
  }
  // one more round of `counter` is done; false when its stage has nothing left to work for
  bool advance(int counter) {
    std::lock_guard<std::mutex> lk(mu_);
    ++count_[counter];
    cv_.notify_all();
    return live();
  }
  // wait until `counter` has passed i; false when another stage has failed or the consumer has stopped
  bool wait_for(int counter, size_t i) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return count_[counter] > i || !live(); });
    return live();
  }
  bool passed(int counter, size_t i) {  // without waiting
    std::lock_guard<std::mutex> lk(mu_);
    return count_[counter] > i;
  }
  bool failed() const { return failed_.load(std::memory_order_acquire); }  // no lock: for a loop that polls
  // The first error, written once.  No lock: for a thread that has seen failed() or a wait return false, or that
  // run_stages has returned to - GLC_OK and no text where nothing failed.
  int code() const { return code_; }
  const std::string &message() const { return msg_; }

 private:
  bool live() const { return code_ == GLC_OK && !stopped_; }  // under mu_
  std::mutex mu_;
  std::condition_variable cv_;
  size_t count_[2] = {};  // glc_encode: rounds uploaded, rounds queued; glc_roundtrip: rounds uploaded
  int code_ = GLC_OK;
  std::string msg_;
  bool stopped_ = false;
  std::atomic<bool> failed_{false};
};

// A helper stage of run_stages: the context's parked thread for it and its job.  Hand the job over as
// std::ref(lambda): a std::function of a reference allocates nothing.
struct Stage {
  Worker &worker;
  std::function<void()> job;
};

// Helpers beside a body on the calling thread.  Every job runs inside a catch-all that turns an exception into
// GLC_ENOMEM "<who>: host allocation failed" (nothing may cross the C ABI, and a job must not throw into its Worker).
// A helper that cannot be started is "<who>: cannot start a helper thread": the body is not run, the helpers already
// started are stopped and waited for.  Never returns while a helper runs, whatever happened - the helpers read the
// caller's frame, and this one - and never throws: what went wrong is in the gate.
template <typename Body>
void run_stages(StageGate &gate, const std::string &who, std::initializer_list<Stage> helpers, Body &&body) {
  auto report = [&](const char *what) {
    try {
      gate.set_error(GLC_ENOMEM, who + what);
    } catch (...) {
    }
  };
  auto guarded = [&](auto &job) {
    try {
      job();
    } catch (...) {
      report(": host allocation failed");
    }
  };
  size_t started = 0;
  try {
    for (const Stage &s : helpers) {
      s.worker.submit([&s, &guarded] { guarded(s.job); });
      ++started;
    }
  } catch (...) {  // std::system_error / std::bad_alloc from starting a helper
    report(": cannot start a helper thread");
  }
  if (started == helpers.size()) guarded(body);
  gate.stop();
  for (size_t k = 0; k < started; ++k) helpers.begin()[k].worker.wait();
}
