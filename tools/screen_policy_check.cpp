// screen_policy_check.cpp - the guard of the screened encode (csrc/glc_resources.hpp ScreenPolicy) on the host alone.
// The policy is handed the counts a repair launch would have left and must take the decisions its comments and
// include/glc_debug.h (glc_debug_set_encode_screen, glc_debug_set_encode_repair) state - the sequences
// tests/test_encode_screen.py pins on the device.  No device, no HIP call: built by tests/test_screen_policy.py with
//   g++ -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I$ROCM/include tools/screen_policy_check.cpp
// (the HIP headers are needed for the types of the header's other structs only).  Exit status 0: every check held.
#include <cstdio>

#include "../gapless-lossy-codec_amd/csrc/glc_resources.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

// One launch chain as the encode driver steps the guard: the words {failed, rows, seq} the device left, the launches
// queued, the seq of the last count read.  (The second chain of a context is idle here: its words never change.)
struct Chain {
  ScreenPolicy p;
  uint32_t queued = 0, judged = 0;
  uint32_t w_failed = 0, w_rows = 0, w_seq = 0;
  bool launch() {  // a launch that may take the path: screened (and then queued) or sent down today's kernels
    p.observe(judged, w_seq, w_failed, w_rows);
    const bool screened = p.admit(w_seq != queued);
    if (screened) ++queued;
    return screened;
  }
  void count_arrives(uint32_t failed, uint32_t rows) { w_failed = failed, w_rows = rows, w_seq = queued; }
  int refused_in_a_row(int limit) {
    int n = 0;
    while (n < limit && !launch()) ++n;
    return n;
  }
};

int main() {
  constexpr uint32_t kRows = 4096;
  {  // a fresh context: the first screened launch is its probe, the ones queued behind it wait for its count
    Chain c;
    CHECK(c.launch());
    for (int i = 0; i < 5; ++i) CHECK(!c.launch());
    c.count_arrives(0, kRows);
    CHECK(c.launch());
    CHECK(c.launch());  // open: a pending count holds nothing up
    // exactly one row in eight is not "more than one in eight"
    c.count_arrives(kRows / 8, kRows);
    CHECK(c.launch());
    CHECK(c.launch());
    // a bad count: 32 launches take today's kernels, then ONE probes, then nothing until its count is back
    c.count_arrives(kRows / 8 + 1, kRows);
    const uint32_t before = c.queued;
    CHECK(c.refused_in_a_row(1000) == 32);  // (the launch that ended the run was admitted: the probe)
    CHECK(c.queued == before + 1);
    for (int i = 0; i < 40; ++i) CHECK(!c.launch());
    CHECK(c.queued == before + 1);
    // the probe fails too: held off again, for 32 launches again
    c.count_arrives(kRows, kRows);
    CHECK(c.refused_in_a_row(1000) == 32);
    for (int i = 0; i < 3; ++i) CHECK(!c.launch());
    // the probe passes: open again
    c.count_arrives(1, kRows);
    CHECK(c.launch());
    CHECK(c.launch());
    CHECK(c.launch());
  }
  {  // a count of no rows judges nothing bad
    Chain c;
    CHECK(c.launch());
    c.count_arrives(0, 0);
    CHECK(c.launch());
    CHECK(c.launch());
  }
  {  // mode 2: every launch is admitted, whatever the counts say - and the last count is still recorded
    Chain c;
    c.p.set_mode(2);
    CHECK(c.launch());
    CHECK(c.launch());
    c.count_arrives(4000, kRows);
    CHECK(c.launch());
    CHECK(c.p.last_failed == 4000);
    for (int i = 0; i < 40; ++i) CHECK(c.launch());
    c.count_arrives(7, kRows);
    CHECK(c.launch());
    CHECK(c.p.last_failed == 7);
  }
  {  // a mode change clears the guard and nothing else: the kinds survive it
    Chain c;
    c.p.repair_kind = 2, c.p.bound_kind = 2, c.p.edge_kind = 3;
    CHECK(c.launch());
    c.count_arrives(kRows, kRows);
    CHECK(!c.launch());  // held off
    c.p.set_mode(0);
    CHECK(c.p.mode == 0 && c.p.repair_kind == 2 && c.p.bound_kind == 2 && c.p.edge_kind == 3);
    CHECK(c.launch());   // like a fresh context: a probe ...
    CHECK(!c.launch());  // ... and the launches behind it wait
    c.p.set_mode(1);
    c.p.set_mode(0);
    CHECK(c.p.repair_kind == 2 && c.p.bound_kind == 2 && c.p.edge_kind == 3);
  }
  {  // the repair's transform: off before any count has been read, the latency kernel up to 128 failed rows
    Chain c;
    CHECK(!c.p.latency_repair());
    CHECK(c.launch());
    CHECK(!c.p.latency_repair());  // queued, nothing read
    c.count_arrives(128, kRows);
    CHECK(c.launch());
    CHECK(c.p.latency_repair());
    c.count_arrives(129, kRows);
    CHECK(c.launch());
    CHECK(!c.p.latency_repair());
    c.count_arrives(0, kRows);
    CHECK(c.launch());
    CHECK(c.p.latency_repair());
    c.p.repair_kind = 1;
    CHECK(!c.p.latency_repair());
    c.p.repair_kind = 2;
    c.count_arrives(kRows, kRows);
    (void)c.launch();
    CHECK(c.p.latency_repair());
    ScreenPolicy fresh;
    fresh.repair_kind = 2;
    CHECK(fresh.latency_repair());
    fresh.repair_kind = 1;
    CHECK(!fresh.latency_repair());
    // the edge transform: capped unless the latency form is forced (kind 2)
    for (int k = 0; k < 4; ++k) {
      fresh.edge_kind = k;
      CHECK(fresh.edge_capped() == (k != 2));
    }
  }
  if (g_failed) std::printf("%d checks failed\n", g_failed);
  else std::printf("screen policy ok\n");
  return g_failed ? 1 : 0;
}
