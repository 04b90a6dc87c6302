// glc_resources.hpp — what a context owns (private to glc_api.hip): device and pinned buffers, streams and events
// that release themselves, the slot of an encode launch chain and the policy of the screened encode.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <utility>

#include "glc_kernels.h"

namespace glc {

// Live resources of the process (include/glc_debug.h glc_debug_live_resources): bumped where a handle is created or
// destroyed and nowhere else - never on a path that runs per launch.  Relaxed: the helper threads of glc_encode create
// handles too, and nothing is ordered by these counts.
enum LiveKind { kLiveDevBuf = 0, kLivePinnedBuf, kLiveStream, kLiveEvent, kLiveKinds };
inline std::atomic<uint64_t> g_live[kLiveKinds];
inline void live_add(LiveKind k) { g_live[k].fetch_add(1, std::memory_order_relaxed); }
inline void live_sub(LiveKind k) { g_live[k].fetch_sub(1, std::memory_order_relaxed); }

}  // namespace glc

// Device buffer that grows on demand (never shrinks while its owner lives).  reserve() frees before it allocates and
// keeps no contents.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes, glc::live_add(glc::kLiveDevBuf);
    return e;
  }
  void release() {
    if (p) (void)hipFree(p), glc::live_sub(glc::kLiveDevBuf);
    p = nullptr;
    cap = 0;
  }
};

// Pinned host staging buffer (grows on demand): device <-> host copies through it run at PCIe
// speed and truly asynchronously, which pageable memory does not give.
struct HostBuf {
  void *p = nullptr;
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(HostBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  HostBuf &operator=(HostBuf &&o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    return *this;
  }
  ~HostBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes, glc::live_add(glc::kLivePinnedBuf);
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p), glc::live_sub(glc::kLivePinnedBuf);
    p = nullptr;
    cap = 0;
  }
};

// A stream the owner creates on first use (ensure: hipStreamNonBlocking) and destroys with itself, or one it only
// borrows (the caller's, after glc_ctx_set_stream).  Reads as the handle wherever one is expected.
struct Stream {
  hipStream_t h = nullptr;
  bool owned = false;
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  ~Stream() {
    if (owned) (void)hipStreamDestroy(h), glc::live_sub(glc::kLiveStream);
  }
  hipError_t ensure() {
    if (h) return hipSuccess;
    const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    if (e == hipSuccess) owned = true, glc::live_add(glc::kLiveStream);
    return e;
  }
  void borrow(hipStream_t s) { h = s; }  // of a Stream that owns nothing
  operator hipStream_t() const { return h; }
};

// An event the owner creates on first use and destroys with itself.
struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  Event(Event &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Event &operator=(Event &&) = delete;
  ~Event() {
    if (h) (void)hipEventDestroy(h), glc::live_sub(glc::kLiveEvent);
  }
  hipError_t ensure(unsigned flags = hipEventDisableTiming) {
    if (h) return hipSuccess;
    const hipError_t e = hipEventCreateWithFlags(&h, flags);
    if (e == hipSuccess) glc::live_add(glc::kLiveEvent);
    return e;
  }
  operator hipEvent_t() const { return h; }
};

// The policy of the screened encode (glc_kernels.h launch_encode_screened): which launches take the path, which
// transform repairs them, which form of the bound and which edge transform they get, and what they have added up to.
// Plain host code: the guard is handed the counts the device left (observe), it does not read them.
struct ScreenPolicy {
  int mode = 0;         // include/glc_debug.h glc_debug_set_encode_screen
  int repair_kind = 0;  // include/glc_debug.h glc_debug_set_encode_repair
  int bound_kind = 0;   // include/glc_debug.h glc_debug_set_encode_bound
  int edge_kind = 0;    // include/glc_debug.h glc_debug_set_encode_edge
  int k1_variant = 0;   // include/glc_debug.h: which forward-transform kernel takes launches of >= 4096 rows
  bool usable = false;  // the rate's last band starts where a screen pays (encode_screen_shape)
  glc::ScreenShape shape{};
  const glc::DeviceTables *dev = nullptr;  // the context's tables: where the matrix form is built
  // the guard
  uint32_t backoff = 0;      // launches the guard still sends down today's path
  bool held = false;         // the last count read was a bad one: one probe at a time
  bool judged_any = false;   // a count has been read since the context was created (or the mode set)
  uint32_t last_failed = 0;  // ... and the failed rows of the last one read: picks the repair's transform
  // counters
  uint64_t rows_screened = 0;
  uint64_t repair_launches[2] = {0, 0};       // screened launches that took k_mdct_fwd_small_cols / k_mdct_fwd_small_rows
  uint64_t edge_launches = 0, edge_rows = 0;  // screened launches that took the edge path, and their edge rows
  uint32_t tap_rows = 0, tap_planes = 0;  // the last screened launch on slot 0: its rows and hf planes (glc_debug_encode_bound_tap)

  // A mode change clears the guard and nothing else: the kinds survive it.
  void set_mode(int m) {
    mode = m;
    backoff = 0;
    held = false;
    judged_any = false;
  }

  // Whether a launch of M rows may take the screened path at all (the mode and the launch's shape; the guard aside).
  bool may(uint32_t M, uint32_t ch) const {
    if (!usable || mode == 1) return false;
    // (forced on: from one row tile of the form the launch takes - 256 rows, 128 where the matrix form is forced too)
    if (mode == 2) return M >= (bound_kind == 2 && glc::encode_matrix_bound_built(*dev, shape, ch) ? 128u : 256u);
    return glc::mdct_forward_is_st16(M, ch, k1_variant);
  }

  // Whether a launch of M rows takes the screened path.  Automatic mode: where launch_mdct_forward would pick the
  // 16-wave kernel, unless the guard holds it off.  The guard: content that fails the screen everywhere (noise)
  // pays the fast pass AND a slow repair, so when a count a repair launch left shows more than 1 row in
  // kScreenGuardDen failed, the path is held off: the next kScreenGuardBackoff launches take today's kernels, then
  // ONE launch probes again, and until its count has come back - the host may be many launches ahead of the
  // device - nothing else is screened.  A launch that passes opens the path again.  A context that has read no count
  // yet is treated the same way: its first screened launch is its probe, and the launches queued behind it before
  // its count is back take today's kernels (a burst of noise on a fresh context pays the repair once).  What the
  // guard cannot shorten: when content turns from passing to failing, the launches queued before the first bad
  // count is back are screened and repaired - as many as the caller queues without waiting.
  // The count is a heuristic's input and nothing more: the device leaves {failed, rows, seq} as three plain
  // stores in no order, and the caller reads them without synchronising - it may see a launch's seq beside the counts
  // of the one before, or judge a launch late.  Either only moves the decision by a launch; the records are the
  // same whichever path a launch takes.
  // The same count picks the repair's transform (glc_kernels.h launch_encode_screened), in the forced mode 2 as well:
  // latency_repair below.
  // The step, for a launch that may(): observe() every slot's words as they stand - `judged` is the slot's, the seq of
  // the last count read from it - then admit(pending), pending: a slot holds a screened launch whose count is not back.
  static constexpr uint32_t kScreenGuardDen = 8, kScreenGuardBackoff = 32;
  void observe(uint32_t &judged, uint32_t seq, uint32_t failed, uint32_t rows) {
    if (seq == judged) return;
    judged = seq;
    const bool bad = rows && static_cast<uint64_t>(failed) * kScreenGuardDen > rows;
    if (bad) backoff = kScreenGuardBackoff;
    held = bad;
    judged_any = true;
    last_failed = failed;
  }
  bool admit(bool pending) {
    if (mode == 2) return true;
    if (backoff) {
      --backoff;
      return false;
    }
    return !((held || !judged_any) && pending);
  }

  // Which transform repairs a screened launch: the latency kernel when the last count the device left (read by
  // observe just before) is small, today's when it is large - and when no count has been read yet, so that a
  // fresh context on noise pays what it paid.  A heuristic like the guard: the records are the same either way.
  // kScreenRepairLatencyRows is the measured crossover (profiles/encode_repair_bench.txt section 5, 8192-row launches):
  // with the failed frames spread over the launch the latency kernel wins at every count measured, 2 .. 1024 rows; with
  // them in one run - the tile kernel's best case, a tile of 32 rows is all failed rows - it still wins at 132 failed
  // rows (by 5.8 us) and loses at 516 (by 119 us).  128 is the largest count of the sweep at which it wins either way.
  static constexpr uint32_t kScreenRepairLatencyRows = 128;
  bool latency_repair() const {
    if (repair_kind) return repair_kind == 2;
    return judged_any && last_failed <= kScreenRepairLatencyRows;
  }

  // Which edge transform a launch that takes the edge path gets (include/glc_debug.h glc_debug_set_encode_edge): the
  // capped one unless the latency form is forced.  Measured (profiles/encode_edge_bench.txt): the latency form's waves
  // do not fit beside two resident workgroups of K2 and cost K2 its single round; the capped form's do.
  bool edge_capped() const { return edge_kind != 2; }

  // Which form of the transform a screened launch of M rows takes (glc_kernels.h MatrixBound): the matrix form where
  // it is built - the rate's ne, a channel count with a segment loader - and, in the automatic mode, where the launch
  // is one the automatic screen takes at all (mdct_forward_is_st16: 3584 rows and up); the forced kind 2 takes it
  // wherever it is built, kind 1 never.
  bool matrix_bound(uint32_t M, uint32_t ch) const {
    if (bound_kind == 1 || !glc::encode_matrix_bound_built(*dev, shape, ch)) return false;
    return bound_kind == 2 || M >= 3584u;
  }

  // Bytes of the screened path's workspace for the largest launch of a range of `frames` frames in chunks of `chunk`
  // that may take the path (0: none may).
  uint64_t workspace_bytes(uint32_t ch, uint64_t frames, uint64_t chunk) const {
    const uint32_t m_full = static_cast<uint32_t>(std::min(chunk, frames) * ch);
    const uint32_t m_last = frames > chunk ? static_cast<uint32_t>(frames % chunk * ch) : 0u;
    uint64_t need = 0;
    if (may(m_full, ch)) need = glc::encode_screen_bytes(m_full, shape);
    if (m_last && may(m_last, ch)) need = std::max(need, glc::encode_screen_bytes(m_last, shape));
    return need;
  }
};

// What one encode launch chain owns.  A chain is the caller's stream (slot 0) or the context's second stream (slot 1):
// launches of one slot are in stream order, so each of these has one user at a time.
struct EncodeSlot {
  int index = 0;                // 0 / 1: which half of the context's shared words is this slot's
  DevBuf coef;                  // MDCT coefficient workspace [rows][1024]
  DevBuf screen_ws;             // the screened path's workspace: hf planes and flags (glc_kernels.h encode_screen_bytes)
  uint32_t *stat = nullptr;     // its 8 host-mapped words the repair launch leaves its count in (the context's screen_stat)
  uint32_t seq = 0, judged = 0; // launches queued / whose count the guard has read
  DevBuf edge_coef;             // the edge rows' coefficients, [kEdgeRowsMax][1024]
  unsigned long long *failed_total = nullptr;  // device: the edge rows of this slot that failed the screen so far (the context's edge_failed)
  Event ev_edge[2];             // {fork, edge rows done} of a launch's edge path

  // The screened path's workspace, reserved where the coefficient workspace is: for the largest launch of a range of
  // `frames` frames in chunks of `chunk` that may take the path.
  hipError_t reserve_screen(const ScreenPolicy &policy, uint32_t ch, uint64_t frames, uint64_t chunk) {
    const uint64_t need = policy.workspace_bytes(ch, frames, chunk);
    return need ? screen_ws.reserve(need) : hipSuccess;
  }
};
