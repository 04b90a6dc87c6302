// glc_api.hip — context, encode/decode drivers and the extern "C" surface (include/glc.h).
//
// Host-side counterpart of Encoder::new / encode (src/codec.rs:406-565) and Decoder::new /
// decode_streaming / decode (src/codec.rs:581-768).  There is no CPU compute path in this
// library: every entry point that transforms audio launches the gfx950 kernels and fails with
// GLC_ENODEV / GLC_EHIP when that is impossible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <cstdio>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <cstdlib>
#include <vector>

#include "../../include/glc_debug.h"
#include "glc_args.hpp"
#include "glc_common.h"
#include "glc_kernels.h"
#include "glc_resources.hpp"
#include "glc_rounds.hpp"
#include "glc_stages.hpp"

namespace glc {

static std::mutex g_err_mu;
static std::string g_err;

void set_global_error(const std::string &msg) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = msg;
}

}  // namespace glc

// The tables of a batch call: written into the context's pinned image (rtb_stage), sent up to rtb_tab in ONE copy with
// rtb_ev recorded behind it.  The image is shared by every such call of the context and may still be on its way up for
// the call before, so begin() waits for that copy - not for any kernel of that call, they are queued behind it - before
// the caller may write host<T>(); send() queues the copy, after which the launches may read dev<T>().  Owns nothing:
// buffers and event are the context's.
struct TableImage {
  bool pending = false;  // an upload has been queued and its event not waited for
  uint8_t *img = nullptr;
  const uint8_t *tab = nullptr;  // of the call that last began
  int begin(glc_ctx *ctx, size_t bytes);
  int send(glc_ctx *ctx, size_t bytes);
  template <typename T>
  T *host(size_t off) const { return reinterpret_cast<T *>(img + off); }
  template <typename T>
  const T *dev(size_t off) const { return reinterpret_cast<const T *>(tab + off); }
};

// Everything a context owns releases itself (glc_resources.hpp), and `delete ctx` is all glc_ctx_destroy does about
// it.  Members are destroyed in reverse order of declaration, so THE ORDER BELOW IS THE ORDER OF RELEASE, backwards:
// the helper threads stand last and are joined first, the events before them are destroyed next, then the streams,
// and the buffers are freed last - the encode slots stand among them, so a slot's two edge events go with its buffers,
// behind the side stream as they always did.  A new member goes into the group of its kind; state that owns nothing
// may stand anywhere in front of the streams.
struct glc_ctx {
  int device = 0;
  uint32_t sample_rate = 0;
  glc::HostTables host;
  glc::DeviceTables dev{};
  DevBuf tables;     // all constant tables in one allocation
  // The two encode launch chains: slot 0 goes with the caller's stream, slot 1 with `stream_b` (odd rounds / chunks).
  EncodeSlot slot[2];
  DevBuf &coef = slot[0].coef;  // slot 0's coefficient workspace, as the round trip, store, stream and batch drivers name it
  DevBuf pcm;        // staging for host-boundary encode / decode output
  DevBuf pcm_int;    // glc_encode_int / glc_encode_batch_int: the integer samples as uploaded, widened into `pcm` on the device
  DevBuf records;    // staging for host-boundary encode
  DevBuf blocks;     // decode: windowed IMDCT blocks [(chunk+1)][ch][2048]
  DevBuf dec_meta;   // decode: pairs / offsets / scales / raw pool
  DevBuf dec_plan;   // decode: union records of the (group, channel) units of one D1 launch (+ the unit order)
  uint32_t dec_plan_groups = 0;
  // the launch whose plan records dec_plan still holds: a repeated launch of the same rows of the same
  // stream skips k_imdct_plan (valid only for launches of one batch, plan_M != 0)
  uint64_t plan_uid = 0;
  uint32_t plan_row_begin = 0, plan_M = 0;
  DevBuf pack_meta;  // compaction scratch: loc, blk, blk_raw, totals
  DevBuf pack_blob;  // compaction: the compact blob of glc_encode / glc_frames_from_device_records
  HostBuf host_stage;  // pinned: the blob on its way to the host
  // round trip (glc_decode_device_records, glc_roundtrip_*): everything is sized by the round
  DevBuf rt_records;  // the round's frame records
  DevBuf rt_rows;     // the row tables R1 builds from them (glc_kernels.h rows_from_records_bytes)
  DevBuf rt_edge;     // two hops: the output hops the gapless trim cuts, before their kept part is copied on
  DevBuf rt_stats;    // counters of the stream the last round trip encoded (glc_kernels.h launch_rows_from_records)
  DevBuf rt_out;      // glc_roundtrip: the trimmed output on its way to the host
  uint64_t rt_info_frames = 0;  // frames of that stream (0: no round trip has completed)
  uint32_t rt_info_ch = 0;
  // glc_roundtrip_batch_device
  DevBuf rtb_vs;       // the virtual stream of a round / a clip longer than a round, staged whole
  DevBuf rtb_tab;      // the call's tables: per round the clip table, the frame map and the hop descriptors
  DevBuf rtb_stats;    // per-clip counters of the last batch call
  HostBuf rtb_stage;   // pinned image of rtb_tab on its way up; rtb_ev is recorded behind that copy
  TableImage rtb_image;  // the upload protocol of the two: every call that writes rtb_stage goes through it
  struct RtbClipInfo {
    uint64_t n_frames, stat_off;  // stat_off: the clip's first counter pair in rtb_stats, in uint64_t
    uint32_t stat_slots;
  };
  std::vector<RtbClipInfo> rtb_info;  // the clips of the last completed batch call (empty: none)
  uint32_t rtb_info_ch = 0;
  // glc_decode_device_compact / glc_decode_batch_device_compact
  DevBuf cd_status;         // one glc::CompactStatus per blob of the last call: what R2 found
  uint64_t cd_status_n = 0; // blobs of that call (0: none has completed)
  // glc_store_compact_device: buffers of its own, so that the call leaves every other family's state alone
  DevBuf sc_ws;             // the scan's move table (glc_kernels.h store_evict_ws_bytes)
  DevBuf sc_stage;          // in place: two staging buffers of one round each
  uint64_t sc_round = 0;    // include/glc_debug.h glc_debug_set_store_compact_round (0: kStoreCompactRound)
  HostBuf batch_stage;  // pinned: a round of glc_encode_batch's short clips going up, then its payload coming down / of glc_decode_batch's rows going up
  std::string err;
  // decode session (decode_prepare / round_launch): device-resident sparse rows + position
  glc::DecodeRows dec_rows{};
  uint64_t dec_uid = 0;  // glc_frames::uid whose rows dec_meta holds (0: none)
  // header of that stream (what glc_decode needs besides the rows) and a fingerprint of its pools: a
  // caller-supplied stream id that comes back with different counts is treated as a new stream
  uint32_t dec_delay = 0;
  uint64_t dec_orig_len = 0, dec_n_pairs = 0, dec_n_raw = 0;
  int d1_variant = 0;    // include/glc_debug.h: which inverse-transform kernel / path to launch
  // The screened encode (glc_kernels.h launch_encode_screened): its policy, and what the two slots share - the words
  // their launches report through, allocated and cleared once (ensure_screen_shared).
  ScreenPolicy policy;
  HostBuf screen_stat;             // [2][8] uint32_t, host-mapped: slot i's repair launch leaves its count in words 8 i ..
  DevBuf edge_failed;              // [2] uint64_t, zeroed once: per slot the edge rows that failed the screen so far
  DevBuf bound_tables;             // the matrix form's table image (glc_kernels.h MatrixBound), where the form is built
  HostBuf probe_out;               // include/glc_debug.h clock probe
  uint32_t dec_ch = 0;
  uint64_t dec_frames = 0, dec_next = 0;
  bool stream_open = false;  // glc_decode_stream_begin called, last chunk not yet delivered
  int stream_elem = 0;       // bytes per sample of the chunks handed out so far (4: float, 2: int16_t; 0: none yet)
  // streaming session: chunk i is copied to the host while chunk i+1 is already being decoded
  DevBuf stream_out;                           // two chunk-sized output buffers; ev_dec[b]: "kernels of the chunk in buffer b are done"
  int stream_buf = 0;                          // buffer holding the chunk the next call delivers
  uint64_t stream_frames = 0;                  // its frame count
  bool stream_last = false;                    // ... and whether it is the last one (carries the tail)
  // ---- streams: each but own_stream is opened where a call first needs it ----
  Stream own_stream;   // the context's private stream
  Stream stream;       // stream in use: own_stream's handle, or the caller's (glc_ctx_set_stream) - borrowed either way
  Stream copy_stream;  // glc_encode: uploads run ahead of the kernels on this one
  Stream stream_b;     // odd rounds / chunks of an encode are transformed here, beside the even ones on `stream`
  Stream down_stream;  // glc_encode: round i is compacted and its blob comes down while round i+1 is transformed
  Stream edge_stream;  // the edge path of a screened launch (glc_kernels.h EdgeLaunch): a side stream of the context's own - not
                       // stream_b, which the chunk alternation uses; the slot holds the events of a launch's fork and join
  Stream probe_stream; // include/glc_debug.h clock probe
  // ---- events ----
  Event ev_begin, ev_end;        // glc_ctx_timer_* (the two that keep time)
  Event ev_fork, ev_join;        // glc_encode_range_device: second stream after the caller's work, caller's stream after both
  std::vector<Event> ev_round;   // glc_encode, one per round: records written
  Event ev_dec[2];               // decode: "kernels of the chunk in buffer b are done"
  Event rtb_ev;                  // recorded behind the upload of rtb_stage: the next call waits for it before it rewrites the image
  // ---- threads ----
  Worker enc_up, enc_launch;     // the helper threads of glc_encode* and glc_roundtrip: started by the first multi-round stream
};

namespace {

constexpr uint64_t kEncodeChunkFrames = 4096;  // frames per K1/K2/K3 round: coef stays MALL-sized
// ... of at least 8192 rows: a 128 x 128-tile launch of 4096 rows is one workgroup per CU, two waves per
// SIMD (mono, k1_tune: 27.1 T MAC/s at 4096 rows, 30.8 T at 8192)
inline uint64_t encode_chunk_frames(uint32_t ch) { return ch == 1 ? 2 * kEncodeChunkFrames : kEncodeChunkFrames; }
constexpr uint64_t kDecodeChunkFrames = 4096;

constexpr uint32_t kPlanGroups = 2048;  // (group, channel) units per D1 batch: 135 MB of workspace

// glc_encode's helper threads run stages that report through fail(): they must not write ctx->err
// (one std::string, two writers) - each helper points this at a string of its own for the duration of
// its job, and the calling thread stores the winning message into ctx->err once, at the end.
thread_local std::string *t_err_sink = nullptr;
struct SinkGuard {
  std::string *prev;
  explicit SinkGuard(std::string *s) : prev(t_err_sink) { t_err_sink = s; }
  ~SinkGuard() { t_err_sink = prev; }
};

int fail(glc_ctx *ctx, int code, const std::string &msg) {
  if (t_err_sink) {
    *t_err_sink = msg;
    return code;
  }
  if (ctx) ctx->err = msg;
  glc::set_global_error(msg);
  return code;
}

int hip_fail(glc_ctx *ctx, hipError_t e, const char *what) {
  return fail(ctx, e == hipErrorOutOfMemory ? GLC_ENOMEM : GLC_EHIP,
              std::string(what) + ": " + hipGetErrorString(e));
}

#define GLC_HIP(ctx, call)                                   \
  do {                                                       \
    hipError_t e__ = (call);                                 \
    if (e__ != hipSuccess) return hip_fail(ctx, e__, #call); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// The body of a device batch, store or stream call behind its argument checks: the context's device is current while
// it runs, and no C++ exception crosses the C ABI.  `w` names the call.
template <typename Body>
int on_device(glc_ctx *ctx, const std::string &w, Body body) {
  DeviceGuard guard(ctx->device);
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return fail(ctx, GLC_ENOMEM, w + ": host allocation failed");
  }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The counters of a StageGate (glc_stages.hpp): rounds whose samples are on the device / whose records event has been recorded.
enum { kUploaded, kQueued };

// THE uploader stage of glc_encode* and glc_roundtrip: for every round i of n_rounds, what of the stream `pcm` lies
// between the mark of the round before and its own, mark_of(i) (glc::upload_mark), goes up on `st`, back to back, and
// the round is reported to the gate as `counter`.  Floats (GLC_PCM_F32) go straight into d_pcm.  Integer samples go
// up as they are, 2 or 4 bytes each, into d_int, and the round's increment is widened into d_pcm behind its copy: the
// next stage finds the same floats as after a float upload.
// host_wait: the stage waits for `st` before it reports - a copy from pageable memory has completed when the call
// returns; should the runtime ever queue it instead, this is where it is waited for (the next stage queues nothing
// behind it).  Without it the caller's kernels follow on `st` itself.  Ends early once another stage has failed or the
// consumer has stopped; a failure of its own is "<who>: upload: <hip error string>" in the gate.
template <typename MarkOf>
void upload_rounds(glc_ctx *ctx, const char *who, StageGate &gate, int counter, size_t n_rounds, MarkOf mark_of,
                   const void *pcm, glc_pcm_format fmt, uint32_t bits, float *d_pcm, uint8_t *d_int, hipStream_t st, bool host_wait) {
  DeviceGuard g(ctx->device);
  const uint8_t *h = static_cast<const uint8_t *>(pcm);
  const bool is_int = fmt != GLC_PCM_F32;
  const size_t elem = pcm_elem(fmt);
  uint64_t copied = 0;
  for (size_t i = 0; i < n_rounds; ++i) {
    const uint64_t hi = mark_of(i);
    hipError_t e = hipSuccess;
    if (hi > copied) {
      void *dst = is_int ? static_cast<void *>(d_int + copied * elem) : d_pcm + copied;
      e = hipMemcpyAsync(dst, h + copied * elem, (hi - copied) * elem, hipMemcpyHostToDevice, st);
      if (e == hipSuccess && is_int)
        e = glc::launch_pcm_widen(dst, fmt == GLC_PCM_S32, bits, hi - copied, d_pcm + copied, st);
      copied = hi;
    }
    if (e == hipSuccess && host_wait) e = hipStreamSynchronize(st);
    if (e != hipSuccess)
      return gate.set_error(e == hipErrorOutOfMemory ? GLC_ENOMEM : GLC_EHIP, std::string(who) + ": upload: " + hipGetErrorString(e));
    if (!gate.advance(counter)) return;
  }
}

}  // namespace

extern "C" {

const char *glc_last_error(const glc_ctx *ctx) {
  if (ctx) return ctx->err.c_str();
  static thread_local std::string copy;
  {
    std::lock_guard<std::mutex> lk(glc::g_err_mu);
    copy = glc::g_err;
  }
  return copy.c_str();
}

int glc_ctx_create(int device, uint32_t sample_rate, glc_ctx **out) {
  if (!out) return GLC_EINVAL;
  *out = nullptr;
  int n_dev = 0;
  hipError_t e = hipGetDeviceCount(&n_dev);
  if (e != hipSuccess || n_dev <= 0)
    return fail(nullptr, GLC_ENODEV,
                std::string("glc_ctx_create: no HIP device (") + hipGetErrorString(e) +
                    "); this library has no CPU fallback");
  if (device < 0 || device >= n_dev)
    return fail(nullptr, GLC_EINVAL, "glc_ctx_create: device index out of range");
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(nullptr, GLC_ENODEV,
                std::string("glc_ctx_create: device is ") + prop.gcnArchName +
                    ", kernels are built for gfx950 only");

  DeviceGuard guard(device);  // in front of `ctx`: a context that fails below is released with its device current
  std::unique_ptr<glc_ctx> ctx(new (std::nothrow) glc_ctx);
  if (!ctx) return GLC_ENOMEM;
  ctx->device = device;
  ctx->sample_rate = sample_rate;
  glc::build_host_tables(sample_rate, ctx->host);

  ctx->slot[1].index = 1;
  ctx->policy.dev = &ctx->dev;

  GLC_HIP(nullptr, ctx->own_stream.ensure());
  ctx->stream.borrow(ctx->own_stream);

  // one allocation, 256-B aligned sub-buffers
  const glc::HostTables &h = ctx->host;
  const size_t nb = h.edges.size() - 1;
  TableOffsets offs;
  const size_t o_cos_t = offs.take(h.cos_table_t.size() * 4);
  const size_t o_cos = offs.take(h.cos_table.size() * 4);
  const size_t o_win = offs.take(h.window.size() * 4);
  const size_t o_indiv = offs.take(h.indiv.size() * 4);
  const size_t o_pf = offs.take(64 * 4);
  const size_t o_len = offs.take(64 * 4);
  const size_t o_bof = offs.take(h.band_of.size() * 2);
  const size_t o_edges = offs.take(65 * 4);
  e = ctx->tables.reserve(offs.size());
  if (e != hipSuccess) return hip_fail(nullptr, e, "hipMalloc(tables)");
  uint8_t *base = static_cast<uint8_t *>(ctx->tables.p);
  auto up = [&](size_t o, const void *src, size_t bytes) {
    return hipMemcpy(base + o, src, bytes, hipMemcpyHostToDevice);
  };
  std::vector<float> pf(64, 0.f), len(64, 1.f);
  std::vector<uint32_t> edges(65, glc::kHop);
  std::copy(h.band_pf.begin(), h.band_pf.end(), pf.begin());
  std::copy(h.band_len.begin(), h.band_len.end(), len.begin());
  std::copy(h.edges.begin(), h.edges.end(), edges.begin());
  hipError_t es[8] = {up(o_cos_t, h.cos_table_t.data(), h.cos_table_t.size() * 4),
                      up(o_cos, h.cos_table.data(), h.cos_table.size() * 4),
                      up(o_win, h.window.data(), h.window.size() * 4),
                      up(o_indiv, h.indiv.data(), h.indiv.size() * 4),
                      up(o_pf, pf.data(), 64 * 4),
                      up(o_len, len.data(), 64 * 4),
                      up(o_bof, h.band_of.data(), h.band_of.size() * 2),
                      up(o_edges, edges.data(), 65 * 4)};
  for (hipError_t x : es)
    if (x != hipSuccess) return hip_fail(nullptr, x, "hipMemcpy(tables)");
  glc::DeviceTables &d = ctx->dev;
  d.cos_t = reinterpret_cast<const float *>(base + o_cos_t);
  d.cos = reinterpret_cast<const float *>(base + o_cos);
  d.window = reinterpret_cast<const float *>(base + o_win);
  d.indiv = reinterpret_cast<const float *>(base + o_indiv);
  d.band_pf = reinterpret_cast<const float *>(base + o_pf);
  d.band_len = reinterpret_cast<const float *>(base + o_len);
  d.band_of = reinterpret_cast<const uint16_t *>(base + o_bof);
  d.edges = reinterpret_cast<const uint32_t *>(base + o_edges);
  d.n_bands = static_cast<uint32_t>(nb);
  d.norm = h.norm;
  d.cf = h.cf;
  d.noise_floor = h.noise_floor;
  ScreenPolicy &pol = ctx->policy;
  pol.usable = glc::encode_screen_shape(h.edges.data(), static_cast<uint32_t>(nb), &pol.shape);
  d.cos_bf = nullptr;
  if (pol.usable && pol.shape.ne == static_cast<uint32_t>(glc::MatrixBound::kNe)) {
    // the bf16 pieces of the bound columns depend on the rate's C0 alone: built and uploaded once per context
    std::vector<uint16_t> img;
    glc::build_bound_table_image(h, pol.shape.c0, img);
    e = ctx->bound_tables.reserve(img.size() * 2);
    if (e == hipSuccess) e = hipMemcpy(ctx->bound_tables.p, img.data(), img.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipMemcpy(bound tables)");
    d.cos_bf = static_cast<const uint16_t *>(ctx->bound_tables.p);
  }
  *out = ctx.release();
  return GLC_OK;
}

void glc_ctx_destroy(glc_ctx *ctx) {
  if (!ctx) return;
  DeviceGuard guard(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx;  // the helper threads are idle (glc_encode waits for them before it returns); the members' order does the rest
}

void *glc_ctx_stream(glc_ctx *ctx) { return ctx ? static_cast<hipStream_t>(ctx->stream) : nullptr; }
int glc_ctx_device(const glc_ctx *ctx) { return ctx ? ctx->device : -1; }

int glc_ctx_set_stream(glc_ctx *ctx, void *hip_stream) {
  if (!ctx) return GLC_EINVAL;
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream.borrow(hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream);
  return GLC_OK;
}

int glc_ctx_synchronize(glc_ctx *ctx) {
  if (!ctx) return GLC_EINVAL;
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GLC_OK;
}

int glc_ctx_timer_begin(glc_ctx *ctx) {
  if (!ctx) return GLC_EINVAL;
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, ctx->ev_begin.ensure(hipEventDefault));
  GLC_HIP(ctx, ctx->ev_end.ensure(hipEventDefault));
  GLC_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
  return GLC_OK;
}

int glc_ctx_timer_end(glc_ctx *ctx, float *elapsed_ms) {
  if (!ctx || !elapsed_ms || !ctx->ev_begin) return fail(ctx, GLC_EINVAL, "glc_ctx_timer_end: no timer running");
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
  GLC_HIP(ctx, hipEventSynchronize(ctx->ev_end));
  GLC_HIP(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev_begin, ctx->ev_end));
  return GLC_OK;
}

int glc_ctx_tables(const glc_ctx *ctx, float *cos_table, float *window, float *norm,
                   float *weights, uint32_t *band_edges, uint32_t *n_edges) {
  if (!ctx) return GLC_EINVAL;
  const glc::HostTables &h = ctx->host;
  if (cos_table) std::memcpy(cos_table, h.cos_table.data(), h.cos_table.size() * 4);
  if (window) std::memcpy(window, h.window.data(), h.window.size() * 4);
  if (norm) *norm = h.norm;
  if (weights) std::memcpy(weights, h.weights.data(), h.weights.size() * 4);
  if (band_edges) std::memcpy(band_edges, h.edges.data(), h.edges.size() * 4);
  if (n_edges) *n_edges = static_cast<uint32_t>(h.edges.size());
  return GLC_OK;
}

// ------------------------------------------------------------------------------ encode

// A frame-range encode: frames [frame_begin, frame_end) of the stream `view` shows (whole, or a shard with halo) ->
// their records.
struct EncodeRange {
  glc::PcmView view;
  uint64_t frame_begin, frame_end;
  void *records;
  float *coef_tap;   // optional: the range's coefficients go here, in one launch, instead of into the slot's workspace
  EncodeSlot *slot;  // the launch chain the range is queued on (null where nothing is transformed)
};
// What a caller of encode_range_on allows the range:
enum : unsigned {
  kEncodeAlternate = 1u,  // a range of several chunks may alternate between the given stream and stream_b (slot 1)
  kEncodeBeside = 2u,     // the launch runs beside others: launch_mdct_forward deals its rows accordingly
  kEncodeEdge = 4u,       // the caller owns its stream's order: a screened chunk may hand its edge frames to the side stream
};

// Arguments of a frame-range encode (glc_encode_range_device, glc_debug_quantize_device): `fn` names the
// entry point in the error message.  `whole_tap`: the range's rows go into one caller-supplied coefficient
// buffer, so their count must fit one launch.
static int check_encode_range(glc_ctx *ctx, const char *fn, const EncodeRange &r, bool whole_tap) {
  const std::string f(fn);
  const uint64_t t0 = r.view.t0, t_count = r.view.t_count, frame_begin = r.frame_begin, frame_end = r.frame_end;
  const uint16_t channels = static_cast<uint16_t>(r.view.ch);
  if (!ctx || !r.view.p || !r.records) return fail(ctx, GLC_EINVAL, f + ": null argument");
  const glc_plan plan = glc::plan_encode(r.view.n_samples, channels);
  if (plan.n_frames == 0)
    return fail(ctx, GLC_EINVAL, f + ": the reference encoder panics on this input");
  if (frame_begin > frame_end || frame_end > plan.n_frames)
    return fail(ctx, GLC_EINVAL, f + ": frame range out of bounds");
  if (whole_tap && (frame_end - frame_begin) * channels > 0xFFFFFFFFull)
    return fail(ctx, GLC_EINVAL, f + ": range too large for one coefficient tap");
  // The shard must hold every real sample the frame range reads.
  if (frame_end > frame_begin) {
    const glc::SampleWindow need = glc::frame_sample_window(frame_begin, frame_end, plan.per_channel);
    if (need.hi > need.lo && (t0 > need.lo || t0 + t_count < need.hi))
      return fail(ctx, GLC_EINVAL, f + ": PCM shard does not cover the frame range (halo missing)");
  }
  return GLC_OK;
}

// K2, then K3 for the channel counts whose raw-vs-compressed decision K2 does not take itself, on the
// coefficient rows of frames [frame_begin, frame_begin + n_frames) -> their records.
static hipError_t launch_quantize_decide(glc_ctx *ctx, const float *coef, const glc::PcmView &view,
                                         uint64_t frame_begin, uint64_t n_frames, uint8_t *records, hipStream_t st) {
  bool decided = false;
  hipError_t e = glc::launch_quantize(ctx->dev, coef, static_cast<uint32_t>(n_frames * view.ch), view.ch, view,
                                      frame_begin, records, st, &decided);
  if (e == hipSuccess && !decided)
    e = glc::launch_decide_raw(ctx->dev, view, frame_begin, static_cast<uint32_t>(n_frames), records, st);
  return e;
}

// What the two slots' screened launches share, allocated and cleared once per context, in front of the first
// workspace a slot reserves: the host-mapped words and the edge path's running totals.
static hipError_t ensure_screen_shared(glc_ctx *ctx) {
  if (!ctx->screen_stat.p) {
    const hipError_t e = ctx->screen_stat.reserve(2 * 8 * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    std::memset(ctx->screen_stat.p, 0, 2 * 8 * sizeof(uint32_t));
  }
  if (!ctx->edge_failed.p) {
    // the edge path's running total, cleared where it is allocated - beside the workspaces, before any launch is
    // queued - and waited for here, since the streams that will use it do not order themselves behind this one
    hipError_t e = ctx->edge_failed.reserve(2 * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(ctx->edge_failed.p, 0, 2 * sizeof(uint64_t));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return e;
  }
  for (EncodeSlot &s : ctx->slot) {
    s.stat = static_cast<uint32_t *>(ctx->screen_stat.p) + 8 * s.index;
    s.failed_total = static_cast<unsigned long long *>(ctx->edge_failed.p) + s.index;
  }
  return hipSuccess;
}

// A slot's workspaces for a range of `frames` frames in chunks of `chunk`: the coefficients of its largest launch
// and, where one of its launches may take the screened path, that path's workspace and the shared words.  The one
// place that reserves for a launch: screen_takes below decides from the same policy and the same launch shapes.
static hipError_t reserve_slot(glc_ctx *ctx, EncodeSlot &slot, uint32_t ch, uint64_t frames, uint64_t chunk) {
  const uint64_t rows = std::min<uint64_t>(chunk, frames) * ch;
  hipError_t e = slot.coef.reserve(std::max<size_t>(rows, 1) * glc::kHop * sizeof(float));
  if (e == hipSuccess && ctx->policy.workspace_bytes(ch, frames, chunk)) e = ensure_screen_shared(ctx);
  if (e == hipSuccess) e = slot.reserve_screen(ctx->policy, ch, frames, chunk);
  return e;
}

// Whether a launch of M rows takes the screened path (ScreenPolicy): the guard's step, fed the words the slots'
// repair launches left - plain loads of host-mapped memory, not synchronised.
static bool screen_takes(glc_ctx *ctx, uint32_t M, uint32_t ch) {
  ScreenPolicy &pol = ctx->policy;
  if (!pol.may(M, ch)) return false;
  bool pending = false;  // a screened launch whose count has not come back
  for (EncodeSlot &s : ctx->slot) {
    const volatile uint32_t *hs = s.stat;
    const uint32_t seq = hs[2], failed = hs[0], rows = hs[1];
    pol.observe(s.judged, seq, failed, rows);
    pending = pending || seq != s.seq;
  }
  return pol.admit(pending);
}

// glc_encode_range_device on a given stream and slot (glc_encode runs alternate rounds on two streams)
static int encode_range_on(glc_ctx *ctx, hipStream_t stream, const EncodeRange &r, unsigned flags = 0) {
  const int rc = check_encode_range(ctx, "glc_encode_range_device", r, r.coef_tap != nullptr);
  if (rc != GLC_OK) return rc;
  const glc::PcmView &view = r.view;
  const uint32_t ch = view.ch;
  const uint64_t frame_begin = r.frame_begin, frame_end = r.frame_end;
  float *const d_coeffs = r.coef_tap;
  ScreenPolicy &pol = ctx->policy;
  DeviceGuard guard(ctx->device);
  const uint64_t rec = glc::record_bytes(ch);
  uint8_t *recs = static_cast<uint8_t *>(r.records);
  const uint64_t chunk = d_coeffs ? (frame_end - frame_begin ? frame_end - frame_begin : 1) : encode_chunk_frames(ch);
  if (!d_coeffs) GLC_HIP(ctx, reserve_slot(ctx, *r.slot, ch, frame_end - frame_begin, chunk));
  // A range of several chunks alternates between the caller's stream and a second one (its own
  // coefficient workspace): chunk c's quantiser then runs beside chunk c+1's transform instead of in
  // front of it (six 4096-frame chunks: 3.78 -> 3.68 ms).  Fork and join by events, so the caller sees
  // plain stream order: everything queued before the call is finished before the second stream
  // starts, and the caller's stream continues only when both are done.
  const bool alternate = (flags & kEncodeAlternate) && !d_coeffs && frame_end - frame_begin > chunk;
  if (alternate) {
    GLC_HIP(ctx, ctx->stream_b.ensure());
    GLC_HIP(ctx, ctx->ev_fork.ensure());
    GLC_HIP(ctx, ctx->ev_join.ensure());
    GLC_HIP(ctx, reserve_slot(ctx, ctx->slot[1], ch, frame_end - frame_begin, chunk));
    GLC_HIP(ctx, hipEventRecord(ctx->ev_fork, stream));
    GLC_HIP(ctx, hipStreamWaitEvent(ctx->stream_b, ctx->ev_fork, 0));
  }
  // The stream's edge frames (glc_kernels.h edge_frames): a screened chunk that holds some hands them to the side
  // stream.  Only the call that owns its stream's order does (kEncodeEdge): the drivers pass no edge range.
  const glc_plan plan = glc::plan_encode(view.n_samples, static_cast<uint16_t>(ch));
  const glc::EdgeFrames ef = glc::edge_frames(plan.per_channel, plan.n_frames);
  uint64_t c_idx = 0;
  for (uint64_t f = frame_begin; f < frame_end; f += chunk, ++c_idx) {
    const uint64_t nf = std::min<uint64_t>(chunk, frame_end - f);
    const uint32_t M = static_cast<uint32_t>(nf * ch);
    const bool odd = alternate && (c_idx & 1);
    hipStream_t st = odd ? ctx->stream_b : stream;
    uint8_t *rp = recs + (f - frame_begin) * rec;
    EncodeSlot &slot = odd ? ctx->slot[1] : *r.slot;
    float *coef = d_coeffs ? d_coeffs + (f - frame_begin) * ch * glc::kHop : static_cast<float *>(slot.coef.p);
    if (!d_coeffs && screen_takes(ctx, M, ch)) {
      if (slot.screen_ws.cap < glc::encode_screen_bytes(M, pol.shape))
        return fail(ctx, GLC_EINVAL, "glc_encode_range_device: the screen's workspace was not reserved for this launch");
      bool decided = false;
      glc::ScreenLaunch sl{slot.screen_ws.p, slot.stat, 0, rp, st, pol.latency_repair(), pol.matrix_bound(M, ch), nullptr};
      if (slot.index == 0) pol.tap_rows = M, pol.tap_planes = sl.matrix_bound ? glc::MatrixBound::kGroups : pol.shape.n_planes;
      glc::EdgeLaunch edge{ef.a, ef.b, nullptr, nullptr, nullptr, nullptr, false, nullptr};
      const uint32_t n_edge = glc::edge_rows(ef.a, ef.b, f, M, ch).n;
      if ((flags & kEncodeEdge) && pol.edge_kind != 1 && n_edge >= 1 && n_edge <= glc::kEdgeRowsMax) {
        GLC_HIP(ctx, ctx->edge_stream.ensure());
        for (Event &ev : slot.ev_edge) GLC_HIP(ctx, ev.ensure());
        GLC_HIP(ctx, slot.edge_coef.reserve(static_cast<size_t>(glc::kEdgeRowsMax) * glc::kHop * sizeof(float)));
        edge.side = ctx->edge_stream;
        edge.ev_fork = slot.ev_edge[0], edge.ev_edge = slot.ev_edge[1];
        edge.coef = static_cast<float *>(slot.edge_coef.p);
        edge.capped = pol.edge_capped();
        edge.failed_total = slot.failed_total;
        ++pol.edge_launches;
        pol.edge_rows += n_edge;
        sl.edge = &edge;
      }
      sl.seq = ++slot.seq;
      GLC_HIP(ctx, glc::launch_encode_screened(ctx->dev, pol.shape, view, f, M, coef, sl, &decided));
      ++pol.repair_launches[sl.latency_repair ? 1 : 0];
      if (!decided) GLC_HIP(ctx, glc::launch_decide_raw(ctx->dev, view, f, static_cast<uint32_t>(nf), rp, st));
      pol.rows_screened += M;
      continue;
    }
    GLC_HIP(ctx, glc::launch_mdct_forward(ctx->dev, view, f, M, coef, st, pol.k1_variant, (flags & kEncodeBeside) != 0));
    GLC_HIP(ctx, launch_quantize_decide(ctx, coef, view, f, nf, rp, st));
  }
  if (alternate) {
    GLC_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->stream_b));
    GLC_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_join, 0));
  }
  return GLC_OK;
}

int glc_encode_range_device(glc_ctx *ctx, const float *d_pcm, uint64_t t0, uint64_t t_count,
                            uint64_t n_samples, uint16_t channels, uint64_t frame_begin,
                            uint64_t frame_end, void *d_records, float *d_coeffs) {
  if (!ctx) return GLC_EINVAL;
  const EncodeRange r{{d_pcm, t0, t_count, n_samples, channels}, frame_begin, frame_end, d_records, d_coeffs, &ctx->slot[0]};
  return encode_range_on(ctx, ctx->stream, r, kEncodeAlternate | kEncodeEdge);
}

int glc_debug_quantize_device(glc_ctx *ctx, const float *d_coeffs, const float *d_pcm, uint64_t t0, uint64_t t_count,
                              uint64_t n_samples, uint16_t channels, uint64_t frame_begin, uint64_t frame_end,
                              void *d_records) {
  if (!ctx) return GLC_EINVAL;
  if (!d_coeffs) return fail(ctx, GLC_EINVAL, "glc_debug_quantize_device: null argument");
  const glc::PcmView view{d_pcm, t0, t_count, n_samples, channels};
  const int rc = check_encode_range(ctx, "glc_debug_quantize_device", EncodeRange{view, frame_begin, frame_end, d_records, nullptr, nullptr},
                                    /*whole_tap=*/true);
  if (rc != GLC_OK) return rc;
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, launch_quantize_decide(ctx, d_coeffs, view, frame_begin, frame_end - frame_begin,
                                      static_cast<uint8_t *>(d_records), ctx->stream));
  return GLC_OK;
}

int glc_mdct_forward_device(glc_ctx *ctx, const float *d_pcm, uint64_t t0, uint64_t t_count,
                            uint64_t n_samples, uint16_t channels, uint64_t frame_begin,
                            uint64_t frame_end, float *d_coeffs) {
  if (!ctx || !d_pcm || !d_coeffs) return fail(ctx, GLC_EINVAL, "glc_mdct_forward_device: null argument");
  const glc_plan plan = glc::plan_encode(n_samples, channels);
  if (plan.n_frames == 0 || frame_begin > frame_end || frame_end > plan.n_frames)
    return fail(ctx, GLC_EINVAL, "glc_mdct_forward_device: bad stream length or frame range");
  const uint64_t rows = (frame_end - frame_begin) * channels;
  if (rows > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, "glc_mdct_forward_device: range too large");
  DeviceGuard guard(ctx->device);
  glc::PcmView view{d_pcm, t0, t_count, n_samples, channels};
  GLC_HIP(ctx, glc::launch_mdct_forward(ctx->dev, view, frame_begin, static_cast<uint32_t>(rows), d_coeffs,
                                        ctx->stream, ctx->policy.k1_variant));
  return GLC_OK;
}

// Queue the compaction of `n_frames` records into `d_blob` (capacity checked by the caller) on
// the context's stream; nothing is synchronised.
static int compact_launch(glc_ctx *ctx, const void *d_records, uint64_t n_frames, uint32_t ch, void *d_blob,
                          hipStream_t stream) {
  const uint64_t M = n_frames * ch;
  if (M > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, "compaction: frame range too long");
  const glc::CompactLayout l = glc::compact_layout(ch, n_frames);
  GLC_HIP(ctx, ctx->pack_meta.reserve(glc::compact_scratch_bytes(M)));
  uint8_t *blob = static_cast<uint8_t *>(d_blob);
  GLC_HIP(ctx, hipMemsetAsync(blob, 0, l.o_pairs, stream));  // header + section padding: deterministic bytes
  GLC_HIP(ctx, glc::launch_compact(static_cast<const uint8_t *>(d_records), static_cast<uint32_t>(M), ch, n_frames,
                                   ctx->pack_meta.p, blob, l, nullptr, nullptr, stream));
  return GLC_OK;
}

int glc_compact_device_records(glc_ctx *ctx, const void *d_records, uint64_t n_frames, uint16_t channels,
                               void *d_blob, uint64_t cap, glc_compact_info *info) {
  if (!ctx || !d_blob || !info || (!d_records && n_frames)) return fail(ctx, GLC_EINVAL, "glc_compact_device_records: null argument");
  if (channels == 0) return fail(ctx, GLC_EINVAL, "glc_compact_device_records: channels == 0");
  // the kernels read rows as short4 and write the header as 64-bit words (include/glc.h)
  if (!all_aligned(8, d_records, d_blob))
    return fail(ctx, GLC_EINVAL, "glc_compact_device_records: d_records and d_blob must be 8-byte aligned");
  const glc::CompactLayout l = glc::compact_layout(channels, n_frames);
  if (cap < l.bound) return fail(ctx, GLC_EINVAL, "glc_compact_device_records: blob buffer smaller than glc_compact_bound()");
  DeviceGuard guard(ctx->device);
  int rc = compact_launch(ctx, d_records, n_frames, channels, d_blob, ctx->stream);
  if (rc != GLC_OK) return rc;
  glc::CompactHeader h;
  GLC_HIP(ctx, hipMemcpyAsync(&h, d_blob, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (const char *bad = glc::compact_header_error(h, channels, n_frames, /*exact=*/true, l.bound))
    return fail(ctx, GLC_EHIP, std::string("glc_compact_device_records: the device wrote an inconsistent header (") + bad + ")");
  info->n_frames = h.n_frames;
  info->n_pairs = h.n_pairs;
  info->n_raw_rows = h.n_raw_rows;
  info->bytes = h.bytes;
  return GLC_OK;
}

// Compacts the records of frames [f_at, f_at + nf) into `d_blob` on `st` and lands the blob in F: its
// pairs at p_at and raw planes at r_at of the pools (grown to fit), its index vectors from frame f_at on.
// Only the bitstream's payload crosses PCIe, and it lands where it stays: the (u16, i16) pairs and the
// raw planes are copied straight into the pools, the small per-frame / per-row metadata through the
// pinned host_stage (which holds at least the metadata).  `drain(st)` blocks until `st` has drained (a
// hooked encode hands out finished frames meanwhile).  `expect_pairs`: pairs the blob is expected to
// hold; `reserve_scale` > 0: the pools are reserved for that many times this blob's payload first.
// *n_pairs / *n_raw: what the blob added to the pools.  May throw std::bad_alloc.
static int land_blob(glc_ctx *ctx, const char *who, glc_frames *F, const void *d_records, uint64_t nf, uint8_t *d_blob,
                     uint64_t f_at, uint64_t p_at, uint64_t r_at, uint64_t expect_pairs, double reserve_scale, hipStream_t st,
                     const std::function<hipError_t(hipStream_t)> &drain, uint64_t *n_pairs, uint64_t *n_raw) {
  const uint32_t ch = F->channels;
  const glc::CompactLayout l = glc::compact_layout(ch, nf);
  uint8_t *hm = static_cast<uint8_t *>(ctx->host_stage.p);
  const int crc = compact_launch(ctx, d_records, nf, ch, d_blob, st);
  if (crc != GLC_OK) return crc;
  // One copy fetches the metadata (header, raw flags, scale factors, list lengths: they say how
  // long the payload is) AND as much of the pair section behind it as this round is expected to
  // fill, into pinned memory; a round that holds more, or raw planes, fetches the rest straight into
  // the pools once the header is known.  That is for short rounds, where the second round trip is
  // what costs; a long round's payload (3.7 MB for 4096 stereo frames) goes straight into the pools -
  // the host copy out of the pinned buffer would cost more than the round trip (one hour of stereo:
  // 61 ms with it, 54 without).
  // (Queueing the last round's compaction and download behind its quantiser on the round's own
  // stream, to save the launch latency, measured 70 us SLOWER at config 2.)
  if (expect_pairs * 4 > (size_t(3) << 19)) expect_pairs = 0;
  const uint64_t first_bytes = std::min<uint64_t>({l.o_pairs + expect_pairs * 4, l.bound, ctx->host_stage.cap});
  hipError_t e = hipMemcpyAsync(hm, d_blob, first_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = drain(st);
  if (e != hipSuccess) return hip_fail(ctx, e, (std::string(who) + ": download").c_str());
  glc::CompactHeader h;
  std::memcpy(&h, hm, sizeof h);
  if (const char *bad = glc::compact_header_error(h, ch, nf, /*exact=*/true, l.bound))
    return fail(ctx, GLC_EHIP, std::string(who) + ": the device wrote an inconsistent compact header (" + bad + ")");
  if (reserve_scale > 0) {
    F->pairs.reserve(static_cast<size_t>(static_cast<double>(h.n_pairs) * reserve_scale) + 4096);
    if (h.n_raw_rows) F->raw.reserve(static_cast<size_t>(static_cast<double>(h.n_raw_rows * glc::kFrame) * reserve_scale));
  }
  *n_pairs = h.n_pairs;
  *n_raw = h.n_raw_rows * glc::kFrame;
  if (F->pairs.size() < p_at + *n_pairs) F->pairs.resize(p_at + *n_pairs);
  if (F->raw.size() < r_at + *n_raw) F->raw.resize(r_at + *n_raw);
  const uint64_t have = std::min<uint64_t>(h.n_pairs, (first_bytes - l.o_pairs) / 4);  // pairs already on the host
  if (h.n_pairs > have)
    e = hipMemcpyAsync(F->pairs.data() + p_at + have, d_blob + l.o_pairs + have * 4, (h.n_pairs - have) * 4,
                       hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && h.n_raw_rows)
    e = hipMemcpyAsync(F->raw.data() + r_at, d_blob + glc::compact_raw_offset(l, h.n_pairs), *n_raw * 2,
                       hipMemcpyDeviceToHost, st);
  if (have) std::memcpy(F->pairs.data() + p_at, hm + l.o_pairs, have * 4);
  bool canonical = true;
  int rc = GLC_OK;
  if (e == hipSuccess) rc = glc::index_compact_meta(F, ch, h, hm, f_at, p_at, r_at, /*trusted=*/true, &canonical);
  // the pools may move when they grow next, and host_stage is reused: all of it has to have landed
  if (h.n_pairs > have || h.n_raw_rows) {
    const hipError_t e2 = drain(st);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return hip_fail(ctx, e, (std::string(who) + ": download").c_str());
  if (rc != GLC_OK) return fail(ctx, rc, std::string(who) + ": " + glc_last_error(nullptr));
  return GLC_OK;
}

int glc_frames_from_device_records(glc_ctx *ctx, const void *d_records, uint64_t n_frames,
                                   uint64_t n_samples, uint16_t channels, glc_frames **out) {
  if (!ctx || !d_records || !out) return fail(ctx, GLC_EINVAL, "glc_frames_from_device_records: null argument");
  *out = nullptr;
  const glc_plan plan = glc::plan_encode(n_samples, channels);
  if (plan.n_frames == 0 || plan.n_frames != n_frames)
    return fail(ctx, GLC_EINVAL, "glc_frames_from_device_records: record count does not match the stream length");
  DeviceGuard guard(ctx->device);
  const glc::CompactLayout l = glc::compact_layout(channels, n_frames);
  GLC_HIP(ctx, ctx->pack_blob.reserve(l.bound));
  GLC_HIP(ctx, ctx->host_stage.reserve(l.o_pairs));
  std::unique_ptr<glc_frames> F(new (std::nothrow) glc_frames);
  if (!F) return fail(ctx, GLC_ENOMEM, "glc_frames_from_device_records: host allocation failed");
  int rc;
  try {
    glc::init_frames(F.get(), ctx->sample_rate, n_samples, channels, plan);
    uint64_t n_pairs, n_raw;
    rc = land_blob(ctx, "glc_frames_from_device_records", F.get(), d_records, n_frames, static_cast<uint8_t *>(ctx->pack_blob.p),
                   0, 0, 0, /*expect_pairs=*/0, /*reserve_scale=*/0, ctx->stream, hipStreamSynchronize, &n_pairs, &n_raw);
  } catch (const std::bad_alloc &) {
    rc = fail(ctx, GLC_ENOMEM, "glc_frames_from_device_records: host allocation failed");
  }
  if (rc != GLC_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing may still be in flight into F's pools
    return rc;
  }
  F->lists_canonical = true;  // ballot-packed in ascending k
  *out = F.release();
  return GLC_OK;
}

int glc_encode(glc_ctx *ctx, const float *pcm, uint64_t n_samples, uint16_t channels,
               glc_frames **out) {
  if (!out) return fail(ctx, GLC_EINVAL, "glc_encode: null argument");
  return glc_encode_hooked(ctx, pcm, n_samples, channels, nullptr, nullptr, out);
}

// The host-boundary encode of glc_encode / glc_encode_hooked (fmt == GLC_PCM_F32: `pcm` are floats) and
// of glc_encode_int (int16_t / int32_t samples of `bits` bits, widened on the device as they arrive).
static int encode_pipeline(glc_ctx *ctx, const void *pcm_any, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples,
                           uint16_t channels, glc_frames_hook hook, void *hook_user, glc_frames **out);

int glc_encode_hooked(glc_ctx *ctx, const float *pcm, uint64_t n_samples, uint16_t channels,
                      glc_frames_hook hook, void *hook_user, glc_frames **out) {
  return encode_pipeline(ctx, pcm, GLC_PCM_F32, 32, n_samples, channels, hook, hook_user, out);
}

int glc_encode_int(glc_ctx *ctx, const void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples,
                   uint16_t channels, glc_frames **out) {
  if (!ctx || !pcm || !out) return fail(ctx, GLC_EINVAL, "glc_encode_int: null argument");
  *out = nullptr;
  if (fmt == GLC_PCM_F32) return glc_encode(ctx, static_cast<const float *>(pcm), n_samples, channels, out);
  if (fmt != GLC_PCM_S16 && fmt != GLC_PCM_S32) return fail(ctx, GLC_EINVAL, "glc_encode_int: unknown sample format");
  if (bits == 0 || bits > (fmt == GLC_PCM_S16 ? 16u : 32u))
    return fail(ctx, GLC_EINVAL, "glc_encode_int: bits must be 1..16 for 16-bit samples, 1..32 for 32-bit ones");
  return encode_pipeline(ctx, pcm, fmt, bits, n_samples, channels, nullptr, nullptr, out);
}

int glc_pcm_widen_device(glc_ctx *ctx, const void *d_in, glc_pcm_format fmt, uint32_t bits, uint64_t n, float *d_out) {
  if (!ctx || ((!d_in || !d_out) && n)) return fail(ctx, GLC_EINVAL, "glc_pcm_widen_device: null argument");
  if (const char *bad = fmt_fault(fmt, bits)) return fail(ctx, GLC_EINVAL, std::string("glc_pcm_widen_device: ") + bad);
  if (n && (!aligned(d_in, pcm_elem(fmt)) || !aligned(d_out, sizeof(float))))
    return fail(ctx, GLC_EINVAL, "glc_pcm_widen_device: a pointer is not aligned to its sample size");
  if (n == 0) return GLC_OK;
  DeviceGuard guard(ctx->device);
  if (fmt == GLC_PCM_F32) {
    if (d_in != d_out) GLC_HIP(ctx, hipMemcpyAsync(d_out, d_in, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return GLC_OK;
  }
  GLC_HIP(ctx, glc::launch_pcm_widen(d_in, fmt == GLC_PCM_S32, bits, n, d_out, ctx->stream));
  return GLC_OK;
}

static int encode_pipeline(glc_ctx *ctx, const void *pcm_any, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples,
                           uint16_t channels, glc_frames_hook hook, void *hook_user, glc_frames **out) {
  if (!ctx || !pcm_any || (!out && !hook)) return fail(ctx, GLC_EINVAL, "glc_encode: null argument");
  const bool is_int = fmt != GLC_PCM_F32;
  if (out) *out = nullptr;
  const glc_plan plan = glc::plan_encode(n_samples, channels);
  if (plan.n_frames == 0)
    return fail(ctx, GLC_EINVAL,
                "glc_encode: the reference encoder panics on this input (channels == 0, <= 512 "
                "samples per channel, or ragged channels)");
  DeviceGuard guard(ctx->device);
  const uint32_t ch = channels;
  const uint64_t rec = glc::record_bytes(ch);
  const uint64_t t_count = (n_samples + ch - 1) / ch;
  // the rounds of the stream (glc_rounds.hpp), where each round's blob lands and what must be up before it runs
  struct Round {
    uint64_t f0, nf, blob_off, hi;  // hi: its upload mark
    glc::CompactLayout l;
  };
  std::vector<Round> rounds;
  std::unique_ptr<glc_frames> F;
  uint64_t max_nf = 0;
  try {
    uint64_t blob_off = 0;
    for (const StreamRound &sr : encode_stream_rounds(plan.n_frames, ch, encode_chunk_frames(ch))) {
      Round r{sr.f0, sr.nf, blob_off, glc::upload_mark(sr.f0, sr.nf, plan.per_channel, ch, n_samples), glc::compact_layout(ch, sr.nf)};
      blob_off += align_up(r.l.bound, 256);
      max_nf = std::max(max_nf, sr.nf);
      rounds.push_back(r);
    }
    F.reset(new glc_frames);
    glc::init_frames(F.get(), ctx->sample_rate, n_samples, channels, plan);
  } catch (const std::bad_alloc &) {
    return fail(ctx, GLC_ENOMEM, "glc_encode: host allocation failed");
  }
  const size_t n_rounds = rounds.size();
  // pinned landing zone of a round's blob: metadata + its expected pairs (at most the whole blob, at most 64 MiB)
  const size_t stage_cap = std::max<size_t>(std::min<size_t>(align_up(glc::compact_layout(ch, max_nf).bound, 256), size_t(64) << 20),
                                            align_up(glc::compact_layout(ch, max_nf).o_pairs, 256));
  GLC_HIP(ctx, ctx->pcm.reserve(static_cast<size_t>(t_count) * ch * sizeof(float)));
  if (is_int) GLC_HIP(ctx, ctx->pcm_int.reserve(static_cast<size_t>(t_count) * ch * pcm_elem(fmt)));
  GLC_HIP(ctx, ctx->records.reserve(static_cast<size_t>(plan.n_frames) * rec));
  GLC_HIP(ctx, ctx->pack_blob.reserve(rounds.back().blob_off + align_up(rounds.back().l.bound, 256)));
  GLC_HIP(ctx, ctx->host_stage.reserve(stage_cap));
  // the per-round workspaces at their largest now: growing one mid-pipeline would free it under queued work
  GLC_HIP(ctx, ctx->coef.reserve(static_cast<size_t>(max_nf) * ch * glc::kHop * sizeof(float)));
  if (n_rounds > 1) GLC_HIP(ctx, ctx->slot[1].coef.reserve(static_cast<size_t>(max_nf) * ch * glc::kHop * sizeof(float)));
  GLC_HIP(ctx, ctx->pack_meta.reserve(glc::compact_scratch_bytes(max_nf * ch)));
  GLC_HIP(ctx, ctx->stream_b.ensure());
  GLC_HIP(ctx, ctx->copy_stream.ensure());
  GLC_HIP(ctx, ctx->down_stream.ensure());
  while (ctx->ev_round.size() < n_rounds) {
    Event e;
    GLC_HIP(ctx, e.ensure());
    try {
      ctx->ev_round.push_back(std::move(e));
    } catch (const std::bad_alloc &) {
      return fail(ctx, GLC_ENOMEM, "glc_encode: host allocation failed");
    }
  }
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // earlier work may still read the staging buffers
  float *d_pcm = static_cast<float *>(ctx->pcm.p);
  uint8_t *d_blob = static_cast<uint8_t *>(ctx->pack_blob.p);
  const Event *ev_rec = ctx->ev_round.data();

  // what the three threads meet at (kUploaded, kQueued)
  StageGate prog;
  auto hip_msg = [](const char *what, hipError_t e) { return std::string(what) + ": " + hipGetErrorString(e); };
  double pairs_per_frame = 0.0;  // stored pairs per frame so far, + 25 % (sizes the next round's first copy)

  // A stream of a single round has nothing to run ahead of: integer samples have their copy and their widening
  // queued on the stream the round's kernels follow on, and nobody waits for them on the host.
  const bool up_in_order = is_int && n_rounds == 1;
  auto upload = [&] {  // stage 1
    upload_rounds(ctx, "glc_encode", prog, kUploaded, n_rounds, [&](size_t i) { return rounds[i].hi; }, pcm_any, fmt, bits, d_pcm,
                  static_cast<uint8_t *>(ctx->pcm_int.p), up_in_order ? ctx->stream : ctx->copy_stream, !up_in_order);
  };
  auto launch = [&] {  // stage 2
    std::string my_err;  // failures of this stage land here, not in ctx->err (another thread's to write)
    SinkGuard sink(&my_err);
    DeviceGuard g(ctx->device);
    for (size_t i = 0; i < n_rounds; ++i) {
      const Round &r = rounds[i];
      if (!prog.wait_for(kUploaded, i)) return;
      hipStream_t cs = (i & 1) ? ctx->stream_b : ctx->stream;
      hipError_t e = hipSuccess;
      uint8_t *recs = static_cast<uint8_t *>(ctx->records.p) + r.f0 * rec;
      int rc = encode_range_on(ctx, cs, EncodeRange{{d_pcm, 0, t_count, n_samples, ch}, r.f0, r.f0 + r.nf, recs, nullptr, &ctx->slot[i & 1]},
                               kEncodeBeside);
      if (rc != GLC_OK) return prog.set_error(rc, my_err);
      e = hipEventRecord(ev_rec[i], cs);
      if (e != hipSuccess) return prog.set_error(GLC_EHIP, hip_msg("glc_encode: queueing a round", e));
      prog.advance(kQueued);
    }
  };
  uint64_t p_used = 0, r_used = 0;  // the pools are grown ahead of need (below): what of them is filled
  // glc_encode_hooked: the hook runs on THIS thread (the collecting one), in the time it would otherwise
  // spend blocked waiting for the device: while round i's records are not ready, the frames of the
  // rounds already collected are handed out in small ranges, the event polled in between; whatever is
  // left when the last round has been collected follows at the end.  (A hook thread of the library's
  // own was built first and measured 2.46 ms against 1.49 for the config-2 call: what a hook does is
  // allocate - the host's nested vectors - and memory allocated on a helper thread and freed by the
  // caller lives in a secondary malloc arena that is trimmed and re-faulted on every call.)
  uint64_t delivered = 0, complete = 0;  // frames handed to the hook / complete in the EncodedAudio
  constexpr uint64_t kHookSlice = 64;    // frames per call while the device is being polled (a few microseconds of host work)
  auto deliver = [&](uint64_t upto) -> bool {  // frames [delivered, upto), upto <= complete
    glc_frames_view v;
    (void)glc_frames_get_view(F.get(), &v);
    v.n_frames = upto;
    v.n_lists = F->list_begin[upto];
    v.n_pairs = F->list_off[v.n_lists];
    v.n_scales = F->scale_begin[upto];
    v.n_raw = F->raw_begin[upto];
    const int hrc = hook(hook_user, &v, delivered, upto);
    delivered = upto;
    if (hrc != 0) prog.set_error(GLC_EINVAL, "glc_encode_hooked: the hook asked to stop");
    return hrc == 0;
  };
  // block until `st` has drained - handing out finished frames meanwhile (hooked encodes)
  const std::function<hipError_t(hipStream_t)> drain = [&](hipStream_t st) {
    if (hook)
      while (delivered < complete && hipStreamQuery(st) == hipErrorNotReady)
        if (!deliver(std::min(complete, delivered + kHookSlice))) break;
    return hipStreamSynchronize(st);
  };
  auto collect = [&] {  // stage 3
    std::string my_err;  // land_blob reports here; the calling thread stores the winning message at the end
    SinkGuard sink(&my_err);
    for (size_t i = 0; i < n_rounds; ++i) {
      const Round &r = rounds[i];
      if (i > 0) {
        // Growing a pool zero-fills it: do that for this round while its kernels still run, from the
        // density of the stream so far (+ 25 %); a round that turns out denser grows again as it lands.
        const double per_frame = static_cast<double>(p_used) / static_cast<double>(r.f0) * 1.25;
        const uint64_t want = p_used + static_cast<uint64_t>(per_frame * static_cast<double>(r.nf)) + 1024;
        if (F->pairs.size() < want) F->pairs.resize(want);
      }
      if (hook) {  // hand out finished frames while this round's records are not ready
        while (delivered < complete) {
          if (prog.failed()) return;
          if (prog.passed(kQueued, i) && hipEventQuery(ev_rec[i]) == hipSuccess) break;
          if (!deliver(std::min(complete, delivered + kHookSlice))) return;
        }
      }
      if (!prog.wait_for(kQueued, i)) return;
      hipError_t e = hipEventSynchronize(ev_rec[i]);  // the round's records are written: compact them now
      if (e != hipSuccess) return prog.set_error(GLC_EHIP, hip_msg("glc_encode: waiting for a round", e));
      // pairs the round is expected to hold, from the density of the stream so far (+ 25 %)
      uint64_t guess_pairs = 0;
      if (i > 0) guess_pairs = static_cast<uint64_t>(pairs_per_frame * static_cast<double>(r.nf)) + 1024;
      // the first of several rounds reserves the pools for the stream from its density (+ 30 %)
      const double reserve = i == 0 && n_rounds > 1 ? static_cast<double>(plan.n_frames) / static_cast<double>(r.nf) * 1.3 : 0.0;
      uint64_t n_pairs = 0, n_raw = 0;
      const int rc = land_blob(ctx, "glc_encode", F.get(), static_cast<uint8_t *>(ctx->records.p) + r.f0 * rec, r.nf,
                               d_blob + r.blob_off, r.f0, p_used, r_used, guess_pairs, reserve, ctx->down_stream, drain,
                               &n_pairs, &n_raw);
      if (rc != GLC_OK) return prog.set_error(rc, my_err);
      p_used += n_pairs;
      r_used += n_raw;
      pairs_per_frame = static_cast<double>(p_used) / static_cast<double>(r.f0 + r.nf) * 1.25;
      complete = r.f0 + r.nf;
    }
    if (hook && delivered < complete) (void)deliver(complete);
  };

  // A pipeline over rounds of at most kEncodeChunkFrames frames.  Every stage has its own stream AND
  // its own host thread, because two of the stages block their caller: a copy from or to pageable
  // memory returns when it is done.
  //   uploader thread   round i+1's samples go up, back to back                      (copy_stream)
  //   launcher thread   round i is transformed and quantised as soon as it is up     (stream / stream_b)
  //   this thread       round i-1 is compacted, its blob comes down - metadata, then the payload
  //                     straight into the EncodedAudio's pools - and is indexed       (down_stream)
  // PCIe is full duplex and the compaction kernels are small, so a call costs
  // max(upload, kernels) + the first upload + the last round's compaction and download instead of
  // their sum.  One rule keeps the stages from blocking each other: NOTHING IS QUEUED BEHIND AN
  // UNFINISHED DEPENDENCY.  A process has a handful of hardware queues for all its streams, and a
  // queue is in order: a `hipStreamWaitEvent` that has to wait parks every stream that shares its
  // queue (seen in the trace: the compaction's wait for the quantiser held the NEXT upload's event
  // back, and with it the next transform), and the copy engines execute in submission order.  So a
  // stage waits on the host (the gate, hipEventSynchronize) and only then queues its work.
  // An opening round's 2048-row launch alone leaves the chip half empty (its time is one workgroup's
  // 2048-step chain, 0.22 ms whatever the row count), so consecutive rounds run on TWO streams with
  // a coefficient workspace each: the next round's transform fills in beside this one's, and a
  // round's quantiser runs beside the next transform (four 1024-frame stereo launches: 0.87 ms on
  // one stream, 0.67 ms alternating, 0.59 ms as one launch; two 2048-frame ones 0.66 / 0.60).
  // A stream of one round runs on this thread alone.
  if (n_rounds == 1)
    run_stages(prog, "glc_encode", {}, [&] { upload(), launch(), collect(); });
  else
    run_stages(prog, "glc_encode", {{ctx->enc_up, std::ref(upload)}, {ctx->enc_launch, std::ref(launch)}}, collect);
  if (prog.failed()) {
    // nothing may still be in flight into the caller's or the result's memory when this returns
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->stream_b);
    (void)hipStreamSynchronize(ctx->down_stream);
    return fail(ctx, prog.code(), prog.message());
  }
  try {
    F->pairs.resize(p_used);  // shrinks: the pools were grown ahead of need
    F->raw.resize(r_used);
  } catch (const std::bad_alloc &) {
    return fail(ctx, GLC_ENOMEM, "glc_encode: host allocation failed");
  }
  F->lists_canonical = true;  // ballot-packed in ascending k
  if (out) *out = F.release();
  return GLC_OK;
}

// ------------------------------------------------------------------------------ encode, many clips

namespace {

// The blob of a batch round (glc_encode_batch): header | clip directory u64[2 n_clips] |
// raw flags | scales | counts | pairs | raw planes, over the n_real REAL frames of the round's clips (M rows).
struct BatchBlobLayout {
  glc::CompactLayout at;  // the sections, behind a directory of dir_bytes
  uint64_t n_real, M, V;  // frames of the clips / their rows / records of the virtual stream (a junk one behind every clip)
  uint64_t o_dir, dir_bytes;
};
BatchBlobLayout batch_blob_layout(uint32_t ch, const uint64_t *clip_frames, uint64_t n_clips) {
  uint64_t n_real = 0, V = 0;
  for (uint64_t i = 0; i < n_clips; ++i) n_real += clip_frames[i], V += clip_frames[i] + 1;
  return BatchBlobLayout{glc::compact_layout(ch, n_real, 16 * n_clips), n_real, n_real * ch, V, sizeof(glc::CompactHeader),
                         16 * n_clips};
}

// Queues the segment-aware compaction of a batch round on `st`: clip i of clip_frames[i] frames owns the records
// slot_i .. slot_i + clip_frames[i] - 1 of `d_records`, record slot_i + clip_frames[i] is junk and slot_{i+1} comes
// behind it.  The frame map (pinned in host_stage behind the blob's first o_pairs bytes, on the device behind the
// scratch of compact_launch in pack_meta), the zeroed header / directory / section padding, then P1-P3 into
// `d_blob` (l.bound bytes).  Nothing is synchronised.
int compact_batch_launch(glc_ctx *ctx, const void *d_records, const uint64_t *clip_frames, uint64_t n_clips, uint32_t ch,
                         const BatchBlobLayout &l, uint8_t *d_blob, hipStream_t st) {
  if (l.M > 0xFFFFFFFFull || l.V > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, "batch compaction: frame range too long");
  const size_t scratch = glc::compact_scratch_bytes(l.M), o_fmap_h = align_up(l.at.o_pairs, 256);
  GLC_HIP(ctx, ctx->pack_meta.reserve(scratch + align_up(l.n_real * sizeof(glc::FrameMap), 256)));
  GLC_HIP(ctx, ctx->host_stage.reserve(o_fmap_h + l.n_real * sizeof(glc::FrameMap)));
  glc::FrameMap *fmap = reinterpret_cast<glc::FrameMap *>(static_cast<uint8_t *>(ctx->host_stage.p) + o_fmap_h);
  uint64_t slot = 0, real = 0;
  for (uint64_t i = 0; i < n_clips; ++i) {
    for (uint64_t f = 0; f < clip_frames[i]; ++f)
      fmap[real + f] = glc::FrameMap{static_cast<uint32_t>(slot + f), f == 0 ? static_cast<uint32_t>(i) : 0xFFFFFFFFu};
    slot += clip_frames[i] + 1;
    real += clip_frames[i];
  }
  glc::FrameMap *d_fmap = reinterpret_cast<glc::FrameMap *>(static_cast<uint8_t *>(ctx->pack_meta.p) + scratch);
  GLC_HIP(ctx, hipMemcpyAsync(d_fmap, fmap, l.n_real * sizeof(glc::FrameMap), hipMemcpyHostToDevice, st));
  GLC_HIP(ctx, hipMemsetAsync(d_blob, 0, l.at.o_pairs, st));  // header + directory + section padding: deterministic bytes
  GLC_HIP(ctx, glc::launch_compact(static_cast<const uint8_t *>(d_records), static_cast<uint32_t>(l.M), ch, l.n_real, ctx->pack_meta.p,
                                   d_blob, l.at, d_fmap, reinterpret_cast<uint64_t *>(d_blob + l.o_dir), st));
  return GLC_OK;
}

struct BatchClip {
  uint64_t index;  // in the caller's arrays
  glc_plan plan;
};

// One round of glc_encode_batch: the clips `clips` (together at most encode_chunk_frames(ch) virtual
// frames) through K1 / K2 / K3 as ONE virtual stream, one segment-aware compaction, two downloads.
// Layout of the virtual stream: clip i of nf_i frames owns the (nf_i + 1) * 1024
// per-channel samples from 1024 * slot_i on, its samples first, +0.0 behind them - the reference's own
// padding (src/codec.rs:433-447), here in memory because the next clip follows.  Frame f of the clip
// is virtual frame slot_i + f and reads nothing outside the clip's slot and the zeros in front of it;
// virtual frame slot_i + nf_i straddles two clips and is junk: computed, in no frame map, never sent.
// Integer clips (glc_encode_batch_int, fmt != GLC_PCM_F32): the same image in the clips' own element width -
// memset, pinned image, uploads all hold the INTEGERS, in ctx->pcm_int - and ONE widening of the whole
// virtual stream into ctx->pcm behind them.  Slots are whole multiples of 1024 * ch elements, so a slot
// starts at the same element index in either width.
int encode_batch_round(glc_ctx *ctx, const std::vector<BatchClip> &clips, const void *const *pcm, glc_pcm_format fmt,
                       uint32_t bits, const uint64_t *n_samples, uint16_t channels,
                       std::vector<std::unique_ptr<glc_frames>> &result) {
  const uint32_t ch = channels;
  const bool is_int = fmt != GLC_PCM_F32;
  const uint64_t elem = pcm_elem(fmt);  // bytes per sample as uploaded
  const uint64_t n = clips.size();
  std::vector<uint64_t> clip_frames(n);
  for (uint64_t i = 0; i < n; ++i) clip_frames[i] = clips[i].plan.n_frames;
  const BatchBlobLayout bl = batch_blob_layout(ch, clip_frames.data(), n);  // the round's blob
  const uint64_t V = bl.V, n_real = bl.n_real;  // frames of the virtual stream / of the clips
  const uint64_t T = V * glc::kHop, n_virtual = T * ch;
  const uint64_t rec = glc::record_bytes(ch);
  const uint64_t o_dir = bl.o_dir, o_israw = bl.at.o_israw, o_scale = bl.at.o_scale, o_cnt = bl.at.o_cnt, o_pairs = bl.at.o_pairs,
                 bound = bl.at.bound;
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // earlier work may still read the staging buffers
  GLC_HIP(ctx, ctx->pcm.reserve(static_cast<size_t>(n_virtual) * sizeof(float)));
  if (is_int) GLC_HIP(ctx, ctx->pcm_int.reserve(static_cast<size_t>(n_virtual) * elem));
  GLC_HIP(ctx, ctx->records.reserve(static_cast<size_t>(V) * rec));
  GLC_HIP(ctx, ctx->pack_blob.reserve(bound));
  float *d_pcm = static_cast<float *>(ctx->pcm.p);
  uint8_t *d_up = static_cast<uint8_t *>(is_int ? ctx->pcm_int.p : ctx->pcm.p);  // where the uploads land
  uint8_t *d_blob = static_cast<uint8_t *>(ctx->pack_blob.p);
  hipStream_t st = ctx->stream;

  // Staging: zeros everywhere (a recycled buffer holds old samples), then every clip into its slot.  A copy
  // from pageable memory costs 11 us before it moves a byte, a host memcpy into pinned memory runs at half
  // the speed of the DMA (tools/h2d_probe.cpp `clips`: 64 x 689 KiB take 1.49 ms with a copy each against 2.07 packed,
  // 512 x 86 KiB 5.84 against 2.26): clips of at most kPackClipBytes are packed, slot by slot with their zeros, into
  // a pinned image that goes up in runs of kPackRunBytes (the next run is packed while one is in flight);
  // longer clips go up on their own, straight from the caller's memory.  Both limits are bytes as they travel:
  // a 16-bit clip is packed up to twice the samples of a float one.
  constexpr uint64_t kPackClipBytes = 256u << 10, kPackRunBytes = 4u << 20;
  auto slot_bytes = [&](const BatchClip &c) { return (c.plan.n_frames + 1) * glc::kHop * ch * elem; };
  uint64_t packed = 0;
  for (const BatchClip &c : clips)
    if (n_samples[c.index] * elem <= kPackClipBytes) packed += slot_bytes(c);
  if (packed) GLC_HIP(ctx, ctx->batch_stage.reserve(packed));
  uint8_t *pin = static_cast<uint8_t *>(ctx->batch_stage.p);
  uint64_t pin_at = 0, run_begin = 0, run_dev = 0;  // bytes packed / where the open run starts in `pin` / in d_up (samples)
  auto send_run = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    if (pin_at > run_begin)
      e = hipMemcpyAsync(d_up + run_dev * elem, pin + run_begin, pin_at - run_begin, hipMemcpyHostToDevice, st);
    run_begin = pin_at;
    return e;
  };
  GLC_HIP(ctx, hipMemsetAsync(d_up, 0, static_cast<size_t>(n_virtual) * elem, st));
  uint64_t slot = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const BatchClip &c = clips[i];
    const uint64_t bytes = n_samples[c.index] * elem, at = slot * glc::kHop * ch;
    if (bytes <= kPackClipBytes) {
      if (pin_at == run_begin) run_dev = at;  // a run starts with this clip; consecutive clips have consecutive slots
      std::memcpy(pin + pin_at, pcm[c.index], bytes);
      std::memset(pin + pin_at + bytes, 0, slot_bytes(c) - bytes);
      pin_at += slot_bytes(c);
      if (pin_at - run_begin >= kPackRunBytes) GLC_HIP(ctx, send_run());
    } else {
      GLC_HIP(ctx, send_run());
      GLC_HIP(ctx, hipMemcpyAsync(d_up + at * elem, pcm[c.index], bytes, hipMemcpyHostToDevice, st));
    }
    slot += c.plan.n_frames + 1;
  }
  GLC_HIP(ctx, send_run());
  // One widening for the round, whatever the number of clips: every element of the virtual stream, the zeros
  // between and behind the clips included (d_pcm needs no memset of its own).  A zero widens to +0.0 - except
  // with bits == 32, whose divisor is -2^31 (quirk Q11): there it, like a zero SAMPLE of glc_encode_int, becomes
  // -0.0 where the reference pads with +0.0.  No output tells the two apart: a transform sum starts from +0.0
  // and +0.0 + -0.0 = +0.0, the raw planes narrow both to 0.
  if (is_int) GLC_HIP(ctx, glc::launch_pcm_widen(d_up, fmt == GLC_PCM_S32, bits, n_virtual, d_pcm, st));

  int rc = encode_range_on(ctx, st, EncodeRange{{d_pcm, 0, T, n_virtual, ch}, 0, V, ctx->records.p, nullptr, &ctx->slot[0]});
  if (rc != GLC_OK) return rc;

  rc = compact_batch_launch(ctx, ctx->records.p, clip_frames.data(), n, ch, bl, d_blob, st);
  if (rc != GLC_OK) return rc;
  uint8_t *hm = static_cast<uint8_t *>(ctx->host_stage.p);  // reserved by compact_batch_launch: o_pairs bytes and the frame map
  // download 1: header, directory and the per-frame / per-row sections - they say how long the payload is
  GLC_HIP(ctx, hipMemcpyAsync(hm, d_blob, o_pairs, hipMemcpyDeviceToHost, st));
  GLC_HIP(ctx, hipStreamSynchronize(st));
  glc::CompactHeader h;
  std::memcpy(&h, hm, sizeof h);
  if (glc::compact_header_fault(h, ch, n_real, bl.dir_bytes, /*exact=*/true, bound) != glc::HeaderFault::kNone)
    return fail(ctx, GLC_EHIP, "glc_encode_batch: the device wrote an inconsistent compact header");
  const uint64_t raw_off = glc::compact_raw_offset(bl.at, h.n_pairs);
  // download 2: the payload of all clips in one copy, cut per clip on the host below
  const uint64_t payload = h.bytes - o_pairs;
  GLC_HIP(ctx, ctx->batch_stage.reserve(std::max<uint64_t>(payload, 64)));
  const uint8_t *pay = static_cast<const uint8_t *>(ctx->batch_stage.p);
  if (payload) GLC_HIP(ctx, hipMemcpyAsync(ctx->batch_stage.p, d_blob + o_pairs, payload, hipMemcpyDeviceToHost, st));
  // ... and while it is on its way, the index vectors of every clip
  const uint64_t *dir = reinterpret_cast<const uint64_t *>(hm + o_dir);
  const uint8_t *israw = hm + o_israw;
  const float *scale = reinterpret_cast<const float *>(hm + o_scale);
  const uint32_t *cnt = reinterpret_cast<const uint32_t *>(hm + o_cnt);
  std::vector<std::unique_ptr<glc_frames>> made(n);
  uint64_t real = 0;
  for (uint64_t i = 0; i < n && rc == GLC_OK; ++i) {
    const BatchClip &c = clips[i];
    const uint64_t p0 = dir[2 * i], q0 = dir[2 * i + 1];
    const uint64_t p1 = i + 1 < n ? dir[2 * i + 2] : h.n_pairs, q1 = i + 1 < n ? dir[2 * i + 3] : h.n_raw_rows;
    if (p0 > p1 || p1 > h.n_pairs || q0 > q1 || q1 > h.n_raw_rows) {
      rc = fail(ctx, GLC_EHIP, "glc_encode_batch: the device wrote an inconsistent clip directory");
      break;
    }
    made[i].reset(new glc_frames);
    glc_frames *F = made[i].get();
    glc::init_frames(F, ctx->sample_rate, n_samples[c.index], channels, c.plan);
    F->pairs.resize(p1 - p0);
    F->raw.resize((q1 - q0) * glc::kFrame);
    bool canonical = true;
    const int irc = glc::index_compact_rows(F, ch, c.plan.n_frames, p1 - p0, q1 - q0, israw + real, scale + real * ch,
                                            cnt + real * ch, 0, 0, 0, /*trusted=*/true, &canonical);
    if (irc != GLC_OK) rc = fail(ctx, irc, std::string("glc_encode_batch: ") + glc_last_error(nullptr));
    F->lists_canonical = true;  // ballot-packed in ascending k
    real += c.plan.n_frames;
  }
  const hipError_t e = hipStreamSynchronize(st);
  if (rc != GLC_OK) return rc;
  if (e != hipSuccess) return hip_fail(ctx, e, "glc_encode_batch: download");
  const uint32_t *pairs = reinterpret_cast<const uint32_t *>(pay);
  const int16_t *raw = reinterpret_cast<const int16_t *>(pay + (raw_off - o_pairs));
  for (uint64_t i = 0; i < n; ++i) {
    glc_frames *F = made[i].get();
    if (!F->pairs.empty()) std::memcpy(F->pairs.data(), pairs + dir[2 * i], F->pairs.size() * 4);
    if (!F->raw.empty()) std::memcpy(F->raw.data(), raw + dir[2 * i + 1] * glc::kFrame, F->raw.size() * 2);
    result[clips[i].index] = std::move(made[i]);
  }
  return GLC_OK;
}

int encode_batch_impl(glc_ctx *ctx, const char *who, const void *const *pcm, glc_pcm_format fmt, uint32_t bits,
                      const uint64_t *n_samples, uint64_t n_clips, uint16_t channels, glc_frames **out) {
  std::vector<BatchClip> all(n_clips);
  for (uint64_t i = 0; i < n_clips; ++i) {
    all[i] = BatchClip{i, glc::plan_encode(n_samples[i], channels)};
    if (all[i].plan.n_frames == 0)
      return fail(ctx, GLC_EINVAL,
                  std::string(who) + ": clip " + std::to_string(i) +
                      ": the reference encoder panics on this input (channels == 0, <= 512 samples per channel, or "
                      "ragged channels)");
    if (!pcm[i]) return fail(ctx, GLC_EINVAL, std::string(who) + ": clip " + std::to_string(i) + ": null pointer");
  }
  DeviceGuard guard(ctx->device);
  std::vector<std::unique_ptr<glc_frames>> result(n_clips);
  // the budget: virtual frames per round, so that the workspaces stay round-sized
  const auto rounds = pack_rounds(n_clips, [&](uint64_t i) { return all[i].plan.n_frames; }, encode_chunk_frames(channels), 0);
  int rc = GLC_OK;
  for (size_t k = 0; k < rounds.size() && rc == GLC_OK; ++k) {
    const RoundSpan &r = rounds[k];
    // longer than a round, or a round to itself: it shares nothing, and the single-stream pipeline overlaps the uploads,
    // kernels and downloads of one stream
    if (r.lng || r.n == 1) {
      glc_frames *f = nullptr;
      rc = encode_pipeline(ctx, pcm[r.first], fmt, bits, n_samples[r.first], channels, nullptr, nullptr, &f);
      result[r.first].reset(f);
    } else {
      const std::vector<BatchClip> round(all.begin() + r.first, all.begin() + r.first + r.n);
      rc = encode_batch_round(ctx, round, pcm, fmt, bits, n_samples, channels, result);
    }
  }
  if (rc != GLC_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing may still be in flight out of the caller's memory
    return rc;
  }
  for (uint64_t i = 0; i < n_clips; ++i) out[i] = result[i].release();
  return GLC_OK;
}

}  // namespace

// glc_encode_batch / glc_encode_batch_int behind their argument checks
static int encode_batch_checked(glc_ctx *ctx, const char *who, const void *const *pcm, glc_pcm_format fmt, uint32_t bits,
                                const uint64_t *n_samples, uint64_t n_clips, uint16_t channels, glc_frames **out) {
  const std::string w(who);
  if (!ctx) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (n_clips == 0) return GLC_OK;
  if (!pcm || !n_samples || !out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  for (uint64_t i = 0; i < n_clips; ++i) out[i] = nullptr;
  if (channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  try {  // no C++ exception may cross the C ABI
    return encode_batch_impl(ctx, who, pcm, fmt, bits, n_samples, n_clips, channels, out);
  } catch (const std::bad_alloc &) {
    (void)hipStreamSynchronize(ctx->stream);
    return fail(ctx, GLC_ENOMEM, w + ": host allocation failed");
  }
}

int glc_encode_batch(glc_ctx *ctx, const float *const *pcm, const uint64_t *n_samples, uint64_t n_clips, uint16_t channels,
                     glc_frames **out) {
  return encode_batch_checked(ctx, "glc_encode_batch", reinterpret_cast<const void *const *>(pcm), GLC_PCM_F32, 32, n_samples,
                              n_clips, channels, out);
}

int glc_encode_batch_int(glc_ctx *ctx, const void *const *pcm, glc_pcm_format fmt, uint32_t bits, const uint64_t *n_samples,
                         uint64_t n_clips, uint16_t channels, glc_frames **out) {
  if (!ctx) return fail(ctx, GLC_EINVAL, "glc_encode_batch_int: null argument");
  if (fmt == GLC_PCM_F32)
    return glc_encode_batch(ctx, reinterpret_cast<const float *const *>(pcm), n_samples, n_clips, channels, out);
  if (out)
    for (uint64_t i = 0; i < n_clips; ++i) out[i] = nullptr;
  if (fmt != GLC_PCM_S16 && fmt != GLC_PCM_S32) return fail(ctx, GLC_EINVAL, "glc_encode_batch_int: unknown sample format");
  if (bits == 0 || bits > (fmt == GLC_PCM_S16 ? 16u : 32u))
    return fail(ctx, GLC_EINVAL, "glc_encode_batch_int: bits must be 1..16 for 16-bit samples, 1..32 for 32-bit ones");
  return encode_batch_checked(ctx, "glc_encode_batch_int", pcm, fmt, bits, n_samples, n_clips, channels, out);
}

// ------------------------------------------------------------------------------ decode

extern "C++" {  // templates over the output sample type
namespace {

// Upload the sparse representation of `in` and reset the overlap state: after this the stream
// can be decoded front to back in rounds (round_launch).  Sparse lists are used as stored when
// canonical (strictly ascending, idx < 1024 — what the encoder emits); other lists are
// canonicalised on the host with the reference's dense-array semantics (last write wins,
// idx >= 1024 ignored, src/codec.rs:659-665) and appended behind the stored pairs.
int decode_prepare_impl(glc_ctx *ctx, const glc_frames *in);

int decode_prepare(glc_ctx *ctx, const glc_frames *in) {
  try {  // no C++ exception may cross the C ABI
    return decode_prepare_impl(ctx, in);
  } catch (const std::bad_alloc &) {
    return fail(ctx, GLC_ENOMEM, "glc_decode: host allocation failed");
  }
}

// D1's plan workspace for a launch of `nf` frames: its (8-frame group, channel) units, at most kPlanGroups
// per batch (66 KB per unit: a 12-frame clip needs 4 units, not the 135 MB of a full batch)
int reserve_d1_plan(glc_ctx *ctx, uint64_t nf, uint32_t ch) {
  if (ctx->d1_variant == 1) return GLC_OK;
  DeviceGuard guard_plan(ctx->device);
  const uint64_t units = ((nf + 7) / 8) * ch;
  const uint32_t want = static_cast<uint32_t>(std::max<uint64_t>(ch, std::min<uint64_t>(std::max<uint32_t>(kPlanGroups, ch), units)));
  if (want > ctx->dec_plan_groups) {
    GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // queued launches may still read the old workspace
    GLC_HIP(ctx, ctx->dec_plan.reserve(glc::imdct_plan_bytes(want)));
    ctx->dec_plan_groups = want;
    ctx->plan_uid = 0;
  }
  return GLC_OK;
}

// The row tables D1 reads, for ONE stream (decode_prepare_impl) or for the streams of a round of
// glc_decode_batch laid end to end: rows in stream order, the stored pairs of all streams back to back
// (a row's pair range rebased by what the streams before it hold), then the canonicalised copies of
// non-canonical lists; raw vectors likewise in one pool.
// The five per-row arrays are built in ONE host block in the layout they have on the device, so that
// they go up in one copy (each copy from pageable memory costs ~20 us before it moves a byte: eight
// of them were a third of what a context spends on a stream it has not seen).
struct RowTable {
  size_t h_begin = 0, h_cnt = 0, h_scale = 0, h_raw = 0, h_rawlen = 0, h_end = 0;  // byte offsets inside `block`
  std::vector<uint64_t> block;  // 8-byte aligned storage
  std::vector<uint32_t> extra;  // canonicalised copies of non-canonical lists
  uint64_t n_stored = 0, n_raw = 0;  // stored pairs / raw samples of all the streams
  uint32_t any_raw = 0;
};

// `M`: rows of all the streams (each of `ch` channels).  `who`: the entry point for the error message, which
// names the stream when there are several.
int build_row_table(glc_ctx *ctx, const char *who, const glc_frames *const *streams, uint64_t n_streams, uint32_t ch,
                    uint64_t M, RowTable &t) {
  const size_t Mr = std::max<size_t>(M, 1);
  t.h_begin = 0, t.h_cnt = align_up(t.h_begin + Mr * 8, 256), t.h_scale = align_up(t.h_cnt + Mr * 4, 256),
  t.h_raw = align_up(t.h_scale + Mr * 4, 256), t.h_rawlen = align_up(t.h_raw + Mr * 8, 256),
  t.h_end = align_up(t.h_rawlen + Mr * 8, 256);
  t.block.assign(t.h_end / 8, 0);
  uint8_t *hb = reinterpret_cast<uint8_t *>(t.block.data());
  uint64_t *row_begin = reinterpret_cast<uint64_t *>(hb + t.h_begin);
  uint32_t *row_cnt = reinterpret_cast<uint32_t *>(hb + t.h_cnt);
  float *row_scale = reinterpret_cast<float *>(hb + t.h_scale);
  int64_t *row_raw = reinterpret_cast<int64_t *>(hb + t.h_raw);
  uint64_t *row_raw_len = reinterpret_cast<uint64_t *>(hb + t.h_rawlen);
  for (uint64_t m = 0; m < M; ++m) row_raw[m] = -1;
  t.any_raw = 0;
  t.extra.clear();
  t.n_stored = t.n_raw = 0;
  for (uint64_t s = 0; s < n_streams; ++s) t.n_stored += streams[s]->pairs.size(), t.n_raw += streams[s]->raw.size();
  std::vector<int32_t> dense;
  uint64_t row0 = 0, pair0 = 0, raw0 = 0;  // what the streams in front of this one hold
  for (uint64_t s = 0; s < n_streams; ++s) {
    const glc_frames *in = streams[s];
    const uint64_t nf = in->n_frames;
    for (uint64_t f = 0; f < nf; ++f) {
      if (in->raw_tag[f]) {
        t.any_raw = 1;
        for (uint32_t c = 0; c < ch; ++c) {
          row_raw[row0 + f * ch + c] = static_cast<int64_t>(raw0 + in->raw_begin[f]);
          row_raw_len[row0 + f * ch + c] = in->raw_begin[f + 1] - in->raw_begin[f];
        }
        continue;
      }
      const uint64_t l0 = in->list_begin[f], nl = in->list_begin[f + 1] - l0;
      const uint64_t s0 = in->scale_begin[f], ns = in->scale_begin[f + 1] - s0;
      if (nl < ch || ns < ch)  // the reference indexes [ch] out of bounds and panics, :652-653
        return fail(ctx, GLC_EFORMAT,
                    std::string(who) + (n_streams > 1 ? ": stream " + std::to_string(s) : std::string()) +
                        ": frame has fewer channel vectors than header.channels");
      for (uint32_t c = 0; c < ch; ++c) {
        const uint64_t a = in->list_off[l0 + c], b = in->list_off[l0 + c + 1];
        bool canonical = true;
        if (!in->lists_canonical && b > a) {
          // strictly ascending indices below 1024: branch-free over the whole list, so that the compiler
          // vectorises it (streams built by glc_frames_from_parts / _gather / glc_deserialize come through
          // here on their first decode: 0.9 M pairs at config 2)
          const uint32_t *pp = in->pairs.data() + a;
          const uint64_t n_p = b - a;
          uint32_t bad = (pp[0] & 0xFFFFu) >= glc::kHop ? 1u : 0u;
          for (uint64_t j = 1; j < n_p; ++j) {
            const uint32_t k = pp[j] & 0xFFFFu, kp = pp[j - 1] & 0xFFFFu;
            bad |= (k <= kp ? 1u : 0u) | (k >= glc::kHop ? 1u : 0u);
          }
          canonical = bad == 0;
        }
        const uint64_t m = row0 + f * ch + c;
        if (canonical) {
          row_begin[m] = pair0 + a;
          row_cnt[m] = static_cast<uint32_t>(b - a);
        } else {
          dense.assign(glc::kHop, INT32_MIN);
          for (uint64_t j = a; j < b; ++j) {
            const uint32_t k = in->pairs[j] & 0xFFFFu;
            if (k < glc::kHop) dense[k] = static_cast<int16_t>(in->pairs[j] >> 16);
          }
          row_begin[m] = t.n_stored + t.extra.size();
          // stored zeros stay: 0 * scale is NaN when the scale is infinite (src/codec.rs:663), and
          // the result must not depend on whether the list happened to be in canonical order
          for (uint32_t k = 0; k < glc::kHop; ++k)
            if (dense[k] != INT32_MIN)
              t.extra.push_back(k | (static_cast<uint32_t>(static_cast<uint16_t>(dense[k])) << 16));
          row_cnt[m] = static_cast<uint32_t>(t.n_stored + t.extra.size() - row_begin[m]);
        }
        row_scale[m] = in->scales[s0 + c];
      }
    }
    row0 += nf * ch;
    pair0 += in->pairs.size();
    raw0 += in->raw.size();
  }
  return GLC_OK;
}

int decode_prepare_impl(glc_ctx *ctx, const glc_frames *in) {
  const uint32_t ch = in->channels;
  if (ch == 0) return fail(ctx, GLC_EINVAL, "glc_decode: header.channels == 0");
  const uint64_t nf = in->n_frames;
  const uint64_t M = nf * ch;
  if (M > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, "glc_decode: stream too long");
  int rc = reserve_d1_plan(ctx, nf, ch);
  if (rc != GLC_OK) return rc;
  // The sparse rows of this stream are still on the device from an earlier call (a glc_frames is
  // immutable and its uid is unique in the process, or a caller-supplied identity of the content;
  // the pool sizes are compared as well, so that a recycled id does not silently decode old rows).
  if (ctx->dec_uid != 0 && ctx->dec_uid == in->uid && ctx->dec_frames == nf && ctx->dec_ch == ch &&
      ctx->dec_n_pairs == in->pairs.size() && ctx->dec_n_raw == in->raw.size() && ctx->dec_delay == in->encoder_delay &&
      ctx->dec_orig_len == in->original_length) {
    ctx->dec_next = 0;
    return GLC_OK;
  }
  ctx->dec_uid = 0;
  ctx->plan_uid = 0;

  RowTable t;
  rc = build_row_table(ctx, "glc_decode", &in, 1, ch, M, t);
  if (rc != GLC_OK) return rc;

  DeviceGuard guard(ctx->device);
  TableOffsets offs;
  const size_t o_pairs = offs.take(std::max<size_t>(t.n_stored + t.extra.size(), 1) * 4);
  const size_t o_rows = offs.take(t.h_end);  // the row block, as it is
  const size_t o_pool = offs.take(std::max<size_t>(in->raw.size(), 1) * 2);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a previous session may still read dec_meta
  GLC_HIP(ctx, ctx->dec_meta.reserve(offs.size()));
  uint8_t *mb = static_cast<uint8_t *>(ctx->dec_meta.p);
  auto up = [&](size_t o, const void *src, size_t bytes) -> hipError_t {
    if (!bytes) return hipSuccess;
    return hipMemcpyAsync(mb + o, src, bytes, hipMemcpyHostToDevice, ctx->stream);
  };
  GLC_HIP(ctx, up(o_pairs, in->pairs.data(), t.n_stored * 4));
  GLC_HIP(ctx, up(o_pairs + t.n_stored * 4, t.extra.data(), t.extra.size() * 4));
  GLC_HIP(ctx, up(o_rows, t.block.data(), t.h_end));
  GLC_HIP(ctx, up(o_pool, in->raw.data(), in->raw.size() * 2));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host vectors above go out of scope
  ctx->dec_rows = glc::DecodeRows{reinterpret_cast<const uint32_t *>(mb + o_pairs),
                                  reinterpret_cast<const uint64_t *>(mb + o_rows + t.h_begin),
                                  reinterpret_cast<const uint32_t *>(mb + o_rows + t.h_cnt),
                                  reinterpret_cast<const float *>(mb + o_rows + t.h_scale),
                                  reinterpret_cast<const int64_t *>(mb + o_rows + t.h_raw),
                                  reinterpret_cast<const uint64_t *>(mb + o_rows + t.h_rawlen),
                                  reinterpret_cast<const int16_t *>(mb + o_pool), t.any_raw};
  ctx->dec_ch = ch;
  ctx->dec_frames = nf;
  ctx->dec_next = 0;
  ctx->dec_uid = in->uid;
  ctx->dec_delay = in->encoder_delay;
  ctx->dec_orig_len = in->original_length;
  ctx->dec_n_pairs = in->pairs.size();
  ctx->dec_n_raw = in->raw.size();
  return GLC_OK;
}

// D1 of rows [row0, row0 + M) of `rows` on `st`, by the context's variant and through its plan workspace.  `reuse`:
// the workspace still holds the plan of this very launch (launch_d1).
hipError_t launch_d1_rows(glc_ctx *ctx, const glc::DecodeRows &rows, uint32_t row0, uint32_t M, uint32_t ch, float *blocks, hipStream_t st,
                          bool reuse = false) {
  return glc::launch_imdct_rows(ctx->dev, rows, row0, M, ch, blocks, st, ctx->d1_variant, ctx->dec_plan.p,
                                ctx->dec_plan.p ? ctx->dec_plan_groups : 0, reuse);
}

// D1 for rows [row_begin, row_begin + M) of the prepared stream.  A launch that fits one batch of the
// plan workspace leaves its plan records (and the unit order) behind; the same launch of the same
// stream again - a repeated decode - skips k_imdct_plan.
int launch_d1(glc_ctx *ctx, uint32_t row_begin, uint32_t M, float *blocks) {
  const uint32_t ch = ctx->dec_ch;
  const bool planned = ctx->d1_variant != 1 && ch != 0 && M % ch == 0;
  const bool one_batch = planned && ((M / ch + 7) / 8) * ch <= ctx->dec_plan_groups;
  const bool reuse = one_batch && ctx->plan_uid == ctx->dec_uid && ctx->plan_uid != 0 && ctx->plan_row_begin == row_begin &&
                     ctx->plan_M == M;
  GLC_HIP(ctx, launch_d1_rows(ctx, ctx->dec_rows, row_begin, M, ch, blocks, ctx->stream, reuse));
  if (planned) {
    ctx->plan_uid = one_batch ? ctx->dec_uid : 0;
    ctx->plan_row_begin = row_begin;
    ctx->plan_M = M;
  }
  return GLC_OK;
}

// One decode round: D1 of frames [f0, f0 + n) into block slots 1.., the overlap-add of their hops
// (+ `tail`: the bare overlap tail, hop n_frames) into dout, then, when another round follows
// (`carry`), the last frame's block copied to slot 0 for that round's overlap-add.
// T (here and below): the sample type of the output, float or int16_t.
template <typename T>
int decode_round(glc_ctx *ctx, uint64_t f0, uint64_t n, bool tail, bool carry, T *dout) {
  const uint32_t ch = ctx->dec_ch;
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;  // floats per frame
  float *blocks = static_cast<float *>(ctx->blocks.p);
  if (n) {
    const int rc = launch_d1(ctx, static_cast<uint32_t>(f0 * ch), static_cast<uint32_t>(n * ch), blocks + slot);
    if (rc != GLC_OK) return rc;
  }
  GLC_HIP(ctx, glc::launch_overlap_add(blocks, static_cast<int64_t>(f0) - 1, ctx->dec_frames, ch, f0, f0 + n + (tail ? 1 : 0), dout,
                                       ctx->stream));
  if (carry)
    GLC_HIP(ctx, hipMemcpyAsync(blocks, blocks + n * slot, slot * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  return GLC_OK;
}

// Queue the kernels of the next round of at most `round_frames` frames of the prepared session into
// `dout` (hop dec_next at dout[0]) and mark their completion with `ev`.  A round that reaches the
// last frame also produces the bare overlap tail (src/codec.rs:722-729); `flush_at_full` selects
// the reference's streaming rule (a chunk is flushed once it holds >= 500 frames, :708-717, so a
// stream of exactly k*500 frames ends with a tail-only chunk).  Slot 0 of the block ring carries
// the previous round's last frame for the overlap-add.
template <typename T>
int round_launch(glc_ctx *ctx, uint64_t round_frames, bool flush_at_full, T *dout, hipEvent_t ev,
                 uint64_t *frames_out, bool *last_out) {
  const uint64_t f0 = ctx->dec_next, left = ctx->dec_frames - f0;
  const bool last = flush_at_full ? left < round_frames : left <= round_frames;
  const uint64_t n = last ? left : round_frames;
  DeviceGuard guard(ctx->device);
  // (overlap = 0.0 before the first frame, :601: the overlap-add never reads slot 0 for hop 0)
  const int rc = decode_round(ctx, f0, n, /*tail=*/last, /*carry=*/!last, dout);
  if (rc != GLC_OK) return rc;
  GLC_HIP(ctx, hipEventRecord(ev, ctx->stream));
  ctx->dec_next = f0 + n;
  *frames_out = n;
  *last_out = last;
  return GLC_OK;
}

int ensure_copy_objects(glc_ctx *ctx) {
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, ctx->copy_stream.ensure());
  for (Event &e : ctx->ev_dec) GLC_HIP(ctx, e.ensure());
  return GLC_OK;
}

// Hops [hop_begin, hop_end) of the un-trimmed stream (hop h = second half of frame h-1 + first
// half of frame h; hop n_frames is the bare tail) into device memory at d_out, after
// decode_prepare.  A range that does not start at 0 recomputes frame hop_begin-1 as its halo: the
// only state the overlap-add carries (src/codec.rs:701-705), which is what lets GPUs decode
// disjoint hop ranges of one stream independently.
template <typename T>
int decode_hops_prepared(glc_ctx *ctx, uint64_t hop_begin, uint64_t hop_end, T *d_out) {
  if (hop_end <= hop_begin) return GLC_OK;
  const uint32_t ch = ctx->dec_ch;
  const uint64_t nf = ctx->dec_frames;
  DeviceGuard guard(ctx->device);
  const uint64_t f_end = std::min(hop_end, nf);  // frames [hop_begin, f_end) are decoded for their own hops
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(kDecodeChunkFrames, f_end > hop_begin ? f_end - hop_begin : 1));
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;
  GLC_HIP(ctx, ctx->blocks.reserve((chunk + 1) * slot * sizeof(float)));
  float *blocks = static_cast<float *>(ctx->blocks.p);
  if (hop_begin != 0) {  // (hop 0 has no frame before it: overlap = 0.0, :601, and slot 0 is never read for it)
    const int rc = launch_d1(ctx, static_cast<uint32_t>((hop_begin - 1) * ch), ch, blocks);
    if (rc != GLC_OK) return rc;
  }
  for (uint64_t f0 = hop_begin; f0 < hop_end;) {
    const uint64_t nchunk = f0 < f_end ? std::min(chunk, f_end - f0) : 0;
    const bool tail = f0 + nchunk == nf && hop_end == nf + 1;  // this round also emits the bare overlap tail
    const uint64_t next = f0 + nchunk + (tail ? 1 : 0);
    const int rc = decode_round(ctx, f0, nchunk, tail, /*carry=*/next < hop_end, d_out + (f0 - hop_begin) * glc::kHop * ch);
    if (rc != GLC_OK) return rc;
    f0 = next;
  }
  return GLC_OK;
}

// Copies a finished device buffer out behind the event its kernels recorded: `cs` waits for the event, takes the
// `n` samples and is drained.  On ctx->stream itself - what follows the kernels in stream order - there is no wait.
template <typename T>
int copy_out_behind(glc_ctx *ctx, const Event &done, hipStream_t cs, T *dst, const T *src, uint64_t n) {
  if (cs != ctx->stream) GLC_HIP(ctx, hipStreamWaitEvent(cs, done, 0));
  if (n) GLC_HIP(ctx, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, cs));
  GLC_HIP(ctx, hipStreamSynchronize(cs));
  return GLC_OK;
}

// Decoder::decode of the prepared session into host memory (src/codec.rs:744-768).
template <typename T>
int decode_prepared_to_host(glc_ctx *ctx, T *pcm_out, uint64_t cap, uint64_t *n_out, const char *who) {
  const uint64_t n_frames = ctx->dec_frames;
  const uint32_t channels = ctx->dec_ch;
  const glc::Trim trim = glc::gapless_trim(n_frames, channels, ctx->dec_delay, ctx->dec_orig_len);
  if (n_out) *n_out = trim.n;
  if (cap < trim.n) return fail(ctx, GLC_EINVAL, std::string(who) + ": output buffer too small");
  ctx->dec_next = 0;
  // Rounds of 4096 frames through two device output buffers: the kernels of round r+1 are queued
  // before round r is copied out (on the copy stream, behind that round's event), so the D2H of
  // one round overlaps the decode of the next.  The block ring is sized once: slot 0 carries state.
  const uint64_t round = std::max<uint64_t>(1, std::min<uint64_t>(kDecodeChunkFrames, n_frames));
  const uint64_t per_hop = static_cast<uint64_t>(glc::kHop) * channels;
  const size_t bufcap = static_cast<size_t>(round + 1) * per_hop;  // samples per output buffer
  {
    DeviceGuard guard(ctx->device);
    GLC_HIP(ctx, ctx->blocks.reserve((round + 1) * static_cast<size_t>(channels) * glc::kFrame * sizeof(float)));
    GLC_HIP(ctx, ctx->pcm.reserve(2 * bufcap * sizeof(T)));
  }
  int rc = ensure_copy_objects(ctx);
  if (rc != GLC_OK) return rc;
  DeviceGuard guard(ctx->device);
  T *stage = static_cast<T *>(ctx->pcm.p);
  int buf = 0;
  uint64_t f0 = 0, frames = 0;
  bool last = false;
  rc = round_launch(ctx, round, false, stage, ctx->ev_dec[0], &frames, &last);
  if (rc != GLC_OK) return rc;
  for (;;) {
    const uint64_t cur_f0 = f0, cur_frames = frames;
    const bool cur_last = last;
    if (!cur_last) {
      f0 += frames;
      rc = round_launch(ctx, round, false, stage + static_cast<size_t>(buf ^ 1) * bufcap, ctx->ev_dec[buf ^ 1], &frames, &last);
      if (rc != GLC_OK) return rc;
    }
    const glc::OutSpan out = glc::decode_round_span(trim, per_hop, cur_f0, cur_frames, cur_last);
    // a stream of a single round (short clips) has nothing to overlap: copy in stream order
    hipStream_t cs = (cur_last && cur_f0 == 0) ? ctx->stream : ctx->copy_stream;
    const T *from = stage + static_cast<size_t>(buf) * bufcap + (out.hi > out.lo ? out.lo - cur_f0 * per_hop : 0);
    rc = copy_out_behind(ctx, ctx->ev_dec[buf], cs, pcm_out + (out.lo - trim.start), from, out.hi - out.lo);
    if (rc != GLC_OK) return rc;
    if (cur_last) break;
    buf ^= 1;
  }
  return GLC_OK;
}

// ---- the hop descriptors of the descriptor overlap-add (glc::HopDescStrided), as every batch driver writes them

// The descriptors of hops [h0, h1) of a clip of `nf` frames whose frame f is block slot base + f: one per hop that
// the clip's trim keeps something of, in hop order.  The kept samples land from element `dst` on, interleaved, or
// (planes) in planes `cstride` apart.
glc::HopDescStrided *write_hop_descs(glc::HopDescStrided *d, uint64_t nf, uint32_t ch, const glc::Trim &trim, uint64_t h0,
                                     uint64_t h1, int64_t base, uint64_t dst, bool planes, uint64_t cstride) {
  for (uint64_t h = h0; h < h1; ++h)
    if (glc::hop_desc(d, nf, ch, trim, h, base, dst, planes, cstride)) ++d;  // glc_kernels.h: the one statement of a descriptor
  return d;
}

// How many descriptors write_hop_descs makes of hops [h0, h1): a hop keeps something exactly when it lies from the
// hop of the first kept sample to the hop of the last one.
inline uint64_t count_hop_descs(const glc::Trim &trim, uint64_t per_hop, uint64_t h0, uint64_t h1) {
  if (trim.n == 0) return 0;
  const uint64_t lo = std::max(h0, trim.start / per_hop), hi = std::min(h1, (trim.start + trim.n - 1) / per_hop + 1);
  return hi > lo ? hi - lo : 0;
}

// All descriptors of one clip of a batch round.  `lng` (the one clip of a round of its own, longer than a decode
// round): round by round, block slots counted in the ring (frame f0 - 1 of a round in slot 0); otherwise flat, the
// clip's frame 0 in block slot `real`.  `win` (a crop, `trim` what it keeps): only the window's frames have blocks -
// its first frame is the one in slot `real`, or the first of the ring rounds - and only its hops are described.
glc::HopDescStrided *write_clip_descs(glc::HopDescStrided *d, bool lng, uint64_t nf, uint32_t ch, const glc::Trim &trim,
                                      uint64_t real, uint64_t dst, bool planes, uint64_t cstride, const glc_crop_plan *win = nullptr) {
  const uint64_t fb = win ? win->first_frame : 0, fe = win ? fb + win->n_frames : nf;
  if (!lng) {
    const uint64_t h0 = win ? win->first_hop : 0, h1 = win ? h0 + win->n_hops : nf + 1;
    return write_hop_descs(d, nf, ch, trim, h0, h1, static_cast<int64_t>(real) - static_cast<int64_t>(fb), dst, planes, cstride);
  }
  for (uint64_t f0 = fb; f0 < fe; f0 += kDecodeChunkFrames) {
    const uint64_t f1 = std::min(fe, f0 + kDecodeChunkFrames);
    d = write_hop_descs(d, nf, ch, trim, f0, f1 + (f1 == nf ? 1 : 0), 1 - static_cast<int64_t>(f0), dst, planes, cstride);
  }
  return d;
}

// One round of glc_decode_batch: streams[0 .. n) (all of `ch` channels, together at most a round's frames)
// through D1 as one row table, then the segment-aware overlap-add, which writes every stream's TRIMMED
// samples back to back, and one copy of them to pcm_out.  lens[i]: glc_decoded_len of stream i.
// T: float (glc_decode_batch) or int16_t (glc_decode_batch_i16: narrowed by the overlap-add itself).
template <typename T>
int decode_batch_round(glc_ctx *ctx, const glc_frames *const *streams, uint64_t n, uint32_t ch, const uint64_t *lens,
                       T *pcm_out) {
  uint64_t frames = 0, n_out = 0;
  for (uint64_t i = 0; i < n; ++i) frames += streams[i]->n_frames, n_out += lens[i];
  const uint64_t M = frames * ch;
  int rc = reserve_d1_plan(ctx, frames, ch);
  if (rc != GLC_OK) return rc;
  RowTable t;
  rc = build_row_table(ctx, "glc_decode_batch", streams, n, ch, M, t);
  if (rc != GLC_OK) return rc;
  // a descriptor per output hop that the stream's gapless trim keeps something of
  std::vector<glc::HopDesc> desc;
  {
    std::vector<glc::HopDescStrided> wide(frames + n);  // at most a hop per frame and a tail per stream
    glc::HopDescStrided *d = wide.data();
    uint64_t slot0 = 0, dst0 = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const glc_frames *in = streams[i];
      const glc::Trim trim = glc::gapless_trim(in->n_frames, ch, in->encoder_delay, in->original_length);
      d = write_hop_descs(d, in->n_frames, ch, trim, 0, in->n_frames + 1, static_cast<int64_t>(slot0), dst0, false, 0);
      slot0 += in->n_frames;
      dst0 += trim.n;
    }
    // uploaded in the 24-byte form: a round's output is addressed in 31 bits (decode_batch_impl's hop_budget)
    for (const glc::HopDescStrided *w = wide.data(); w != d; ++w)
      desc.push_back(glc::HopDesc{w->prev, w->cur, static_cast<uint32_t>(w->dst), w->first, w->cnt, 0u});
  }
  // everything D1 and D2 read, as ONE image in pinned memory and one copy: the pairs of all streams, the
  // canonicalised lists, the row arrays, the raw pool, the hop descriptors
  TableOffsets offs;
  const size_t o_pairs = offs.take(std::max<size_t>(t.n_stored + t.extra.size(), 1) * 4);
  const size_t o_rows = offs.take(t.h_end);
  const size_t o_pool = offs.take(std::max<size_t>(t.n_raw, 1) * 2);
  const size_t o_desc = offs.take(std::max<size_t>(desc.size(), 1) * sizeof(glc::HopDesc));
  DeviceGuard guard(ctx->device);
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a previous session may still read dec_meta
  GLC_HIP(ctx, ctx->dec_meta.reserve(offs.size()));
  GLC_HIP(ctx, ctx->batch_stage.reserve(offs.size()));
  GLC_HIP(ctx, ctx->blocks.reserve(std::max<size_t>(frames, 1) * slot * sizeof(float)));
  GLC_HIP(ctx, ctx->pcm.reserve(std::max<size_t>(n_out, 1) * sizeof(T)));
  uint8_t *img = static_cast<uint8_t *>(ctx->batch_stage.p);
  {
    uint8_t *p = img + o_pairs;
    int16_t *r = reinterpret_cast<int16_t *>(img + o_pool);
    for (uint64_t i = 0; i < n; ++i) {
      const glc_frames *in = streams[i];
      if (!in->pairs.empty()) std::memcpy(p, in->pairs.data(), in->pairs.size() * 4);
      p += in->pairs.size() * 4;
      if (!in->raw.empty()) std::memcpy(r, in->raw.data(), in->raw.size() * 2);
      r += in->raw.size();
    }
    if (!t.extra.empty()) std::memcpy(p, t.extra.data(), t.extra.size() * 4);
    std::memcpy(img + o_rows, t.block.data(), t.h_end);
    if (!desc.empty()) std::memcpy(img + o_desc, desc.data(), desc.size() * sizeof(glc::HopDesc));
  }
  uint8_t *mb = static_cast<uint8_t *>(ctx->dec_meta.p);
  GLC_HIP(ctx, hipMemcpyAsync(mb, img, offs.size(), hipMemcpyHostToDevice, ctx->stream));
  const glc::DecodeRows rows{reinterpret_cast<const uint32_t *>(mb + o_pairs),
                             reinterpret_cast<const uint64_t *>(mb + o_rows + t.h_begin),
                             reinterpret_cast<const uint32_t *>(mb + o_rows + t.h_cnt),
                             reinterpret_cast<const float *>(mb + o_rows + t.h_scale),
                             reinterpret_cast<const int64_t *>(mb + o_rows + t.h_raw),
                             reinterpret_cast<const uint64_t *>(mb + o_rows + t.h_rawlen),
                             reinterpret_cast<const int16_t *>(mb + o_pool), t.any_raw};
  float *blocks = static_cast<float *>(ctx->blocks.p);
  T *stage = static_cast<T *>(ctx->pcm.p);
  // (D1's 8-frame units may span two streams: that only widens a union)
  GLC_HIP(ctx, launch_d1_rows(ctx, rows, 0, static_cast<uint32_t>(M), ch, blocks, ctx->stream));
  GLC_HIP(ctx, glc::launch_overlap_add_strided(blocks, reinterpret_cast<const glc::HopDesc *>(mb + o_desc),
                                               static_cast<uint32_t>(desc.size()), ch, stage, ctx->stream));
  if (n_out) GLC_HIP(ctx, hipMemcpyAsync(pcm_out, stage, n_out * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GLC_OK;
}

template <typename T>
int decode_batch_impl(glc_ctx *ctx, const char *who, const glc_frames *const *in, uint64_t n_streams, T *pcm_out,
                      const uint64_t *offsets) {
  const uint32_t ch = in[0]->channels;
  const uint64_t per_hop = static_cast<uint64_t>(glc::kHop) * ch;
  // a round: whole streams of together at most kDecodeChunkFrames frames (+ one tail hop each), its output
  // addressed in 32 bits
  const uint64_t hop_budget = std::min<uint64_t>(kDecodeChunkFrames + 1, 0x7FFFFFFFull / per_hop);
  const auto rounds = pack_rounds(n_streams, [&](uint64_t i) { return in[i]->n_frames; }, hop_budget, 0);
  int rc = GLC_OK;
  for (size_t k = 0; k < rounds.size() && rc == GLC_OK; ++k) {
    const uint64_t first = rounds[k].first, end = first + rounds[k].n;
    if (end == first + 1) {  // longer than a round, or a round to itself: the single-stream driver, straight into the stream's span
      rc = decode_prepare(ctx, in[first]);
      if (rc == GLC_OK)
        rc = decode_prepared_to_host(ctx, pcm_out + offsets[first], offsets[end] - offsets[first], nullptr, who);
      ctx->dec_uid = 0;  // a batch decode leaves no stream resident
      ctx->plan_uid = 0;
    } else {
      std::vector<uint64_t> lens(end - first);
      for (uint64_t i = first; i < end; ++i) lens[i - first] = offsets[i + 1] - offsets[i];
      rc = decode_batch_round(ctx, in + first, end - first, ch, lens.data(), pcm_out + offsets[first]);
    }
  }
  return rc;
}

// glc_decode / glc_decode_i16
template <typename T>
int decode_to_host(glc_ctx *ctx, const glc_frames *in, T *pcm_out, uint64_t cap, uint64_t *n_out, const char *who) {
  if (!ctx || !in || (!pcm_out && cap)) return fail(ctx, GLC_EINVAL, std::string(who) + ": null argument");
  ctx->stream_open = false;
  if (n_out) *n_out = glc_decoded_len(in);
  if (cap < glc_decoded_len(in)) return fail(ctx, GLC_EINVAL, std::string(who) + ": output buffer too small");
  const int rc = decode_prepare(ctx, in);
  if (rc != GLC_OK) return rc;
  return decode_prepared_to_host(ctx, pcm_out, cap, n_out, who);
}

// glc_decode_range_device / glc_decode_range_device_i16
template <typename T>
int decode_range_device(glc_ctx *ctx, const glc_frames *in, uint64_t hop_begin, uint64_t hop_end, T *d_out, uint64_t cap,
                        const char *who) {
  if (!ctx || !in || !d_out) return fail(ctx, GLC_EINVAL, std::string(who) + ": null argument");
  ctx->stream_open = false;
  if (hop_begin > hop_end || hop_end > in->n_frames + 1)
    return fail(ctx, GLC_EINVAL, std::string(who) + ": hop range out of bounds");
  if (cap < (hop_end - hop_begin) * glc::kHop * in->channels)
    return fail(ctx, GLC_EINVAL, std::string(who) + ": output buffer too small");
  if (!aligned(d_out, sizeof(T)))
    return fail(ctx, GLC_EINVAL, std::string(who) + ": output pointer not aligned to its sample size");
  int rc = decode_prepare(ctx, in);
  if (rc != GLC_OK) return rc;
  return decode_hops_prepared(ctx, hop_begin, hop_end, d_out);
}

// glc_decode_stream_next / glc_decode_stream_next_i16.  glc_decode_stream_begin cannot know which of
// the two will read the stream and queues the first chunk as floats; a stream read as int16_t queues
// that one chunk again (its plan records are still in place) before it goes on as the float one does.
template <typename T>
int decode_stream_next(glc_ctx *ctx, T *chunk, uint64_t cap, uint64_t *n_out, int *is_last) {
  if (!ctx || !n_out || !is_last) return fail(ctx, GLC_EINVAL, "glc_decode_stream_next: null argument");
  if (!ctx->stream_open) return fail(ctx, GLC_EINVAL, "glc_decode_stream_next: no stream open");
  if (ctx->stream_elem != 0 && ctx->stream_elem != static_cast<int>(sizeof(T)))
    return fail(ctx, GLC_EINVAL, "glc_decode_stream_next: this stream is being read in the other sample format");
  const int buf = ctx->stream_buf;
  const size_t bufcap = (static_cast<size_t>(GLC_FRAMES_PER_CHUNK) + 1) * glc::kHop * ctx->dec_ch;
  T *stage = static_cast<T *>(ctx->stream_out.p);
  if (ctx->stream_elem == 0 && sizeof(T) != sizeof(float)) {
    ctx->dec_next = 0;
    const int rc = round_launch(ctx, GLC_FRAMES_PER_CHUNK, true, stage + static_cast<size_t>(buf) * bufcap, ctx->ev_dec[buf],
                                &ctx->stream_frames, &ctx->stream_last);
    if (rc != GLC_OK) {
      ctx->stream_open = false;
      return rc;
    }
  }
  const bool last = ctx->stream_last;
  const uint64_t per_hop = static_cast<uint64_t>(glc::kHop) * ctx->dec_ch;
  const uint64_t n = (ctx->stream_frames + (last ? 1 : 0)) * per_hop;
  *n_out = n;
  *is_last = last ? 1 : 0;
  ctx->stream_elem = static_cast<int>(sizeof(T));
  if (cap < n || (!chunk && n)) return fail(ctx, GLC_EINVAL, "glc_decode_stream_next: chunk buffer too small");
  DeviceGuard guard(ctx->device);
  // double buffering: the kernels of the following chunk are queued first, then this chunk is
  // copied out on the copy stream as soon as its own kernels have finished
  if (!last) {
    const int rc = round_launch(ctx, GLC_FRAMES_PER_CHUNK, true, stage + static_cast<size_t>(buf ^ 1) * bufcap,
                                ctx->ev_dec[buf ^ 1], &ctx->stream_frames, &ctx->stream_last);
    if (rc != GLC_OK) return rc;
  }
  const int rc = copy_out_behind(ctx, ctx->ev_dec[buf], ctx->copy_stream, chunk, stage + static_cast<size_t>(buf) * bufcap, n);
  if (rc != GLC_OK) return rc;
  ctx->stream_buf = buf ^ 1;
  if (last) ctx->stream_open = false;
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

int glc_decode(glc_ctx *ctx, const glc_frames *in, float *pcm_out, uint64_t cap, uint64_t *n_out) {
  return decode_to_host(ctx, in, pcm_out, cap, n_out, "glc_decode");
}

int glc_decode_i16(glc_ctx *ctx, const glc_frames *in, int16_t *pcm_out, uint64_t cap, uint64_t *n_out) {
  return decode_to_host(ctx, in, pcm_out, cap, n_out, "glc_decode_i16");
}

extern "C++" {
namespace {
// glc_decode_batch / glc_decode_batch_i16
template <typename T>
int decode_batch_to_host(glc_ctx *ctx, const char *who, const glc_frames *const *in, uint64_t n_streams, T *pcm_out, uint64_t cap,
                         uint64_t *offsets) {
  const std::string w(who);
  if (!ctx) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (n_streams == 0) {
    if (offsets) offsets[0] = 0;
    return GLC_OK;
  }
  if (!in || !offsets || (!pcm_out && cap)) return fail(ctx, GLC_EINVAL, w + ": null argument");
  offsets[0] = 0;
  for (uint64_t i = 0; i < n_streams; ++i) {
    if (!in[i]) return fail(ctx, GLC_EINVAL, w + ": stream " + std::to_string(i) + ": null pointer");
    offsets[i + 1] = offsets[i] + glc_decoded_len(in[i]);
  }
  if (in[0]->channels == 0) return fail(ctx, GLC_EINVAL, w + ": header.channels == 0");
  for (uint64_t i = 1; i < n_streams; ++i)
    if (in[i]->channels != in[0]->channels)
      return fail(ctx, GLC_EINVAL,
                  w + ": stream " + std::to_string(i) + " has " + std::to_string(in[i]->channels) +
                      " channels, stream 0 has " + std::to_string(in[0]->channels));
  if (cap < offsets[n_streams]) return fail(ctx, GLC_EINVAL, w + ": output buffer too small");
  // no stream is resident afterwards: the row tables on the device are a round's, not a stream's
  ctx->stream_open = false;
  ctx->dec_uid = 0;
  ctx->plan_uid = 0;
  int rc;
  try {  // no C++ exception may cross the C ABI
    rc = decode_batch_impl(ctx, who, in, n_streams, pcm_out, offsets);
  } catch (const std::bad_alloc &) {
    rc = fail(ctx, GLC_ENOMEM, w + ": host allocation failed");
  }
  if (rc != GLC_OK) {
    DeviceGuard guard(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);  // nothing may still be in flight into the caller's memory
  }
  return rc;
}
}  // namespace
}  // extern "C++"

int glc_decode_batch(glc_ctx *ctx, const glc_frames *const *in, uint64_t n_streams, float *pcm_out, uint64_t cap,
                     uint64_t *offsets) {
  return decode_batch_to_host(ctx, "glc_decode_batch", in, n_streams, pcm_out, cap, offsets);
}

int glc_decode_batch_i16(glc_ctx *ctx, const glc_frames *const *in, uint64_t n_streams, int16_t *pcm_out, uint64_t cap,
                         uint64_t *offsets) {
  return decode_batch_to_host(ctx, "glc_decode_batch_i16", in, n_streams, pcm_out, cap, offsets);
}

// ------------------------------------------------------------------------------ round trip

extern "C++" {
namespace {

// Grow a workspace of the round trip.  Work queued earlier may still use the old allocation: the stream is
// drained first - only when the buffer has to grow, so that a repeated call of the same size only queues.
int rt_reserve(glc_ctx *ctx, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return GLC_OK;
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  GLC_HIP(ctx, b.reserve(bytes));
  return GLC_OK;
}

// A decode of `n_frames` frames of `ch` channels from records on the device, in rounds of `round` frames, into
// the samples `trim` keeps.
struct RtGeom {
  uint32_t ch;
  uint64_t n_frames, round, per_hop;
  glc::Trim trim;
};

// Every call of the family: no decode session survives it, no stream is resident afterwards.
void rt_forget_streams(glc_ctx *ctx) {
  ctx->stream_open = false;
  ctx->dec_uid = 0;
  ctx->plan_uid = 0;
}

// Workspaces of the decode half of a round.
int rt_prepare(glc_ctx *ctx, const RtGeom &g) {
  const size_t slot = static_cast<size_t>(g.ch) * glc::kFrame;
  int rc = rt_reserve(ctx, ctx->blocks, (g.round + 1) * slot * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_records_bytes(static_cast<uint32_t>(g.round * g.ch)));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_edge, 2 * g.per_hop * sizeof(float));
  if (rc == GLC_OK) rc = reserve_d1_plan(ctx, g.round, g.ch);
  return rc;
}

// Hops [h0, h1) of the un-trimmed stream, whose frames are in the block ring (frame h0 - 1 in slot 0), into
// the TRIMMED output: hops that lie inside the kept window [trim.start, trim.start + trim.n) are
// overlap-added straight to their place in d_out; the at most two hops the window cuts go through a
// hop-sized buffer, and only their kept part is copied on.  Nothing outside d_out[0 .. trim.n) is written.
template <typename T>
int rt_emit_hops(glc_ctx *ctx, const RtGeom &g, uint64_t h0, uint64_t h1, T *d_out) {
  const float *blocks = static_cast<const float *>(ctx->blocks.p);
  const int64_t blk0 = static_cast<int64_t>(h0) - 1;
  const uint64_t lo = g.trim.start, hi = g.trim.start + g.trim.n;
  if (g.trim.n == 0) return GLC_OK;
  const uint64_t full_lo = std::max(h0, (lo + g.per_hop - 1) / g.per_hop), full_hi = std::min(h1, hi / g.per_hop);
  if (full_hi > full_lo)
    GLC_HIP(ctx, glc::launch_overlap_add(blocks, blk0, g.n_frames, g.ch, full_lo, full_hi, d_out + (full_lo * g.per_hop - lo),
                                         ctx->stream));
  const uint64_t cut[2] = {lo / g.per_hop, hi / g.per_hop};  // the hops that hold the window's two ends
  for (int i = 0; i < 2; ++i) {
    const uint64_t h = cut[i];
    if (h < h0 || h >= h1 || (i == 1 && cut[1] == cut[0])) continue;
    if (h >= full_lo && h < full_hi) continue;  // an end on a hop boundary cuts nothing
    const uint64_t a = std::max(lo, h * g.per_hop), b = std::min(hi, (h + 1) * g.per_hop);
    if (b <= a) continue;
    T *edge = static_cast<T *>(ctx->rt_edge.p) + static_cast<size_t>(i) * g.per_hop;
    GLC_HIP(ctx, glc::launch_overlap_add(blocks, blk0, g.n_frames, g.ch, h, h + 1, edge, ctx->stream));
    GLC_HIP(ctx, hipMemcpyAsync(d_out + (a - lo), edge + (a - h * g.per_hop), (b - a) * sizeof(T), hipMemcpyDeviceToDevice,
                                ctx->stream));
  }
  return GLC_OK;
}

// One round: the records of frames [f0, f0 + nf) at `recs` -> row tables (R1) -> D1 into block slots 1.. ->
// the round's hops (+ the bare tail behind the last frame) into the trimmed output -> the last block to
// slot 0 for the next round.  `stats`: device counters of glc_roundtrip_last_info, or null.
// `sink` (glc_roundtrip_batch_device, a clip longer than a round): the round's hops go through the strided
// overlap-add by these descriptors (block slots counted in the ring) instead of into a contiguous d_out.
template <typename T>
struct RtStridedSink {
  const glc::HopDescStrided *desc;
  uint32_t n_desc;
  bool planar;
  T *out;  // float, or int16_t: the strided overlap-add narrows on the way out
};
// ... from row `row0` on of row tables that are on the device (R1 of the round's records, or R2 of a whole blob)
template <typename T>
int rt_decode_round_rows(glc_ctx *ctx, const RtGeom &g, const glc::DecodeRows &rows, uint32_t row0, uint64_t f0, uint64_t nf,
                         T *d_out, const RtStridedSink<T> *sink) {
  const size_t slot = static_cast<size_t>(g.ch) * glc::kFrame;
  float *blocks = static_cast<float *>(ctx->blocks.p);
  const uint32_t M = static_cast<uint32_t>(nf * g.ch);
  GLC_HIP(ctx, launch_d1_rows(ctx, rows, row0, M, g.ch, blocks + slot, ctx->stream));
  const bool last = f0 + nf == g.n_frames;
  if (sink) {
    GLC_HIP(ctx, glc::launch_overlap_add_strided(blocks, sink->desc, sink->n_desc, g.ch, sink->planar, sink->out, ctx->stream));
  } else {
    const int rc = rt_emit_hops(ctx, g, f0, f0 + nf + (last ? 1 : 0), d_out);
    if (rc != GLC_OK) return rc;
  }
  if (!last)
    GLC_HIP(ctx, hipMemcpyAsync(blocks, blocks + nf * slot, slot * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  return GLC_OK;
}
template <typename T>
int rt_decode_round(glc_ctx *ctx, const RtGeom &g, const uint8_t *recs, uint64_t f0, uint64_t nf, uint64_t *stats, T *d_out,
                    const RtStridedSink<T> *sink = nullptr) {
  glc::DecodeRows rows{};
  GLC_HIP(ctx, glc::launch_rows_from_records(recs, static_cast<uint32_t>(nf * g.ch), g.ch, ctx->rt_rows.p, stats, ctx->stream, &rows));
  return rt_decode_round_rows(ctx, g, rows, 0, f0, nf, d_out, sink);
}

RtGeom rt_geom(uint64_t n_frames, uint32_t ch, const glc_plan &plan, uint64_t n_samples) {
  RtGeom g;
  g.ch = ch;
  g.n_frames = n_frames;
  g.round = std::max<uint64_t>(1, std::min<uint64_t>(kDecodeChunkFrames, n_frames));
  g.per_hop = static_cast<uint64_t>(glc::kHop) * ch;
  g.trim = glc::gapless_trim(n_frames, ch, plan.encoder_delay, n_samples);
  return g;
}

// Arguments every call of the family checks the same way.  *n_out is filled before the capacity is judged.
int rt_check(glc_ctx *ctx, const char *who, uint64_t n_samples, uint16_t channels, const void *out, size_t out_align,
             uint64_t cap, uint64_t *n_out, glc_plan *plan, RtGeom *g) {
  const std::string w(who);
  if (channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  if (const char *bad = frames_fault(n_samples, channels, plan)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  *g = rt_geom(plan->n_frames, channels, *plan, n_samples);
  if (n_out) *n_out = g->trim.n;
  if (cap < g->trim.n) return fail(ctx, GLC_EINVAL, w + ": output buffer too small");
  if (!out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (!aligned(out, out_align)) return fail(ctx, GLC_EINVAL, w + ": output pointer not aligned to its sample size");
  return GLC_OK;
}

// Encode + decode of the frames [f0, f0 + nf) of device-resident PCM: K1, K2 (K3) into the round's record
// buffer, then rt_decode_round of it.
template <typename T>
int rt_roundtrip_round(glc_ctx *ctx, const RtGeom &g, const float *d_pcm, uint64_t n_samples, uint64_t f0, uint64_t nf, T *d_out,
                       uint64_t *stats, const RtStridedSink<T> *sink = nullptr) {
  const uint64_t t_count = (n_samples + g.ch - 1) / g.ch;
  int rc = encode_range_on(ctx, ctx->stream,
                           EncodeRange{{d_pcm, 0, t_count, n_samples, g.ch}, f0, f0 + nf, ctx->rt_records.p, nullptr, &ctx->slot[0]});
  if (rc != GLC_OK) return rc;
  return rt_decode_round(ctx, g, static_cast<const uint8_t *>(ctx->rt_records.p), f0, nf, stats, d_out, sink);
}

constexpr size_t kRtStatBytes = size_t(glc::kRowStatSlots) * glc::kRowStatStride * sizeof(uint64_t);

// Workspaces of the encode half and the counters; the counters are zeroed in stream order.
int rt_roundtrip_begin(glc_ctx *ctx, const RtGeom &g) {
  ctx->rt_info_frames = 0;
  int rc = rt_prepare(ctx, g);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_records, g.round * glc::record_bytes(g.ch));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->coef, g.round * g.ch * glc::kHop * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_stats, kRtStatBytes);
  if (rc != GLC_OK) return rc;
  GLC_HIP(ctx, hipMemsetAsync(ctx->rt_stats.p, 0, kRtStatBytes, ctx->stream));
  return GLC_OK;
}

void rt_roundtrip_end(glc_ctx *ctx, const RtGeom &g) {
  ctx->rt_info_frames = g.n_frames;
  ctx->rt_info_ch = g.ch;
}

// glc_roundtrip behind its argument checks.  T: sample type of the output.
template <typename T>
int rt_roundtrip_host(glc_ctx *ctx, const void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples, const RtGeom &g,
                      const glc_plan &plan, T *pcm_out) {
  int rc = rt_roundtrip_begin(ctx, g);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->pcm, static_cast<size_t>(n_samples) * sizeof(float));
  if (rc == GLC_OK && fmt != GLC_PCM_F32) rc = rt_reserve(ctx, ctx->pcm_int, static_cast<size_t>(n_samples) * pcm_elem(fmt));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_out, std::max<size_t>(g.trim.n, 1) * sizeof(T));
  if (rc == GLC_OK) rc = ensure_copy_objects(ctx);
  if (rc != GLC_OK) return rc;
  GLC_HIP(ctx, ctx->down_stream.ensure());
  // the staging buffers are shared with the other host-boundary calls, some of which work on streams of their own
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float *d_pcm = static_cast<float *>(ctx->pcm.p);
  T *d_out = static_cast<T *>(ctx->rt_out.p);
  const uint64_t n_rounds = fixed_round_count(g.n_frames, g.round);
  auto mark_of = [&](size_t i) {
    const StreamRound r = fixed_round(g.n_frames, g.round, i);
    return glc::upload_mark(r.f0, r.nf, plan.per_channel, g.ch, n_samples);
  };
  // Three stages, as in glc_encode: round i + 1's samples go up (copy stream; a helper thread when there is more
  // than one round, because a copy from pageable memory blocks its caller), round i's kernels run, round i - 1's
  // output comes down (download stream, this thread) - PCIe carries both directions at once.  A stage waits on
  // the HOST for what it depends on and only then queues (nothing is queued behind an unfinished dependency);
  // copies from and to pageable memory have completed when they return.
  StageGate gate;
  auto upload = [&] {
    upload_rounds(ctx, "glc_roundtrip", gate, kUploaded, n_rounds, mark_of, pcm, fmt, bits, d_pcm, static_cast<uint8_t *>(ctx->pcm_int.p),
                  ctx->copy_stream, true);
  };
  auto download = [&](uint64_t i) -> hipError_t {  // the trimmed samples round i wrote
    const StreamRound r = fixed_round(g.n_frames, g.round, i);
    const glc::OutSpan out = glc::decode_round_span(g.trim, g.per_hop, r.f0, r.nf, r.f0 + r.nf == g.n_frames);
    hipError_t e = hipEventSynchronize(ctx->ev_dec[i & 1]);
    if (e == hipSuccess && out.hi > out.lo)
      e = hipMemcpyAsync(pcm_out + (out.lo - g.trim.start), d_out + (out.lo - g.trim.start), (out.hi - out.lo) * sizeof(T),
                         hipMemcpyDeviceToHost, ctx->down_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->down_stream);
    return e;
  };
  auto rounds = [&]() -> int {
    for (uint64_t i = 0; i < n_rounds; ++i) {
      if (!gate.wait_for(kUploaded, i)) return fail(ctx, gate.code(), gate.message());
      const StreamRound r = fixed_round(g.n_frames, g.round, i);
      const int rrc = rt_roundtrip_round(ctx, g, d_pcm, n_samples, r.f0, r.nf, d_out, static_cast<uint64_t *>(ctx->rt_stats.p));
      if (rrc != GLC_OK) return rrc;
      GLC_HIP(ctx, hipEventRecord(ctx->ev_dec[i & 1], ctx->stream));
      if (i > 0) GLC_HIP(ctx, download(i - 1));
    }
    GLC_HIP(ctx, download(n_rounds - 1));
    return GLC_OK;
  };
  if (n_rounds == 1)
    run_stages(gate, "glc_roundtrip", {}, [&] { upload(), rc = rounds(); });
  else
    run_stages(gate, "glc_roundtrip", {{ctx->enc_up, std::ref(upload)}}, [&] { rc = rounds(); });
  if (rc == GLC_OK && gate.failed()) rc = fail(ctx, gate.code(), gate.message());  // no helper thread, or an exception in the body
  if (rc != GLC_OK) return rc;
  rt_roundtrip_end(ctx, g);
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

// glc_roundtrip_info of a stream of `nf` frames of `ch` channels from its two device counters
static void rt_fill_info(glc_roundtrip_info *out, uint64_t nf, uint64_t ch, uint64_t nnz, uint64_t n_raw) {
  const uint64_t lists = (nf - n_raw) * ch;
  out->n_frames = nf;
  out->n_raw_frames = n_raw;
  out->total_nnz = nnz;
  // glc_serialized_size: header, per frame {two Vec lengths, Option tag}, per list its length, the pairs and
  // scale factors of compressed frames, {length, planar i16 block} of raw ones, gapless info
  out->serialized_bytes = (4 + 2 + 8 + 8) + nf * (8 + 8 + 1) + lists * 8 + nnz * 4 + lists * 4 +
                          n_raw * (8 + 2ull * glc::kFrame * ch) + (4 + 4 + 8);
}

int glc_decode_device_records(glc_ctx *ctx, const void *d_records, uint64_t n_frames, uint64_t n_samples, uint16_t channels,
                              float *d_out, uint64_t cap, uint64_t *n_out) {
  if (!ctx) return GLC_EINVAL;
  if (n_out) *n_out = 0;
  if (!d_records) return fail(ctx, GLC_EINVAL, "glc_decode_device_records: null argument");
  if (!aligned(d_records, 16)) return fail(ctx, GLC_EINVAL, "glc_decode_device_records: the records are not 16-byte aligned");
  glc_plan plan;
  RtGeom g;
  int rc = rt_check(ctx, "glc_decode_device_records", n_samples, channels, d_out, sizeof(float), cap, n_out, &plan, &g);
  if (rc == GLC_OK && plan.n_frames != n_frames) {
    if (n_out) *n_out = 0;
    rc = fail(ctx, GLC_EINVAL, "glc_decode_device_records: record count does not match the stream length");
  }
  if (rc != GLC_OK) return rc;
  DeviceGuard guard(ctx->device);
  rt_forget_streams(ctx);
  rc = rt_prepare(ctx, g);
  const uint64_t rec = glc::record_bytes(channels);
  for (uint64_t f0 = 0; f0 < n_frames && rc == GLC_OK; f0 += g.round)
    rc = rt_decode_round(ctx, g, static_cast<const uint8_t *>(d_records) + f0 * rec, f0, std::min(g.round, n_frames - f0), nullptr,
                         d_out);
  return rc;
}

int glc_roundtrip_device(glc_ctx *ctx, const float *d_pcm, uint64_t n_samples, uint16_t channels, float *d_out, uint64_t cap,
                         uint64_t *n_out) {
  if (!ctx) return GLC_EINVAL;
  if (n_out) *n_out = 0;
  if (!d_pcm) return fail(ctx, GLC_EINVAL, "glc_roundtrip_device: null argument");
  glc_plan plan;
  RtGeom g;
  int rc = rt_check(ctx, "glc_roundtrip_device", n_samples, channels, d_out, sizeof(float), cap, n_out, &plan, &g);
  if (rc != GLC_OK) return rc;
  DeviceGuard guard(ctx->device);
  rt_forget_streams(ctx);
  rc = rt_roundtrip_begin(ctx, g);
  for (uint64_t f0 = 0; f0 < g.n_frames && rc == GLC_OK; f0 += g.round)
    rc = rt_roundtrip_round(ctx, g, d_pcm, n_samples, f0, std::min(g.round, g.n_frames - f0), d_out,
                            static_cast<uint64_t *>(ctx->rt_stats.p));
  if (rc == GLC_OK) rt_roundtrip_end(ctx, g);
  return rc;
}

int glc_roundtrip(glc_ctx *ctx, const void *pcm, glc_pcm_format fmt, uint32_t bits, uint64_t n_samples, uint16_t channels,
                  void *pcm_out, glc_pcm_format out_fmt, uint64_t cap, uint64_t *n_out) {
  if (!ctx) return GLC_EINVAL;
  if (n_out) *n_out = 0;
  if (!pcm) return fail(ctx, GLC_EINVAL, "glc_roundtrip: null argument");
  if (const char *bad = fmt_fault(fmt, bits)) return fail(ctx, GLC_EINVAL, std::string("glc_roundtrip: ") + bad);
  if (const char *bad = out_fmt_fault(out_fmt)) return fail(ctx, GLC_EINVAL, std::string("glc_roundtrip: ") + bad);
  glc_plan plan;
  RtGeom g;
  int rc = rt_check(ctx, "glc_roundtrip", n_samples, channels, pcm_out, pcm_elem(out_fmt), cap, n_out, &plan, &g);
  if (rc != GLC_OK) return rc;
  // At the host boundary a round is what the copies are cut into, and the first upload and the last download
  // are hidden by nothing: rounds of 4096 ROWS - the smallest launch the large transform kernel takes
  // (launch_mdct_forward), half a device round for stereo.
  g.round = std::max<uint64_t>(1, std::min<uint64_t>(g.round, 4096 / channels));
  DeviceGuard guard(ctx->device);
  rt_forget_streams(ctx);
  rc = out_fmt == GLC_PCM_S16 ? rt_roundtrip_host(ctx, pcm, fmt, bits, n_samples, g, plan, static_cast<int16_t *>(pcm_out))
                              : rt_roundtrip_host(ctx, pcm, fmt, bits, n_samples, g, plan, static_cast<float *>(pcm_out));
  if (rc != GLC_OK) {  // nothing may still be in flight out of or into the caller's memory
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->down_stream) (void)hipStreamSynchronize(ctx->down_stream);
  }
  return rc;
}

int glc_roundtrip_last_info(glc_ctx *ctx, glc_roundtrip_info *out) {
  if (!ctx || !out) return fail(ctx, GLC_EINVAL, "glc_roundtrip_last_info: null argument");
  if (ctx->rt_info_frames == 0 || !ctx->rt_stats.p)
    return fail(ctx, GLC_EINVAL, "glc_roundtrip_last_info: no round trip has completed on this context");
  DeviceGuard guard(ctx->device);
  uint64_t slots[glc::kRowStatSlots * glc::kRowStatStride];
  GLC_HIP(ctx, hipMemcpyAsync(slots, ctx->rt_stats.p, sizeof slots, hipMemcpyDeviceToHost, ctx->stream));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t s[2] = {0, 0};
  for (uint32_t i = 0; i < glc::kRowStatSlots; ++i) s[0] += slots[i * glc::kRowStatStride], s[1] += slots[i * glc::kRowStatStride + 1];
  rt_fill_info(out, ctx->rt_info_frames, ctx->rt_info_ch, s[0], s[1]);
  return GLC_OK;
}

// ------------------------------------------------------------------------------ round trip, many clips

int TableImage::begin(glc_ctx *ctx, size_t bytes) {
  int rc = rt_reserve(ctx, ctx->rtb_tab, bytes);
  if (rc != GLC_OK) return rc;
  GLC_HIP(ctx, ctx->rtb_ev.ensure());
  if (pending) GLC_HIP(ctx, hipEventSynchronize(ctx->rtb_ev));
  pending = false;
  GLC_HIP(ctx, ctx->rtb_stage.reserve(bytes));
  img = static_cast<uint8_t *>(ctx->rtb_stage.p), tab = static_cast<const uint8_t *>(ctx->rtb_tab.p);
  return GLC_OK;
}
int TableImage::send(glc_ctx *ctx, size_t bytes) {
  GLC_HIP(ctx, hipMemcpyAsync(ctx->rtb_tab.p, ctx->rtb_stage.p, bytes, hipMemcpyHostToDevice, ctx->stream));
  GLC_HIP(ctx, hipEventRecord(ctx->rtb_ev, ctx->stream));
  pending = true;
  return GLC_OK;
}

extern "C++" {
namespace {

// (RtbLayout, the view of a glc_clip_layout, and RtbPcm, the input of a batch call: glc_args.hpp)

int rtb_stage(glc_ctx *ctx, const RtbPcm &pcm, const glc::StageClip *clips, uint64_t n_clips, uint32_t ch, const RtbLayout &in, uint64_t V,
              float *vs, hipStream_t st) {
  if (pcm.fmt == GLC_PCM_F32)
    GLC_HIP(ctx, glc::launch_stage_clips(static_cast<const float *>(pcm.p), clips, static_cast<uint32_t>(n_clips), ch, in.planes(),
                                         in.l->channel_stride, static_cast<uint32_t>(V), vs, st));
  else
    GLC_HIP(ctx, glc::launch_stage_clips_int(pcm.p, pcm.fmt == GLC_PCM_S32, pcm.bits, clips, static_cast<uint32_t>(n_clips), ch, in.planes(),
                                             in.l->channel_stride, static_cast<uint32_t>(V), vs, st));
  return GLC_OK;
}

// A round of the batch round trip: clips [first, first + n) packed into one virtual stream, or (lng) ONE clip
// longer than a round, staged whole and sent through rounds with the carried overlap.
struct RtbRound : RoundSpan {
  size_t o_clips = 0, o_fmap = 0, o_desc = 0, o_span = 0;  // in the call's table image (o_span: the store encode's clip table)
  uint64_t n_desc = 0;
  uint64_t stat_off = 0;  // lng: the clip's kRowStatSlots counter pairs
};

// Kept hops of a clip: 512 interleaved samples of delay in front (hop 0 is cut), len * ch kept.
inline uint64_t rtb_hops_kept(uint64_t len, uint32_t ch) { return (glc::kHop / 2 + len * ch - 1) / (uint64_t(glc::kHop) * ch) + 1; }

// pack_rounds (glc_rounds.hpp) into the rounds a driver keeps: R is a RoundSpan and the driver's own offsets.
template <typename R, typename FramesOf>
std::vector<R> plan_rounds(uint64_t n, FramesOf frames_of, uint64_t budget, uint64_t front) {
  std::vector<R> rounds;
  for (const RoundSpan &s : pack_rounds(n, frames_of, budget, front)) static_cast<RoundSpan &>(rounds.emplace_back()) = s;
  return rounds;
}

template <typename Out>  // float, or int16_t: D2 narrows
int rtb_impl(glc_ctx *ctx, const RtbPcm &pcm, const RtbLayout &in, Out *d_out, const RtbLayout &out) {
  const uint64_t n = in.l->n_clips;
  const uint32_t ch = in.l->channels;
  const uint64_t per_hop = uint64_t(glc::kHop) * ch, rec = glc::record_bytes(ch);
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;
  std::vector<glc_plan> plans(n);
  for (uint64_t i = 0; i < n; ++i) plans[i] = glc::plan_encode(in.len(i) * ch, static_cast<uint16_t>(ch));

  auto rounds = plan_rounds<RtbRound>(n, [&](uint64_t i) { return plans[i].n_frames; }, encode_chunk_frames(ch), 0);
  // the call's tables, and what the workspaces have to hold
  TableOffsets offs;
  const uint64_t clip_stat = uint64_t(glc::kClipStatSlots) * glc::kRowStatStride;  // uint64_t per clip
  uint64_t stat_words = n * clip_stat;
  uint64_t max_vs = 0, max_recs = 0, max_rows = 0, max_blocks = 0, max_frames = 0, max_coef_rows = 0;
  for (RtbRound &r : rounds) {
    r.o_clips = offs.take(r.n * sizeof(glc::StageClip));
    for (uint64_t i = r.first; i < r.first + r.n; ++i) r.n_desc += rtb_hops_kept(in.len(i), ch);
    r.o_desc = offs.take(r.n_desc * sizeof(glc::HopDescStrided));
    max_vs = std::max(max_vs, r.V * per_hop);
    if (r.lng) {
      const uint64_t rf = std::min<uint64_t>(kDecodeChunkFrames, r.n_real);
      r.stat_off = stat_words;
      stat_words += kRtStatBytes / sizeof(uint64_t);
      max_recs = std::max(max_recs, rf), max_rows = std::max(max_rows, rf * ch), max_blocks = std::max(max_blocks, rf + 1);
      max_frames = std::max(max_frames, rf), max_coef_rows = std::max(max_coef_rows, rf * ch);
    } else {
      r.o_fmap = offs.take(r.n_real * sizeof(glc::FrameMap));
      max_recs = std::max(max_recs, r.V), max_rows = std::max(max_rows, r.n_real * ch), max_blocks = std::max(max_blocks, r.n_real);
      max_frames = std::max(max_frames, r.n_real), max_coef_rows = std::max(max_coef_rows, r.V * ch);
    }
  }
  rt_forget_streams(ctx);
  ctx->rtb_info.clear();
  int rc = rt_reserve(ctx, ctx->rtb_vs, max_vs * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_records, max_recs * rec);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->coef, max_coef_rows * glc::kHop * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_records_bytes(static_cast<uint32_t>(max_rows)));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->blocks, max_blocks * slot * sizeof(float));
  if (rc == GLC_OK) rc = reserve_d1_plan(ctx, max_frames, ch);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rtb_stats, stat_words * sizeof(uint64_t));
  TableImage &image = ctx->rtb_image;
  if (rc == GLC_OK) rc = image.begin(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  const bool out_planes = out.planes();
  for (const RtbRound &r : rounds) {
    auto *clips = image.host<glc::StageClip>(r.o_clips);
    auto *desc = image.host<glc::HopDescStrided>(r.o_desc);
    auto *fmap = image.host<glc::FrameMap>(r.o_fmap);
    uint64_t vslot = 0, real = 0;
    for (uint64_t k = 0; k < r.n; ++k) {
      const uint64_t i = r.first + k, nf = plans[i].n_frames;
      clips[k] = glc::StageClip{in.at(i), in.len(i), static_cast<uint32_t>(vslot), {0u, 0u, 0u}};
      const glc::Trim trim = glc::gapless_trim(nf, ch, plans[i].encoder_delay, in.len(i) * ch);
      desc = write_clip_descs(desc, r.lng, nf, ch, trim, real, out.at(i), out_planes, out.l->channel_stride);
      if (!r.lng)
        for (uint64_t f = 0; f < nf; ++f)
          fmap[real + f] = glc::FrameMap{static_cast<uint32_t>(vslot + f), static_cast<uint32_t>(i)};
      vslot += nf + 1;
      real += nf;
    }
    if (static_cast<uint64_t>(desc - image.host<glc::HopDescStrided>(r.o_desc)) != r.n_desc)
      return fail(ctx, GLC_EHIP, "glc_roundtrip_batch_device: hop count arithmetic is inconsistent");
  }
  hipStream_t st = ctx->stream;
  rc = image.send(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  uint64_t *d_stats = static_cast<uint64_t *>(ctx->rtb_stats.p);
  GLC_HIP(ctx, hipMemsetAsync(d_stats, 0, stat_words * sizeof(uint64_t), st));

  float *vs = static_cast<float *>(ctx->rtb_vs.p);
  float *blocks = static_cast<float *>(ctx->blocks.p);
  const uint8_t *recs = static_cast<const uint8_t *>(ctx->rt_records.p);
  for (const RtbRound &r : rounds) {
    const auto *desc = image.dev<glc::HopDescStrided>(r.o_desc);
    rc = rtb_stage(ctx, pcm, image.dev<glc::StageClip>(r.o_clips), r.n, ch, in, r.V, vs, st);
    if (rc != GLC_OK) return rc;
    if (r.lng) {
      const uint64_t i = r.first, n_samples = in.len(i) * ch;
      const RtGeom g = rt_geom(r.n_real, ch, plans[i], n_samples);
      for (uint64_t f0 = 0; f0 < g.n_frames; f0 += g.round) {
        const uint64_t nf = std::min(g.round, g.n_frames - f0), f1 = f0 + nf;
        // the round's descriptors: those of hops [f0, f1 (+ 1)) that keep anything - all but none, since only the
        // tail hop can lie wholly behind the kept samples
        const uint64_t nd = count_hop_descs(g.trim, per_hop, f0, f1 + (f1 == g.n_frames ? 1 : 0));
        const RtStridedSink<Out> sink{desc, static_cast<uint32_t>(nd), out_planes, d_out};
        rc = rt_roundtrip_round<Out>(ctx, g, vs, n_samples, f0, nf, nullptr, d_stats + r.stat_off, &sink);
        if (rc != GLC_OK) return rc;
        desc += nd;
      }
      continue;
    }
    const uint64_t T = r.V * glc::kHop;
    rc = encode_range_on(ctx, st, EncodeRange{{vs, 0, T, T * ch, static_cast<uint32_t>(ch)}, 0, r.V, ctx->rt_records.p, nullptr, &ctx->slot[0]});
    if (rc != GLC_OK) return rc;
    const uint32_t M = static_cast<uint32_t>(r.n_real * ch);
    glc::DecodeRows rows{};
    GLC_HIP(ctx, glc::launch_rows_from_records_batch(recs, M, ch, image.dev<glc::FrameMap>(r.o_fmap), ctx->rt_rows.p, d_stats, st, &rows));
    // (D1's 8-frame units may span two clips: that only widens a union)
    GLC_HIP(ctx, launch_d1_rows(ctx, rows, 0, M, ch, blocks, st));
    GLC_HIP(ctx, glc::launch_overlap_add_strided(blocks, desc, static_cast<uint32_t>(r.n_desc), ch, out_planes, d_out, st));
  }
  ctx->rtb_info.resize(n);
  for (uint64_t i = 0; i < n; ++i) ctx->rtb_info[i] = glc_ctx::RtbClipInfo{plans[i].n_frames, i * clip_stat, glc::kClipStatSlots};
  for (const RtbRound &r : rounds)
    if (r.lng) ctx->rtb_info[r.first] = glc_ctx::RtbClipInfo{r.n_real, r.stat_off, glc::kRowStatSlots};
  ctx->rtb_info_ch = ch;
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

// glc_roundtrip_batch_device and glc_roundtrip_batch_device_pcm: the checks, then rtb_impl.
static int rtb_call(glc_ctx *ctx, const char *who, const void *d_pcm, glc_pcm_format fmt, uint32_t bits, const glc_clip_layout *in,
                    void *d_out, glc_pcm_format out_fmt, const glc_clip_layout *out) {
  const std::string w(who);
  if (!ctx) return GLC_EINVAL;
  if (!in || !out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (const char *bad = fmt_fault(fmt, bits)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  if (const char *bad = out_fmt_fault(out_fmt)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  if (in->n_clips != out->n_clips || in->channels != out->channels)
    return fail(ctx, GLC_EINVAL, w + ": the two layouts differ in the number of clips or channels");
  if (in->n_clips == 0) return GLC_OK;
  if (!d_pcm || !d_out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (in->channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  const RtbPcm pcm{d_pcm, fmt, bits};
  if (!aligned(d_pcm, pcm.elem()) || !aligned(d_out, pcm_elem(out_fmt)))
    return fail(ctx, GLC_EINVAL, w + ": a pointer is not aligned to its sample size");
  const RtbLayout li{in}, lo{out};
  const uint64_t n = in->n_clips;
  for (uint64_t i = 0; i < n; ++i) {
    if (li.len(i) != lo.len(i)) return fail(ctx, GLC_EINVAL, clip_name(w, i) + ": the two layouts differ in its length");
    for (const RtbLayout *l : {&li, &lo})
      if (const char *bad = clip_fault(*l, i)) return fail(ctx, GLC_EINVAL, clip_name(w, i) + ": " + bad);
  }
  if (overlaps(span_of(d_pcm, li, pcm.elem()), span_of(d_out, lo, pcm_elem(out_fmt))) && !in_place(d_pcm, li, fmt, d_out, lo, out_fmt))
    return fail(ctx, GLC_EINVAL, w + ": input and output overlap (in place needs the same pointer, the same layout and the same format)");
  return on_device(ctx, w, [&] {
    return out_fmt == GLC_PCM_S16 ? rtb_impl(ctx, pcm, li, static_cast<int16_t *>(d_out), lo)
                                  : rtb_impl(ctx, pcm, li, static_cast<float *>(d_out), lo);
  });
}

int glc_roundtrip_batch_device(glc_ctx *ctx, const float *d_pcm, const glc_clip_layout *in, float *d_out,
                               const glc_clip_layout *out) {
  return rtb_call(ctx, "glc_roundtrip_batch_device", d_pcm, GLC_PCM_F32, 32, in, d_out, GLC_PCM_F32, out);
}

int glc_roundtrip_batch_device_pcm(glc_ctx *ctx, const void *d_pcm, glc_pcm_format fmt, uint32_t bits, const glc_clip_layout *in,
                                   void *d_out, glc_pcm_format out_fmt, const glc_clip_layout *out) {
  return rtb_call(ctx, "glc_roundtrip_batch_device_pcm", d_pcm, fmt, bits, in, d_out, out_fmt, out);
}

int glc_roundtrip_batch_last_info(glc_ctx *ctx, glc_roundtrip_info *infos, uint64_t n_clips) {
  if (!ctx || !infos) return fail(ctx, GLC_EINVAL, "glc_roundtrip_batch_last_info: null argument");
  if (ctx->rtb_info.empty() || !ctx->rtb_stats.p)
    return fail(ctx, GLC_EINVAL, "glc_roundtrip_batch_last_info: no batch round trip has completed on this context");
  if (n_clips != ctx->rtb_info.size())
    return fail(ctx, GLC_EINVAL, "glc_roundtrip_batch_last_info: the last batch had another number of clips");
  uint64_t words = 0;
  for (const glc_ctx::RtbClipInfo &c : ctx->rtb_info) words = std::max(words, c.stat_off + uint64_t(c.stat_slots) * glc::kRowStatStride);
  return on_device(ctx, "glc_roundtrip_batch_last_info", [&]() -> int {
    std::vector<uint64_t> h(words);
    GLC_HIP(ctx, hipMemcpyAsync(h.data(), ctx->rtb_stats.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n_clips; ++i) {
      const glc_ctx::RtbClipInfo &c = ctx->rtb_info[i];
      uint64_t s0 = 0, s1 = 0;
      for (uint32_t k = 0; k < c.stat_slots; ++k) s0 += h[c.stat_off + k * glc::kRowStatStride], s1 += h[c.stat_off + k * glc::kRowStatStride + 1];
      rt_fill_info(&infos[i], c.n_frames, ctx->rtb_info_ch, s0, s1);
    }
    return GLC_OK;
  });
}

// ------------------------------------------------------------------------------ decode of compact blobs in HBM

extern "C++" {
namespace {

// What both calls check of one blob before anything is queued: the fault, or null (as the rules of glc_args.hpp).
const char *cd_blob_fault(const void *d_blob, uint64_t blob_bytes, uint32_t ch, uint64_t n_frames) {
  if (!d_blob) return "null argument";
  if (!aligned(d_blob, 64)) return "the blob is not 64-byte aligned";
  if (blob_bytes < glc::compact_layout(ch, n_frames).o_pairs) return "blob_bytes is smaller than the fixed sections of a blob of that many frames";
  return nullptr;
}

// A blob of `nf` frames through R2 (one pass over all its rows, tables in rt_rows) and the rounds of the family.
// `win` (a crop, g.trim what it keeps): the windowed R2 over the window's rows, and the rounds of its frames only.
template <typename T>
int cd_decode_one(glc_ctx *ctx, const RtGeom &g, const void *d_blob, uint64_t blob_bytes, glc::CompactStatus *d_status,
                  T *d_out, const glc::HopDescStrided *desc, bool planar, T *sink_out, const glc_crop_plan *win = nullptr) {
  const uint64_t fb = win ? win->first_frame : 0, fe = win ? fb + win->n_frames : g.n_frames;
  const uint32_t M = static_cast<uint32_t>((fe - fb) * g.ch), M_blob = static_cast<uint32_t>(g.n_frames * g.ch);
  const size_t slot = static_cast<size_t>(g.ch) * glc::kFrame;
  int rc = rt_reserve(ctx, ctx->blocks, (g.round + 1) * slot * sizeof(float));
  // 32 B per row of the STREAM, or of the window
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_compact_bytes(M));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_edge, 2 * g.per_hop * sizeof(float));
  if (rc == GLC_OK) rc = reserve_d1_plan(ctx, g.round, g.ch);
  if (rc != GLC_OK) return rc;
  const uint32_t front = static_cast<uint32_t>(fb * g.ch);
  const glc::CompactBlob one{reinterpret_cast<uintptr_t>(d_blob), blob_bytes, 0u, M_blob, {front, M}};  // whole: {0, M_blob}
  glc::DecodeRows rows{};
  GLC_HIP(ctx, glc::launch_rows_from_compact(nullptr, one, 1, M, g.ch, glc::R2Mode{!win, front, nullptr}, d_blob, ctx->rt_rows.p, d_status,
                                             ctx->stream, &rows));
  for (uint64_t f0 = fb; f0 < fe; f0 += g.round) {
    const uint64_t nf = std::min(g.round, fe - f0), f1 = f0 + nf;
    // the round's descriptors: those of hops [f0, f1 (+ 1)) that keep anything (rtb_impl)
    const uint64_t nd = desc ? count_hop_descs(g.trim, g.per_hop, f0, f1 + (f1 == g.n_frames ? 1 : 0)) : 0;
    const RtStridedSink<T> sink{desc, static_cast<uint32_t>(nd), planar, sink_out};
    if (desc) desc += nd;
    rc = rt_decode_round_rows<T>(ctx, g, rows, static_cast<uint32_t>((f0 - fb) * g.ch), f0, nf, d_out, desc ? &sink : nullptr);
    if (rc != GLC_OK) return rc;
  }
  return GLC_OK;
}

// A round of glc_decode_batch_device_compact: blobs [first, first + n) with together n_real frames, or (lng) ONE
// blob of more frames than a round.
struct CdRound : RoundSpan {
  size_t o_dir = 0, o_desc = 0;  // in the call's table image
  uint64_t n_desc = 0;
};

// `crops` / `wins` (both or neither; glc_decode_crops_device_compact): entry i is the window wins[i] = plan_crop of
// crops[i] of its blob - a round counts, tabulates and transforms the windows' frames only.
template <typename T>
int cdb_impl(glc_ctx *ctx, const char *who, const void *const *d_blobs, const uint64_t *blob_bytes, T *d_out, const RtbLayout &out,
             const std::vector<glc_plan> &plans, const glc_crop *crops = nullptr, const glc_crop_plan *wins = nullptr) {
  const uint64_t n = out.l->n_clips;
  auto frames_of = [&](uint64_t i) { return wins ? wins[i].n_frames : plans[i].n_frames; };
  const uint32_t ch = out.l->channels;
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;
  // whole clips of together at most kDecodeChunkFrames frames (+ a tail hop each)
  auto rounds = plan_rounds<CdRound>(n, frames_of, kDecodeChunkFrames + 1, 0);
  TableOffsets offs;
  uint64_t max_rows = 0, max_blocks = 0, max_frames = 0;
  for (CdRound &r : rounds) {
    if (!r.lng) r.o_dir = offs.take(r.n * sizeof(glc::CompactBlob));
    for (uint64_t i = r.first; i < r.first + r.n; ++i) r.n_desc += wins ? wins[i].n_hops : rtb_hops_kept(out.len(i), ch);
    r.o_desc = offs.take(r.n_desc * sizeof(glc::HopDescStrided));
    const uint64_t rf = r.lng ? std::min<uint64_t>(kDecodeChunkFrames, r.n_real) : r.n_real;
    max_rows = std::max(max_rows, r.n_real * ch);  // R2 takes a long clip's (or window's) rows in one pass
    max_blocks = std::max(max_blocks, rf + (r.lng ? 1 : 0));
    max_frames = std::max(max_frames, rf);
  }
  rt_forget_streams(ctx);
  ctx->cd_status_n = 0;
  int rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_compact_bytes(static_cast<uint32_t>(max_rows)));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->blocks, max_blocks * slot * sizeof(float));
  if (rc == GLC_OK) rc = reserve_d1_plan(ctx, max_frames, ch);
  TableImage &image = ctx->rtb_image;
  if (rc == GLC_OK) rc = image.begin(ctx, offs.size());
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->cd_status, n * sizeof(glc::CompactStatus));
  if (rc != GLC_OK) return rc;
  const bool out_planes = out.planes();
  // what entry i keeps of its un-trimmed stream: the clip, or the crop behind the delay
  auto trim_of = [&](uint64_t i) {
    const glc::Trim whole = glc::gapless_trim(plans[i].n_frames, ch, plans[i].encoder_delay, crops ? plans[i].per_channel * ch : out.len(i) * ch);
    return crops ? glc::Trim{whole.start + crops[i].start * ch, crops[i].length * ch} : whole;
  };
  for (const CdRound &r : rounds) {
    auto *dir = image.host<glc::CompactBlob>(r.o_dir);
    auto *desc = image.host<glc::HopDescStrided>(r.o_desc);
    uint64_t real = 0;
    for (uint64_t k = 0; k < r.n; ++k) {
      const uint64_t i = r.first + k, nf = plans[i].n_frames;
      const uint32_t w0 = wins ? static_cast<uint32_t>(wins[i].first_frame * ch) : 0u, w1 = static_cast<uint32_t>(frames_of(i) * ch);
      if (!r.lng)
        dir[k] = glc::CompactBlob{reinterpret_cast<uintptr_t>(d_blobs[i]), blob_bytes[i], static_cast<uint32_t>(real * ch),
                                  static_cast<uint32_t>(nf * ch), {w0, w1}};
      desc = write_clip_descs(desc, r.lng, nf, ch, trim_of(i), real, out.at(i), out_planes, out.l->channel_stride, wins ? &wins[i] : nullptr);
      real += frames_of(i);
    }
    if (static_cast<uint64_t>(desc - image.host<glc::HopDescStrided>(r.o_desc)) != r.n_desc)
      return fail(ctx, GLC_EHIP, std::string(who) + ": hop count arithmetic is inconsistent");
  }
  hipStream_t st = ctx->stream;
  rc = image.send(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  auto *d_status = static_cast<glc::CompactStatus *>(ctx->cd_status.p);
  float *blocks = static_cast<float *>(ctx->blocks.p);
  for (const CdRound &r : rounds) {
    const auto *desc = image.dev<glc::HopDescStrided>(r.o_desc);
    if (r.lng) {
      const uint64_t i = r.first;
      RtGeom g = rt_geom(plans[i].n_frames, ch, plans[i], out.len(i) * ch);
      g.trim = trim_of(i);
      rc = cd_decode_one<T>(ctx, g, d_blobs[i], blob_bytes[i], d_status + i, nullptr, desc, out_planes, d_out, wins ? &wins[i] : nullptr);
      if (rc != GLC_OK) return rc;
      continue;
    }
    // pairs and raw planes are addressed from ONE base: the round's lowest blob (offsets are exact, every blob
    // is 64-byte aligned)
    uintptr_t base = reinterpret_cast<uintptr_t>(d_blobs[r.first]);
    for (uint64_t i = r.first; i < r.first + r.n; ++i) base = std::min(base, reinterpret_cast<uintptr_t>(d_blobs[i]));
    const uint32_t M = static_cast<uint32_t>(r.n_real * ch);
    glc::DecodeRows rows{};
    const auto *d_dir = image.dev<glc::CompactBlob>(r.o_dir);
    uint64_t front = 0;  // the most rows any window of the round has in front
    for (uint64_t i = r.first; wins && i < r.first + r.n; ++i) front = std::max(front, wins[i].first_frame * ch);
    GLC_HIP(ctx, glc::launch_rows_from_compact(d_dir, glc::CompactBlob{}, static_cast<uint32_t>(r.n), M, ch,
                                               glc::R2Mode{!wins, static_cast<uint32_t>(front), nullptr},
                                               reinterpret_cast<const void *>(base), ctx->rt_rows.p, d_status + r.first, st, &rows));
    // (D1's 8-frame units may span two clips: that only widens a union)
    GLC_HIP(ctx, launch_d1_rows(ctx, rows, 0, M, ch, blocks, st));
    GLC_HIP(ctx, glc::launch_overlap_add_strided(blocks, desc, static_cast<uint32_t>(r.n_desc), ch, out_planes, d_out, st));
  }
  ctx->cd_status_n = n;
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

int glc_decode_device_compact(glc_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint64_t n_samples, uint16_t channels,
                              float *d_out, uint64_t cap, uint64_t *n_out) {
  const std::string w("glc_decode_device_compact");
  if (!ctx) return GLC_EINVAL;
  if (n_out) *n_out = 0;
  glc_plan plan;
  RtGeom g;
  int rc = rt_check(ctx, w.c_str(), n_samples, channels, d_out, sizeof(float), cap, n_out, &plan, &g);
  if (rc != GLC_OK) return rc;
  if (const char *bad = cd_blob_fault(d_blob, blob_bytes, channels, plan.n_frames)) rc = fail(ctx, GLC_EINVAL, w + ": " + bad);
  if (rc == GLC_OK && overlaps(span_of(d_blob, blob_bytes), span_of(d_out, g.trim.n * sizeof(float))))
    rc = fail(ctx, GLC_EINVAL, w + ": the output overlaps the blob");
  if (rc != GLC_OK) {
    if (n_out) *n_out = 0;
    return rc;
  }
  DeviceGuard guard(ctx->device);
  rt_forget_streams(ctx);
  ctx->cd_status_n = 0;
  rc = rt_reserve(ctx, ctx->cd_status, sizeof(glc::CompactStatus));
  if (rc == GLC_OK)
    rc = cd_decode_one<float>(ctx, g, d_blob, blob_bytes, static_cast<glc::CompactStatus *>(ctx->cd_status.p), d_out, nullptr, false, nullptr);
  if (rc == GLC_OK) ctx->cd_status_n = 1;
  return rc;
}

// glc_decode_batch_device_compact and (crops) glc_decode_crops_device_compact, and their _i16 twins (T = int16_t): the
// checks, then cdb_impl.
extern "C++" {
template <typename T>
static int cd_batch_call(glc_ctx *ctx, const char *who, const void *const *d_blobs, const uint64_t *blob_bytes, const uint64_t *n_samples,
                         const glc_crop *crops, bool windows, T *d_out, const glc_clip_layout *out) {
  const std::string w(who);
  if (!ctx) return GLC_EINVAL;
  if (!out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (out->n_clips == 0) return GLC_OK;
  if (!d_blobs || !blob_bytes || !n_samples || !d_out || (windows && !crops)) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (out->channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  if (!aligned(d_out, sizeof(T))) return fail(ctx, GLC_EINVAL, w + ": output pointer not aligned to its sample size");
  const RtbLayout lo{out};
  const uint64_t n = out->n_clips, ch = out->channels;
  try {  // no C++ exception may cross the C ABI; the device is set only once nothing is left to refuse
    std::vector<glc_plan> plans(n);
    std::vector<glc_crop_plan> wins(windows ? n : 0);
    for (uint64_t i = 0; i < n; ++i) {
      auto refuse = [&](const char *what) { return fail(ctx, GLC_EINVAL, clip_name(w, i) + ": " + what); };
      if (const char *bad = frames_fault(n_samples[i], out->channels, &plans[i])) return refuse(bad);
      if (windows) {
        if (n_samples[i] % ch) return refuse("n_samples is no multiple of the channel count");
        if (!glc::plan_crop(n_samples[i], out->channels, crops[i], &wins[i])) return refuse("an empty crop, or one that ends behind the clip");
        if (lo.len(i) != crops[i].length) return refuse("the layout's length is not the crop's");
      } else if (lo.len(i) * ch != n_samples[i]) {
        return refuse("the layout's length is not the decoded length");
      }
      if (const char *bad = stride_fault(lo, i)) return refuse(bad);
      if (const char *bad = cd_blob_fault(d_blobs[i], blob_bytes[i], out->channels, plans[i].n_frames)) return refuse(bad);
    }
    const ByteSpan all = span_of(d_out, lo, sizeof(T));
    for (uint64_t i = 0; i < n; ++i)
      if (overlaps(span_of(d_blobs[i], blob_bytes[i]), all)) return fail(ctx, GLC_EINVAL, clip_name(w, i) + ": the output extent overlaps the blob");
    DeviceGuard guard(ctx->device);
    return cdb_impl(ctx, who, d_blobs, blob_bytes, d_out, lo, plans, windows ? crops : nullptr, windows ? wins.data() : nullptr);
  } catch (const std::bad_alloc &) {
    return fail(ctx, GLC_ENOMEM, w + ": host allocation failed");
  }
}
}  // extern "C++"

int glc_decode_batch_device_compact(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes, const uint64_t *n_samples,
                                    float *d_out, const glc_clip_layout *out) {
  return cd_batch_call(ctx, "glc_decode_batch_device_compact", d_blobs, blob_bytes, n_samples, nullptr, false, d_out, out);
}

int glc_decode_crops_device_compact(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes, const uint64_t *n_samples,
                                    const glc_crop *crops, float *d_out, const glc_clip_layout *out) {
  return cd_batch_call(ctx, "glc_decode_crops_device_compact", d_blobs, blob_bytes, n_samples, crops, true, d_out, out);
}

int glc_decode_batch_device_compact_i16(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes, const uint64_t *n_samples,
                                        int16_t *d_out, const glc_clip_layout *out) {
  return cd_batch_call(ctx, "glc_decode_batch_device_compact_i16", d_blobs, blob_bytes, n_samples, nullptr, false, d_out, out);
}

int glc_decode_crops_device_compact_i16(glc_ctx *ctx, const void *const *d_blobs, const uint64_t *blob_bytes, const uint64_t *n_samples,
                                        const glc_crop *crops, int16_t *d_out, const glc_clip_layout *out) {
  return cd_batch_call(ctx, "glc_decode_crops_device_compact_i16", d_blobs, blob_bytes, n_samples, crops, true, d_out, out);
}

int glc_decode_compact_last_status(glc_ctx *ctx, glc_compact_status *status, uint64_t n_clips) {
  if (!ctx || !status) return fail(ctx, GLC_EINVAL, "glc_decode_compact_last_status: null argument");
  if (ctx->cd_status_n == 0 || !ctx->cd_status.p)
    return fail(ctx, GLC_EINVAL, "glc_decode_compact_last_status: no compact decode has completed on this context");
  if (n_clips != ctx->cd_status_n) return fail(ctx, GLC_EINVAL, "glc_decode_compact_last_status: the last call had another number of clips");
  return on_device(ctx, "glc_decode_compact_last_status", [&]() -> int {
    std::vector<glc::CompactStatus> h(n_clips);
    GLC_HIP(ctx, hipMemcpyAsync(h.data(), ctx->cd_status.p, n_clips * sizeof(glc::CompactStatus), hipMemcpyDeviceToHost, ctx->stream));
    GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n_clips; ++i)
      status[i] = glc_compact_status{h[i].flags, 0u, h[i].n_bad_rows, h[i].n_bad_rows ? h[i].first_bad_row : 0ull};
    return GLC_OK;
  });
}

// ------------------------------------------------------------------------------ crops drawn from the store by device-side index

extern "C++" {
namespace {

// What glc_decode_crops_device_store, its ragged sibling and their planner hooks share: the checks of everything the
// host can see, and the geometry of the call - the slots of a crop, the crops of a round, and where the planner's three
// arrays lie in rtb_tab.
struct SdGeom {
  glc::CropSlots slots{};
  uint64_t descs = 0;  // descriptors of a crop: its hops, or what a ragged crop needs (glc_common.h store_ragged_slots)
  uint64_t per_round = 0, max_front = 0;
  size_t o_dir = 0, o_desc = 0, o_verdict = 0, tab = 0;
};

// What the ragged draw has beyond the fixed one: per crop the length it wants and the length it got, device arrays
// that may both be absent.  A null SdRagged is the fixed draw.
struct SdRagged {
  const int64_t *d_want;
  int64_t *d_valid;
};

int sd_check(glc_ctx *ctx, const std::string &w, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
             const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips, const int64_t *d_starts,
             uint64_t length, const void *d_out, size_t out_elem, const glc_clip_layout *out, const SdRagged *rg, SdGeom *g) {
  if (!d_arena || !d_entries || !d_lengths || !d_clips || !d_starts || !d_out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (out->channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  const uint64_t n = out->n_clips, ch = out->channels;
  if (!aligned(d_arena, 64)) return fail(ctx, GLC_EINVAL, w + ": the arena is not 64-byte aligned");
  if (!all_aligned(8, d_entries, d_lengths, d_clips, d_starts))
    return fail(ctx, GLC_EINVAL, w + ": entries, lengths, clips and starts must be 8-byte aligned");
  if (rg && !all_aligned(8, rg->d_want, rg->d_valid)) return fail(ctx, GLC_EINVAL, w + ": want and valid must be 8-byte aligned");
  if (!aligned(d_out, out_elem)) return fail(ctx, GLC_EINVAL, w + ": output pointer not aligned to its sample size");
  if (n_entries == 0) return fail(ctx, GLC_EINVAL, w + ": n_entries == 0");
  if (length == 0) return fail(ctx, GLC_EINVAL, w + ": length == 0");
  // a ragged crop may be longer than every clip; its own samples must still not wrap (max_length bounds the fixed crop's)
  if (!rg && max_length < length) return fail(ctx, GLC_EINVAL, w + ": max_length is smaller than the crop");
  if (rg && length > (UINT64_MAX >> 12) / ch) return fail(ctx, GLC_EINVAL, w + ": length: stream too long");
  if (max_length > (UINT64_MAX >> 12) / ch) return fail(ctx, GLC_EINVAL, w + ": max_length: stream too long");
  glc_plan longest;
  if (const char *bad = frames_fault(max_length * ch, out->channels, &longest)) return fail(ctx, GLC_EINVAL, w + ": max_length: " + bad);
  const RtbLayout lo{out};
  if (out->lengths) {
    for (uint64_t i = 0; i < n; ++i)
      if (out->lengths[i] != length) return fail(ctx, GLC_EINVAL, clip_name(w, i) + ": the layout's length is not the crop's");
  } else if (out->length != length) {
    return fail(ctx, GLC_EINVAL, w + ": the layout's length is not the crop's");
  }
  // every clip is `length` long: what the stride rule finds of clip 0 it finds of all
  if (const char *bad = stride_fault(lo, 0)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  g->slots = glc::store_crop_slots(length, out->channels);
  g->descs = rg ? glc::store_ragged_slots(length, out->channels).max_descs : g->slots.max_hops;
  if (g->slots.max_frames + 1 > glc::kStoreRoundBudget)
    return fail(ctx, GLC_EINVAL, w + ": a crop of this length does not fit a round (glc_decode_crops_device_compact takes such windows)");
  g->per_round = glc::kStoreRoundBudget / (g->slots.max_frames + 1);
  g->max_front = longest.n_frames * ch;
  const ByteSpan all = span_of(d_out, lo, out_elem);
  if (overlaps(span_of(d_arena, arena_bytes), all)) return fail(ctx, GLC_EINVAL, w + ": the output extent overlaps the arena");
  const ByteSpan index[] = {span_of(d_entries, n_entries * sizeof(glc_store_entry)), span_of(d_lengths, n_entries * 8),
                            span_of(d_clips, n * 8), span_of(d_starts, n * 8), span_of(rg ? rg->d_want : nullptr, n * 8)};
  for (const ByteSpan &in : index)
    if (in.lo && overlaps(in, all)) return fail(ctx, GLC_EINVAL, w + ": the output extent overlaps an index array");
  if (rg && rg->d_valid) {  // the one array beside the output that the call writes
    const ByteSpan valid = span_of(rg->d_valid, n * 8);
    if (overlaps(valid, all)) return fail(ctx, GLC_EINVAL, w + ": the output extent overlaps valid");
    if (overlaps(valid, span_of(d_arena, arena_bytes))) return fail(ctx, GLC_EINVAL, w + ": valid overlaps the arena");
    for (const ByteSpan &in : index)
      if (in.lo && overlaps(in, valid)) return fail(ctx, GLC_EINVAL, w + ": valid overlaps an index array");
  }
  TableOffsets offs;
  g->o_dir = offs.take(n * sizeof(glc::CompactBlob));
  g->o_desc = offs.take(n * g->descs * sizeof(glc::HopDescStrided));
  g->o_verdict = offs.take(n * sizeof(uint32_t));
  g->tab = offs.size();
  return GLC_OK;
}

// The planner's launch: the call's only word about the selection.  rtb_tab is written by the DEVICE here - the
// pinned image of the other batch calls is not touched and their upload event not waited for (an upload still on
// its way is in front of this kernel on the stream).
int sd_plan(glc_ctx *ctx, const SdGeom &g, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
            const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips, const int64_t *d_starts,
            uint64_t length, const glc_clip_layout *out, const SdRagged *rg) {
  uint8_t *d_tab = static_cast<uint8_t *>(ctx->rtb_tab.p);
  const RtbLayout lo{out};
  glc::StoreDraw a{};
  a.arena = reinterpret_cast<uintptr_t>(d_arena), a.arena_bytes = arena_bytes;
  a.entries = d_entries, a.lengths = d_lengths, a.n_entries = n_entries, a.max_length = max_length;
  a.clips = d_clips, a.starts = d_starts, a.length = length, a.n_crops = out->n_clips;
  a.ch = out->channels, a.max_hops = static_cast<uint32_t>(g.descs), a.max_frames = static_cast<uint32_t>(g.slots.max_frames);
  a.per_round = static_cast<uint32_t>(g.per_round);
  a.clip_stride = out->clip_stride, a.channel_stride = out->channel_stride, a.planes = lo.planes() ? 1u : 0u;
  a.dir = reinterpret_cast<glc::CompactBlob *>(d_tab + g.o_dir);
  a.desc = reinterpret_cast<glc::HopDescStrided *>(d_tab + g.o_desc);
  a.verdict = reinterpret_cast<uint32_t *>(d_tab + g.o_verdict);
  if (rg) a.ragged = 1u, a.want = rg->d_want, a.valid = rg->d_valid;
  GLC_HIP(ctx, glc::launch_store_plan_crops(a, ctx->stream));
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

int glc_store_crop_slots(uint64_t length, uint16_t channels, uint64_t *max_hops, uint64_t *max_frames) {
  if (!max_hops || !max_frames || channels == 0 || length == 0 || length > (UINT64_MAX >> 12) / channels) {
    glc::set_global_error("glc_store_crop_slots: a null pointer, channels == 0, length == 0 or a length whose samples wrap");
    return GLC_EINVAL;
  }
  const glc::CropSlots s = glc::store_crop_slots(length, channels);
  *max_hops = s.max_hops, *max_frames = s.max_frames;
  return GLC_OK;
}

int glc_store_ragged_slots(uint64_t length, uint16_t channels, uint64_t *max_descs, uint64_t *max_frames) {
  if (!max_descs || !max_frames || channels == 0 || length == 0 || length > (UINT64_MAX >> 12) / channels) {
    glc::set_global_error("glc_store_ragged_slots: a null pointer, channels == 0, length == 0 or a length whose samples wrap");
    return GLC_EINVAL;
  }
  const glc::RaggedSlots s = glc::store_ragged_slots(length, channels);
  *max_descs = s.max_descs, *max_frames = s.max_frames;
  return GLC_OK;
}

// glc_decode_crops_device_store, its _i16 twin (T = int16_t) and the ragged pair (rg given): the same plan, the same
// launches - but for the descriptors of a crop, of which a ragged one may have one more - D2 narrowing.
extern "C++" {
template <typename T>
static int sd_call(glc_ctx *ctx, const char *who, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                   const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips, const int64_t *d_starts,
                   uint64_t length, T *d_out, const glc_clip_layout *out, const SdRagged *rg = nullptr) {
  const std::string w(who);
  if (!ctx) return GLC_EINVAL;
  if (!out) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (out->n_clips == 0) return GLC_OK;
  SdGeom g;
  int rc = sd_check(ctx, w, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips, d_starts, length, d_out, sizeof(T),
                    out, rg, &g);
  if (rc != GLC_OK) return rc;
  const uint64_t n = out->n_clips;
  const uint32_t ch = out->channels;
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;
  const uint64_t widest = std::min(n, g.per_round) * g.slots.max_frames;  // frames (block slots) of the fullest round
  DeviceGuard guard(ctx->device);
  rt_forget_streams(ctx);
  ctx->cd_status_n = 0;
  rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_compact_bytes(static_cast<uint32_t>(widest * ch)));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->blocks, widest * slot * sizeof(float));
  if (rc == GLC_OK) rc = reserve_d1_plan(ctx, widest, ch);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rtb_tab, g.tab);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->cd_status, n * sizeof(glc::CompactStatus));
  if (rc == GLC_OK)
    rc = sd_plan(ctx, g, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips, d_starts, length, out, rg);
  if (rc != GLC_OK) return rc;
  const uint8_t *d_tab = static_cast<const uint8_t *>(ctx->rtb_tab.p);
  const auto *d_dir = reinterpret_cast<const glc::CompactBlob *>(d_tab + g.o_dir);
  const auto *d_desc = reinterpret_cast<const glc::HopDescStrided *>(d_tab + g.o_desc);
  const auto *d_verdict = reinterpret_cast<const uint32_t *>(d_tab + g.o_verdict);
  auto *d_status = static_cast<glc::CompactStatus *>(ctx->cd_status.p);
  float *blocks = static_cast<float *>(ctx->blocks.p);
  const bool out_planes = RtbLayout{out}.planes();
  hipStream_t st = ctx->stream;
  // one chain per round, each the same launches whatever the selection holds: the rounds differ only in their first crop
  for (uint64_t first = 0; first < n; first += g.per_round) {
    const uint64_t nr = std::min(g.per_round, n - first);
    const uint32_t M = static_cast<uint32_t>(nr * g.slots.max_frames * ch);
    glc::DecodeRows rows{};
    // pairs and raw planes are addressed from the arena: every usable blob lies inside it, 64-byte aligned
    GLC_HIP(ctx, glc::launch_rows_from_compact(d_dir + first, glc::CompactBlob{}, static_cast<uint32_t>(nr), M, ch,
                                               glc::R2Mode{false, static_cast<uint32_t>(g.max_front), d_verdict + first}, d_arena,
                                               ctx->rt_rows.p, d_status + first, st, &rows));
    GLC_HIP(ctx, launch_d1_rows(ctx, rows, 0, M, ch, blocks, st));
    GLC_HIP(ctx, glc::launch_overlap_add_strided(blocks, d_desc + first * g.descs, static_cast<uint32_t>(nr * g.descs), ch, out_planes,
                                                 d_out, st));
  }
  ctx->cd_status_n = n;
  return GLC_OK;
}

// The two planner hooks (include/glc_debug.h): the checks and the planner's launch as the calls make them, then what it
// wrote copied back - `valid` (ragged only) from a table behind the planner's own in rtb_tab.
static int sd_plan_hook(glc_ctx *ctx, const char *who, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                        const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                        const int64_t *d_starts, const int64_t *d_want, bool ragged, uint64_t length, const float *d_out,
                        const glc_clip_layout *out, void *dir, void *desc, uint32_t *verdict, int64_t *valid) {
  const std::string w(who);
  if (!ctx) return GLC_EINVAL;
  if (!out || !dir || !desc || !verdict || (ragged && !valid)) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (out->n_clips == 0) return GLC_OK;
  SdGeom g;
  SdRagged rg{d_want, nullptr};
  int rc = sd_check(ctx, w, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips, d_starts, length, d_out, sizeof(float),
                    out, ragged ? &rg : nullptr, &g);
  if (rc != GLC_OK) return rc;
  const uint64_t n = out->n_clips;
  DeviceGuard guard(ctx->device);
  rt_forget_streams(ctx);
  ctx->cd_status_n = 0;
  rc = rt_reserve(ctx, ctx->rtb_tab, g.tab + (ragged ? n * 8 : 0));
  if (rc != GLC_OK) return rc;
  uint8_t *d_tab = static_cast<uint8_t *>(ctx->rtb_tab.p);
  rg.d_valid = reinterpret_cast<int64_t *>(d_tab + g.tab);
  rc = sd_plan(ctx, g, d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips, d_starts, length, out,
               ragged ? &rg : nullptr);
  if (rc != GLC_OK) return rc;
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  GLC_HIP(ctx, hipMemcpy(dir, d_tab + g.o_dir, n * sizeof(glc::CompactBlob), hipMemcpyDeviceToHost));
  GLC_HIP(ctx, hipMemcpy(desc, d_tab + g.o_desc, n * g.descs * sizeof(glc::HopDescStrided), hipMemcpyDeviceToHost));
  GLC_HIP(ctx, hipMemcpy(verdict, d_tab + g.o_verdict, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (ragged) {
    GLC_HIP(ctx, hipMemcpy(valid, rg.d_valid, n * 8, hipMemcpyDeviceToHost));
  }
  return GLC_OK;
}
}  // extern "C++"

int glc_decode_crops_device_store(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                  const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                  const int64_t *d_starts, uint64_t length, float *d_out, const glc_clip_layout *out) {
  return sd_call(ctx, "glc_decode_crops_device_store", d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips, d_starts,
                 length, d_out, out);
}

int glc_decode_crops_device_store_i16(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                      const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                      const int64_t *d_starts, uint64_t length, int16_t *d_out, const glc_clip_layout *out) {
  return sd_call(ctx, "glc_decode_crops_device_store_i16", d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                 d_starts, length, d_out, out);
}

int glc_decode_ragged_crops_device_store(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                         const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                         const int64_t *d_starts, const int64_t *d_want, uint64_t length, float *d_out,
                                         const glc_clip_layout *out, int64_t *d_valid) {
  const SdRagged rg{d_want, d_valid};
  return sd_call(ctx, "glc_decode_ragged_crops_device_store", d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                 d_starts, length, d_out, out, &rg);
}

int glc_decode_ragged_crops_device_store_i16(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                             const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                             const int64_t *d_starts, const int64_t *d_want, uint64_t length, int16_t *d_out,
                                             const glc_clip_layout *out, int64_t *d_valid) {
  const SdRagged rg{d_want, d_valid};
  return sd_call(ctx, "glc_decode_ragged_crops_device_store_i16", d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length,
                 d_clips, d_starts, length, d_out, out, &rg);
}

int glc_debug_store_plan_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                const int64_t *d_starts, uint64_t length, const float *d_out, const glc_clip_layout *out, void *dir,
                                void *desc, uint32_t *verdict) {
  return sd_plan_hook(ctx, "glc_debug_store_plan_device", d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                      d_starts, nullptr, false, length, d_out, out, dir, desc, verdict, nullptr);
}

int glc_debug_store_plan_ragged_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                       const int64_t *d_lengths, uint64_t n_entries, uint64_t max_length, const int64_t *d_clips,
                                       const int64_t *d_starts, const int64_t *d_want, uint64_t length, const float *d_out,
                                       const glc_clip_layout *out, void *dir, void *desc, uint32_t *verdict, int64_t *valid) {
  return sd_plan_hook(ctx, "glc_debug_store_plan_ragged_device", d_arena, arena_bytes, d_entries, d_lengths, n_entries, max_length, d_clips,
                      d_starts, d_want, true, length, d_out, out, dir, desc, verdict, valid);
}

// ------------------------------------------------------------------------------ eviction from the store

namespace {
// Packed bytes of an in-place round ("the round of an eviction"): two staging buffers of this size.
constexpr uint64_t kStoreCompactRound = 64ull << 20;
}  // namespace

int glc_store_compact_device(glc_ctx *ctx, void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                             const int64_t *d_lengths, uint64_t n_entries, const uint8_t *d_keep, void *d_dst, uint64_t dst_bytes,
                             glc_store_entry *d_entries_out, int64_t *d_lengths_out, int64_t *d_new_index, uint64_t *d_n_out,
                             uint64_t *d_cursor) {
  const std::string w("glc_store_compact_device");
  if (!ctx) return GLC_EINVAL;
  if (!d_arena || !d_entries || !d_keep || !d_dst || !d_entries_out || !d_new_index || !d_n_out || !d_cursor)
    return fail(ctx, GLC_EINVAL, w + ": null argument");
  if ((d_lengths == nullptr) != (d_lengths_out == nullptr))
    return fail(ctx, GLC_EINVAL, w + ": d_lengths and d_lengths_out are given together or not at all");
  if (!all_aligned(64, d_arena, d_dst)) return fail(ctx, GLC_EINVAL, w + ": the arenas must be 64-byte aligned");
  if (!all_aligned(8, d_entries, d_lengths, d_entries_out, d_lengths_out, d_new_index, d_n_out, d_cursor))
    return fail(ctx, GLC_EINVAL, w + ": entries, lengths, new_index, n_out and cursor must be 8-byte aligned");
  if (n_entries == 0) return fail(ctx, GLC_EINVAL, w + ": n_entries == 0");
  if (n_entries > (1ull << 40)) return fail(ctx, GLC_EINVAL, w + ": too many entries");
  const bool in_place = d_dst == d_arena;
  if (in_place && dst_bytes != arena_bytes) return fail(ctx, GLC_EINVAL, w + ": in place, dst_bytes must be arena_bytes");
  // (an arena or an index array that is updated in place is ONE span: its twin takes no part)
  const char *one, *other;
  if (first_overlap({span_of(d_arena, arena_bytes, "the arena"),
                     in_place ? ByteSpan{} : span_of(d_dst, dst_bytes, "the destination arena"),
                     span_of(d_entries, n_entries * sizeof(glc_store_entry), "d_entries"),
                     span_of(d_lengths, n_entries * 8, "d_lengths"),
                     span_of(d_keep, n_entries, "d_keep"),
                     d_entries_out != d_entries ? span_of(d_entries_out, n_entries * sizeof(glc_store_entry), "d_entries_out") : ByteSpan{},
                     d_lengths_out != d_lengths ? span_of(d_lengths_out, n_entries * 8, "d_lengths_out") : ByteSpan{},
                     span_of(d_new_index, n_entries * 8, "d_new_index"),
                     span_of(d_n_out, 8, "d_n_out"),
                     span_of(d_cursor, 8, "d_cursor")},
                    &one, &other))
    return fail(ctx, GLC_EINVAL, w + ": " + one + " overlaps " + other);
  const uint64_t round = ctx->sc_round ? ctx->sc_round : kStoreCompactRound;
  DeviceGuard guard(ctx->device);
  // not a decode and not an encode: the resident stream, an open session, the kept plan and the last-info records stay
  int rc = rt_reserve(ctx, ctx->sc_ws, glc::store_evict_ws_bytes(n_entries));
  if (rc == GLC_OK && in_place && arena_bytes) rc = rt_reserve(ctx, ctx->sc_stage, 2 * std::min(round, (arena_bytes + 63) / 64 * 64));
  if (rc != GLC_OK) return rc;
  glc::StoreEvict a{};
  a.arena_bytes = arena_bytes, a.dst_bytes = dst_bytes;
  a.entries = d_entries, a.lengths = d_lengths, a.keep = d_keep, a.n_entries = n_entries;
  a.entries_out = d_entries_out, a.lengths_out = d_lengths_out, a.new_index = d_new_index;
  a.n_out = d_n_out, a.cursor = d_cursor, a.ws = static_cast<uint64_t *>(ctx->sc_ws.p);
  GLC_HIP(ctx, glc::launch_store_evict_scan(a, ctx->stream));
  if (!in_place) {
    GLC_HIP(ctx, glc::launch_store_evict_gather(a.ws, d_arena, arena_bytes, d_dst, ctx->stream));
    return GLC_OK;
  }
  if (arena_bytes == 0) return GLC_OK;
  // the host does not know the packed total: every round the arena could need is queued, and one at or behind the total
  // returns at once.  An arena of less than a round is one round of its own size (rounded up to 64).
  const uint64_t rs = std::min(round, (arena_bytes + 63) / 64 * 64), rounds = (arena_bytes + rs - 1) / rs;
  for (uint64_t r = 0; r <= rounds; ++r) GLC_HIP(ctx, glc::launch_store_evict_round(a.ws, d_arena, ctx->sc_stage.p, rs, r, ctx->stream));
  return GLC_OK;
}

int glc_debug_set_store_compact_round(glc_ctx *ctx, uint64_t bytes) {
  if (!ctx || (bytes & 63ull) || bytes > (1ull << 40))
    return fail(ctx, GLC_EINVAL, "glc_debug_set_store_compact_round: the round must be a multiple of 64 (0: the default)");
  ctx->sc_round = bytes;
  return GLC_OK;
}

// ------------------------------------------------------------------------------ joining a clip's segments in the store

int glc_store_join_segments_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                                   const glc_stream_seg *segs, uint64_t n_segs, const uint64_t *lengths, uint16_t channels, void *d_dst,
                                   uint64_t dst_bytes, uint64_t *d_cursor, glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                                   uint32_t *d_seg_status) {
  const std::string w("glc_store_join_segments_device");
  if (!ctx) return GLC_EINVAL;
  if (n_segs == 0) return GLC_OK;  // nothing to join: the cursor stays
  if (!d_arena || !d_entries || !segs || !d_dst || !d_cursor || !d_entries_out || !d_seg_status)
    return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  if ((lengths == nullptr) != (d_lengths_out == nullptr))
    return fail(ctx, GLC_EINVAL, w + ": lengths and d_lengths_out are given together or not at all");
  if (!all_aligned(64, d_arena, d_dst)) return fail(ctx, GLC_EINVAL, w + ": the arenas must be 64-byte aligned");
  if (!all_aligned(8, d_entries, d_cursor, d_entries_out, d_lengths_out))
    return fail(ctx, GLC_EINVAL, w + ": entries, lengths_out and cursor must be 8-byte aligned");
  if (!aligned(d_seg_status, 4)) return fail(ctx, GLC_EINVAL, w + ": d_seg_status must be 4-byte aligned");
  if (n_segs > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": too many segments");
  return on_device(ctx, w, [&]() -> int {
    std::vector<JoinClipSpan> clips;
    uint64_t at = 0;
    bool of_clip = false;
    if (const char *bad = join_segs_fault(segs, n_segs, lengths, channels, &clips, &at, &of_clip))
      return fail(ctx, GLC_EINVAL, w + (of_clip ? ": clip " : ": segment ") + std::to_string(at) + ": " + bad);
    const uint64_t n_clips = clips.size();
    const char *one, *other;
    if (first_overlap({span_of(d_arena, arena_bytes, "the arena"), span_of(d_dst, dst_bytes, "the destination arena"),
                       span_of(d_entries, n_segs * sizeof(glc_store_entry), "d_entries"),
                       span_of(d_entries_out, n_clips * sizeof(glc_store_entry), "d_entries_out"),
                       span_of(d_lengths_out, n_clips * 8, "d_lengths_out"), span_of(d_seg_status, n_segs * 4, "d_seg_status"),
                       span_of(d_cursor, 8, "d_cursor")},
                      &one, &other))
      return fail(ctx, GLC_EINVAL, w + ": " + one + " overlaps " + other);
    // a host bound on the joined bytes, for the shape of the move: what the clips' rows can hold, and the destination
    uint64_t bound = 0;
    for (const JoinClipSpan &c : clips) bound = std::min(dst_bytes, bound + glc::compact_layout(channels, c.n_frames).bound);
    // not a decode and not an encode: the resident stream, an open session, the kept plan and the last-info records stay.
    // The image (the two tables) and, behind it, the workspace the kernels write share the batch calls' table buffer.
    TableOffsets offs;
    const size_t o_segs = offs.take(n_segs * sizeof(glc::StoreJoinSeg));
    const size_t o_clips = offs.take(n_clips * sizeof(glc::StoreJoinClip));
    const size_t img_bytes = offs.size();
    const size_t o_ws = offs.take(glc::store_join_ws_bytes(n_segs, n_clips));
    TableImage &image = ctx->rtb_image;
    if (const int rc = image.begin(ctx, offs.size())) return rc;
    auto *seg_tab = image.host<glc::StoreJoinSeg>(o_segs);
    auto *clip_tab = image.host<glc::StoreJoinClip>(o_clips);
    for (uint64_t c = 0; c < n_clips; ++c) {
      clip_tab[c] = glc::StoreJoinClip{clips[c].seg_first, clips[c].n_segs, clips[c].n_frames, lengths ? static_cast<int64_t>(lengths[c]) : 0};
      for (uint64_t j = clips[c].seg_first; j < clips[c].seg_first + clips[c].n_segs; ++j)
        seg_tab[j] = glc::StoreJoinSeg{static_cast<uint32_t>(c), 0u, segs[j].first_frame, segs[j].n_frames};
    }
    if (const int rc = image.send(ctx, img_bytes)) return rc;
    glc::StoreJoin a{};
    a.arena = static_cast<const unsigned char *>(d_arena), a.arena_bytes = arena_bytes, a.entries = d_entries;
    a.segs = image.dev<glc::StoreJoinSeg>(o_segs), a.n_segs = n_segs;
    a.clips = image.dev<glc::StoreJoinClip>(o_clips), a.n_clips = n_clips;
    a.ch = channels, a.has_lengths = lengths ? 1u : 0u;
    a.dst = static_cast<unsigned char *>(d_dst), a.dst_bytes = dst_bytes, a.cursor = d_cursor;
    a.entries_out = d_entries_out, a.lengths_out = d_lengths_out, a.seg_status = d_seg_status;
    a.ws = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(ctx->rtb_tab.p) + o_ws);
    GLC_HIP(ctx, glc::launch_store_join_plan(a, ctx->stream));
    GLC_HIP(ctx, glc::launch_store_join_move(a, bound, ctx->stream));
    return GLC_OK;
  });
}

// ------------------------------------------------------------------------------ cutting stored clips into frame ranges

int glc_store_cut_device(glc_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, uint64_t n_entries,
                         const glc_store_cut *cuts, uint64_t n_cuts, const uint64_t *lengths, uint16_t channels, void *d_dst,
                         uint64_t dst_bytes, uint64_t *d_cursor, glc_store_entry *d_entries_out, int64_t *d_lengths_out,
                         uint32_t *d_cut_status) {
  const std::string w("glc_store_cut_device");
  if (!ctx) return GLC_EINVAL;
  if (n_cuts == 0) return GLC_OK;  // nothing to cut: the cursor stays
  if (!d_arena || !d_entries || !cuts || !d_dst || !d_cursor || !d_entries_out || !d_lengths_out || !d_cut_status)
    return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  if (!all_aligned(64, d_arena, d_dst)) return fail(ctx, GLC_EINVAL, w + ": the arenas must be 64-byte aligned");
  if (!all_aligned(8, d_entries, d_cursor, d_entries_out, d_lengths_out))
    return fail(ctx, GLC_EINVAL, w + ": entries, lengths_out and cursor must be 8-byte aligned");
  if (!aligned(d_cut_status, 4)) return fail(ctx, GLC_EINVAL, w + ": d_cut_status must be 4-byte aligned");
  if (n_cuts > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": too many cuts");
  if (n_entries > (1ull << 40)) return fail(ctx, GLC_EINVAL, w + ": too many entries");
  return on_device(ctx, w, [&]() -> int {
    uint64_t at = 0;
    if (const char *bad = cuts_fault(cuts, n_cuts, lengths, channels, &at))
      return fail(ctx, GLC_EINVAL, w + ": cut " + std::to_string(at) + ": " + bad);
    const char *one, *other;
    if (first_overlap({span_of(d_arena, arena_bytes, "the arena"), span_of(d_dst, dst_bytes, "the destination arena"),
                       span_of(d_entries, n_entries * sizeof(glc_store_entry), "d_entries"),
                       span_of(d_entries_out, n_cuts * sizeof(glc_store_entry), "d_entries_out"),
                       span_of(d_lengths_out, n_cuts * 8, "d_lengths_out"), span_of(d_cut_status, n_cuts * 4, "d_cut_status"),
                       span_of(d_cursor, 8, "d_cursor")},
                      &one, &other))
      return fail(ctx, GLC_EINVAL, w + ": " + one + " overlaps " + other);
    // a host bound on the pieces' bytes, for the shape of the move: what the pieces' rows can hold, and the destination
    uint64_t bound = 0;
    for (uint64_t i = 0; i < n_cuts; ++i) bound = std::min(dst_bytes, bound + glc::compact_layout(channels, cuts[i].n_frames).bound);
    // not a decode and not an encode: the resident stream, an open session, the kept plan and the last-info records stay.
    // The image (the cut table) and, behind it, the workspace the kernels write share the batch calls' table buffer.
    TableOffsets offs;
    const size_t o_cuts = offs.take(n_cuts * sizeof(glc::StoreCutItem));
    const size_t img_bytes = offs.size();
    const size_t o_ws = offs.take(glc::store_cut_ws_bytes(n_cuts));
    TableImage &image = ctx->rtb_image;
    if (const int rc = image.begin(ctx, offs.size())) return rc;
    auto *cut_tab = image.host<glc::StoreCutItem>(o_cuts);
    for (uint64_t i = 0; i < n_cuts; ++i)
      cut_tab[i] = glc::StoreCutItem{cuts[i].clip, cuts[i].first_frame, cuts[i].n_frames,
                                     static_cast<int64_t>(lengths ? lengths[i] : glc::kHop * cuts[i].n_frames)};
    if (const int rc = image.send(ctx, img_bytes)) return rc;
    glc::StoreCut a{};
    a.arena = static_cast<const unsigned char *>(d_arena), a.arena_bytes = arena_bytes, a.entries = d_entries, a.n_entries = n_entries;
    a.cuts = image.dev<glc::StoreCutItem>(o_cuts), a.n_cuts = n_cuts;
    a.ch = channels;
    a.dst = static_cast<unsigned char *>(d_dst), a.dst_bytes = dst_bytes, a.cursor = d_cursor;
    a.entries_out = d_entries_out, a.lengths_out = d_lengths_out, a.cut_status = d_cut_status;
    a.ws = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(ctx->rtb_tab.p) + o_ws);
    GLC_HIP(ctx, glc::launch_store_cut_plan(a, ctx->stream));
    GLC_HIP(ctx, glc::launch_store_cut_move(a, bound, ctx->stream));
    return GLC_OK;
  });
}

// ------------------------------------------------------------------------------ encode of a batch into per-clip compact blobs

extern "C++" {
namespace {

// The frame map and the clip table of a round whose clip k has frames[k] frames (A1-A3, glc_kernels.h): every real
// frame names its record and its clip; with `junk` a record nobody names lies behind every clip.
void store_round_tables(const uint64_t *frames, uint64_t n, bool junk, glc::FrameMap *fmap, glc::ClipSpan *span) {
  uint64_t vslot = 0, real = 0;
  for (uint64_t k = 0; k < n; ++k) {
    span[k] = glc::ClipSpan{static_cast<uint32_t>(real), static_cast<uint32_t>(frames[k])};
    for (uint64_t f = 0; f < frames[k]; ++f)
      fmap[real + f] = glc::FrameMap{static_cast<uint32_t>(vslot + f), static_cast<uint32_t>(k)};
    vslot += frames[k] + (junk ? 1 : 0);
    real += frames[k];
  }
}

// A1-A3 of one round, as the driver and the hook queue them: the round's tables are on the device already.
int store_round_launch(glc_ctx *ctx, const void *d_records, uint64_t n_real, uint64_t n_clips, uint32_t ch, const TableImage &image,
                       size_t o_fmap, size_t o_span, void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
                       glc_store_entry *d_entries, hipStream_t st) {
  GLC_HIP(ctx, glc::launch_compact_store(static_cast<const uint8_t *>(d_records), static_cast<uint32_t>(n_real * ch), ch,
                                         image.dev<glc::FrameMap>(o_fmap), image.dev<glc::ClipSpan>(o_span), static_cast<uint32_t>(n_clips),
                                         ctx->pack_meta.p, static_cast<uint8_t *>(d_arena), arena_bytes, d_cursor, d_entries, st));
  return GLC_OK;
}

int ebc_impl(glc_ctx *ctx, const RtbPcm &pcm, const RtbLayout &in, void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
             glc_store_entry *d_entries) {
  const uint64_t n = in.l->n_clips;
  const uint32_t ch = in.l->channels;
  const uint64_t per_hop = uint64_t(glc::kHop) * ch, rec = glc::record_bytes(ch);
  std::vector<glc_plan> plans(n);
  for (uint64_t i = 0; i < n; ++i) plans[i] = glc::plan_encode(in.len(i) * ch, static_cast<uint16_t>(ch));
  auto rounds = plan_rounds<RtbRound>(n, [&](uint64_t i) { return plans[i].n_frames; }, encode_chunk_frames(ch), 0);
  TableOffsets offs;
  uint64_t max_vs = 0, max_recs = 0, max_coef_rows = 0, max_scratch = 0;
  for (RtbRound &r : rounds) {
    r.o_clips = offs.take(r.n * sizeof(glc::StageClip));
    r.o_fmap = offs.take(r.n_real * sizeof(glc::FrameMap));
    r.o_span = offs.take(r.n * sizeof(glc::ClipSpan));
    max_vs = std::max(max_vs, r.V * per_hop);
    // a long clip's records are all held at once (the pack scans the whole clip); its transform goes in chunks
    max_recs = std::max(max_recs, r.lng ? r.n_real : r.V);
    max_coef_rows = std::max(max_coef_rows, (r.lng ? std::min(encode_chunk_frames(ch), r.n_real) : r.V) * ch);
    max_scratch = std::max(max_scratch, glc::compact_store_scratch_bytes(r.n_real * ch, r.n));
  }
  rt_forget_streams(ctx);
  int rc = rt_reserve(ctx, ctx->rtb_vs, max_vs * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_records, max_recs * rec);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->coef, max_coef_rows * glc::kHop * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->pack_meta, max_scratch);
  TableImage &image = ctx->rtb_image;
  if (rc == GLC_OK) rc = image.begin(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  std::vector<uint64_t> frames;
  for (const RtbRound &r : rounds) {
    auto *clips = image.host<glc::StageClip>(r.o_clips);
    frames.resize(r.n);
    uint64_t vslot = 0;
    for (uint64_t k = 0; k < r.n; ++k) {
      const uint64_t i = r.first + k;
      frames[k] = plans[i].n_frames;
      clips[k] = glc::StageClip{in.at(i), in.len(i), static_cast<uint32_t>(vslot), {0u, 0u, 0u}};
      vslot += frames[k] + 1;
    }
    // a long clip is encoded as a stream of its own: its records are its frames, no junk one among them
    store_round_tables(frames.data(), r.n, !r.lng, image.host<glc::FrameMap>(r.o_fmap), image.host<glc::ClipSpan>(r.o_span));
  }
  hipStream_t st = ctx->stream;
  rc = image.send(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  float *vs = static_cast<float *>(ctx->rtb_vs.p);
  for (const RtbRound &r : rounds) {
    rc = rtb_stage(ctx, pcm, image.dev<glc::StageClip>(r.o_clips), r.n, ch, in, r.V, vs, st);
    if (rc != GLC_OK) return rc;
    if (r.lng) {
      const uint64_t len = in.len(r.first);
      rc = encode_range_on(ctx, st, EncodeRange{{vs, 0, len, len * ch, static_cast<uint32_t>(ch)}, 0, r.n_real, ctx->rt_records.p, nullptr, &ctx->slot[0]});
    } else {
      const uint64_t T = r.V * glc::kHop;
      rc = encode_range_on(ctx, st, EncodeRange{{vs, 0, T, T * ch, static_cast<uint32_t>(ch)}, 0, r.V, ctx->rt_records.p, nullptr, &ctx->slot[0]});
    }
    if (rc == GLC_OK)
      rc = store_round_launch(ctx, ctx->rt_records.p, r.n_real, r.n, ch, image, r.o_fmap, r.o_span, d_arena, arena_bytes, d_cursor,
                              d_entries + r.first, st);
    if (rc != GLC_OK) return rc;
  }
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

// glc_encode_batch_device_compact and glc_encode_batch_device_compact_int: the checks, then ebc_impl.
static int ebc_call(glc_ctx *ctx, const char *who, const void *d_pcm, glc_pcm_format fmt, uint32_t bits, const glc_clip_layout *in,
                    void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor, glc_store_entry *d_entries) {
  const std::string w(who);
  if (!ctx) return GLC_EINVAL;
  if (!in) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (const char *bad = fmt_fault(fmt, bits)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  if (in->n_clips == 0) return GLC_OK;
  if (!d_pcm || !d_arena || !d_cursor || !d_entries) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (in->channels == 0) return fail(ctx, GLC_EINVAL, w + ": channels == 0");
  const RtbPcm pcm{d_pcm, fmt, bits};
  if (const char *bad = store_fill_misaligned(pcm, d_arena, d_cursor, d_entries)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  const RtbLayout li{in};
  const uint64_t n = in->n_clips;
  for (uint64_t i = 0; i < n; ++i)
    if (const char *bad = clip_fault(li, i)) return fail(ctx, GLC_EINVAL, clip_name(w, i) + ": " + bad);
  if (const char *bad = store_fill_overlap(pcm, li, d_arena, arena_bytes, d_entries)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  return on_device(ctx, w, [&] { return ebc_impl(ctx, pcm, li, d_arena, arena_bytes, d_cursor, d_entries); });
}

int glc_encode_batch_device_compact(glc_ctx *ctx, const float *d_pcm, const glc_clip_layout *in, void *d_arena, uint64_t arena_bytes,
                                    uint64_t *d_cursor, glc_store_entry *d_entries) {
  return ebc_call(ctx, "glc_encode_batch_device_compact", d_pcm, GLC_PCM_F32, 32, in, d_arena, arena_bytes, d_cursor, d_entries);
}

int glc_encode_batch_device_compact_int(glc_ctx *ctx, const void *d_pcm, glc_pcm_format fmt, uint32_t bits, const glc_clip_layout *in,
                                        void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor, glc_store_entry *d_entries) {
  return ebc_call(ctx, "glc_encode_batch_device_compact_int", d_pcm, fmt, bits, in, d_arena, arena_bytes, d_cursor, d_entries);
}

int glc_debug_compact_store_device(glc_ctx *ctx, const void *d_records, const uint64_t *clip_frames, uint64_t n_clips,
                                   uint16_t channels, void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
                                   glc_store_entry *d_entries) {
  const std::string w("glc_debug_compact_store_device");
  if (!ctx || !d_records || !clip_frames || !d_arena || !d_cursor || !d_entries) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (channels == 0 || n_clips == 0 || n_clips > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": no channels, no clips or too many");
  uint64_t n_real = 0;
  for (uint64_t i = 0; i < n_clips; ++i) {
    if (clip_frames[i] == 0 || clip_frames[i] > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": a clip of no frames, or of too many");
    n_real += clip_frames[i];
  }
  if ((n_real + n_clips) * channels > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": frame range too long");
  if (!aligned(d_arena, 64) || !all_aligned(8, d_records, d_cursor, d_entries)) return fail(ctx, GLC_EINVAL, w + ": a pointer is not aligned");
  return on_device(ctx, w, [&]() -> int {
    const size_t o_fmap = 0, o_span = align_up(n_real * sizeof(glc::FrameMap), 256), tab = o_span + n_clips * sizeof(glc::ClipSpan);
    TableImage &image = ctx->rtb_image;
    int rc = rt_reserve(ctx, ctx->pack_meta, glc::compact_store_scratch_bytes(n_real * channels, n_clips));
    if (rc == GLC_OK) rc = image.begin(ctx, tab);
    if (rc != GLC_OK) return rc;
    store_round_tables(clip_frames, n_clips, true, image.host<glc::FrameMap>(o_fmap), image.host<glc::ClipSpan>(o_span));
    rc = image.send(ctx, tab);
    if (rc != GLC_OK) return rc;
    return store_round_launch(ctx, d_records, n_real, n_clips, channels, image, o_fmap, o_span, d_arena, arena_bytes, d_cursor, d_entries,
                              ctx->stream);
  });
}

// ------------------------------------------------------------------------------ streaming encode

extern "C++" {

// A host segment of a lane: the compact blob of frames [first_frame, first_frame + n_frames).
struct StreamBlob {
  uint64_t first_frame, n_frames;
  std::vector<uint64_t> words;  // the blob, 8-byte aligned
  uint64_t bytes;
};

struct StreamLane {
  uint64_t received = 0, done = 0;  // samples per channel so far, frames completed
  uint32_t parity = 0;              // which of the lane's two held-back buffers is current
  bool finished = false;            // host pushes: ended and not taken yet
  uint64_t total = 0;               // ... its samples per channel
  std::vector<StreamBlob> blobs;    // host pushes: the segments so far
};

// What a streaming session of either direction is: `n` lanes of `ch` channels on a context, what each lane carries
// from push to push in device memory, and the pinned buffers of its host pushes.
struct StreamSession {
  glc_ctx *ctx = nullptr;
  uint32_t ch = 0;
  uint64_t n = 0;
  int mode = 0;       // 0: no push yet, 1: host pushes, 2: device pushes
  DevBuf lane_buf;    // what the lanes carry, a fixed number of bytes each (stream_open)
  HostBuf up, down;   // pinned, host pushes: what goes up, what comes down
};

// glc_stream_enc_open / glc_stream_dec_open (`who`): a session S of n_streams lanes that carry `per_lane` bytes each.
template <typename S>
int stream_open(glc_ctx *ctx, const std::string &who, uint16_t channels, uint64_t n_streams, uint64_t per_lane, S **out) {
  if (!ctx) return GLC_EINVAL;
  if (!out) return fail(ctx, GLC_EINVAL, who + ": null argument");
  *out = nullptr;
  if (channels == 0 || n_streams == 0) return fail(ctx, GLC_EINVAL, who + ": no channels or no streams");
  if (n_streams > (1ull << 46) / per_lane) return fail(ctx, GLC_EINVAL, who + ": too many streams");
  return on_device(ctx, who, [&]() -> int {
    std::unique_ptr<S> s(new S);
    s->ctx = ctx, s->ch = channels, s->n = n_streams;
    s->size_lanes(n_streams);
    const hipError_t e = s->lane_buf.reserve(n_streams * per_lane);
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": hipMalloc").c_str());
    *out = s.release();
    return GLC_OK;
  });
}

template <typename S>
void stream_close(S *s) {
  if (!s) return;
  DeviceGuard guard(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);  // queued pushes may still read and write the session's buffers
  delete s;
}

// A session takes host pushes (1) or device pushes (2), whichever came first: the gate of a push of kind `pushing`.
static int stream_mode_gate(const StreamSession *s, const std::string &w, int pushing) {
  if (s->mode == 0 || s->mode == pushing) return GLC_OK;
  return fail(s->ctx, GLC_EINVAL, w + (pushing == 1 ? ": this session takes device pushes" : ": this session takes host pushes"));
}

}  // extern "C++"

struct glc_stream_enc : StreamSession {
  std::vector<StreamLane> lanes;  // lane_buf holds what they keep back: [lane][2][2048 * ch] floats
  void size_lanes(uint64_t k) { lanes.resize(k); }
  DevBuf d_pcm, arena, d_meta;  // host pushes; d_meta: the cursor (8 bytes, padded to 64) and the entries
  uint64_t held_at(uint64_t lane, uint32_t parity) const { return (lane * 2 + parity) * uint64_t(glc::kFrame) * ch; }
};

extern "C++" {
namespace {

// What a device push does with lane `lane`: its plan, and the chunk.
struct StreamLanePush {
  uint64_t lane, n_new;
  bool finish;
  glc_stream_push_plan plan;
};

// The core of both pushes: everything is validated.  Queues the rounds; fills segs / n_segs; updates the lanes.
int stream_push_core(glc_stream_enc *s, const RtbPcm &pcm, const RtbLayout &in, const std::vector<StreamLanePush> &act,
                     void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor, glc_store_entry *d_entries, glc_stream_seg *segs,
                     uint64_t *n_segs) {
  glc_ctx *ctx = s->ctx;
  const uint32_t ch = s->ch;
  const uint64_t per_hop = uint64_t(glc::kHop) * ch, rec = glc::record_bytes(ch), budget = encode_chunk_frames(ch);
  // the segments, in lane order, and the lanes whose held-back samples change (a finished lane holds nothing back)
  std::vector<const StreamLanePush *> seg, keep;
  for (const StreamLanePush &a : act) {
    if (a.plan.n_frames) seg.push_back(&a);
    if (!a.finish && a.n_new) keep.push_back(&a);
  }
  // rounds: a virtual slot in front (its second half is the first segment's lookback), frames + 1 slots per segment
  struct Round : RoundSpan {
    size_t o_spans = 0, o_fmap = 0, o_span = 0;
    uint64_t n_spans = 0;
  };
  auto rounds = plan_rounds<Round>(seg.size(), [&](uint64_t k) { return seg[k]->plan.n_frames; }, budget, 1);
  // no segment is a round of its own: glc_stream_enc_max_push bounds a chunk so that the frames it completes, their
  // junk slot and the slot in front fit a round
  for (const Round &R : rounds)
    if (R.lng) return fail(ctx, GLC_EHIP, "glc_stream_enc_push: internal: a segment does not fit a round");
  if (rounds.empty() && !keep.empty()) rounds.emplace_back();  // the stager alone: no slot at all
  *n_segs = seg.size();
  for (uint64_t k = 0; k < seg.size(); ++k) segs[k] = glc_stream_seg{seg[k]->lane, seg[k]->plan.first_frame, seg[k]->plan.n_frames};
  rt_forget_streams(ctx);
  // what the lanes are after the push: a finished lane is fresh, the others have flipped to their other buffer
  auto commit = [&] {
    for (const StreamLanePush &a : act) {
      StreamLane &L = s->lanes[a.lane];
      if (a.finish) {
        L.received = 0, L.done = 0;
      } else {
        L.received += a.n_new, L.done += a.plan.n_frames;
        if (a.n_new) L.parity ^= 1u;
      }
    }
  };
  if (rounds.empty()) {  // only finishes that complete no frame: nothing to queue
    commit();
    return GLC_OK;
  }
  TableOffsets offs;
  uint64_t max_V = 0, max_scratch = 0;
  for (size_t r = 0; r < rounds.size(); ++r) {
    Round &R = rounds[r];
    R.n_spans = R.n + (r == 0 ? keep.size() : 0);
    R.o_spans = offs.take(R.n_spans * sizeof(glc::StreamSpan));
    R.o_fmap = offs.take(R.n_real * sizeof(glc::FrameMap));
    R.o_span = offs.take(R.n * sizeof(glc::ClipSpan));
    max_V = std::max(max_V, R.V);
    if (R.n) max_scratch = std::max(max_scratch, glc::compact_store_scratch_bytes(R.n_real * ch, R.n));
  }
  int rc = rt_reserve(ctx, ctx->rtb_vs, max_V * per_hop * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->rt_records, max_V * rec);
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->coef, max_V * ch * glc::kHop * sizeof(float));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->pack_meta, max_scratch);
  TableImage &image = ctx->rtb_image;
  if (rc == GLC_OK) rc = image.begin(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  auto span_of = [&](const StreamLanePush &a) {
    const StreamLane &L = s->lanes[a.lane];
    glc::StreamSpan sp{};
    sp.src = in.at(a.lane), sp.received = L.received, sp.n_new = a.n_new;
    sp.held_x = glc::stream_held_from(L.done);
    sp.held_old = s->held_at(a.lane, L.parity), sp.held_new = s->held_at(a.lane, L.parity ^ 1u);
    return sp;
  };
  std::vector<uint64_t> frames;
  for (size_t r = 0; r < rounds.size(); ++r) {
    const Round &R = rounds[r];
    auto *spans = image.host<glc::StreamSpan>(R.o_spans);
    frames.resize(R.n);
    uint64_t slot = 1;
    for (uint64_t k = 0; k < R.n; ++k) {
      const StreamLanePush &a = *seg[R.first + k];
      glc::StreamSpan sp = span_of(a);
      sp.x0 = static_cast<int64_t>(a.plan.first_frame * glc::kHop) - static_cast<int64_t>(glc::kHop / 2);
      sp.unit = static_cast<uint32_t>(2 * slot - 1);
      spans[k] = sp;
      frames[k] = a.plan.n_frames;
      slot += a.plan.n_frames + 1;
    }
    if (r == 0)
      for (size_t q = 0; q < keep.size(); ++q) {
        const StreamLanePush &a = *keep[q];
        glc::StreamSpan sp = span_of(a);
        sp.x0 = static_cast<int64_t>(glc::stream_held_from(a.plan.first_frame + a.plan.n_frames));
        sp.unit = static_cast<uint32_t>(2 * R.V + 4 * q);
        spans[R.n + q] = sp;
      }
    if (R.n) store_round_tables(frames.data(), R.n, true, image.host<glc::FrameMap>(R.o_fmap), image.host<glc::ClipSpan>(R.o_span));
  }
  hipStream_t st = ctx->stream;
  rc = image.send(ctx, offs.size());
  if (rc != GLC_OK) return rc;
  float *vs = static_cast<float *>(ctx->rtb_vs.p);
  for (size_t r = 0; r < rounds.size(); ++r) {
    const Round &R = rounds[r];
    GLC_HIP(ctx, glc::launch_stage_segments(pcm.p, pcm.fmt, pcm.bits, image.dev<glc::StreamSpan>(R.o_spans), static_cast<uint32_t>(R.n_spans), static_cast<uint32_t>(2 * R.V),
                                            static_cast<uint32_t>(r == 0 ? 4 * keep.size() : 0), ch, in.planes(), in.l->channel_stride,
                                            static_cast<float *>(s->lane_buf.p), vs, st));
    if (!R.n) continue;
    // the virtual stream's frames [1, V - 1): frame 0 is the slot in front, frame V - 1 the last segment's junk one;
    // record j is virtual frame j + 1, which is how store_round_tables numbers them
    const uint64_t T = R.V * glc::kHop;
    rc = encode_range_on(ctx, st, EncodeRange{{vs, 0, T, T * ch, static_cast<uint32_t>(ch)}, 1, R.V - 1, ctx->rt_records.p, nullptr, &ctx->slot[0]});
    if (rc == GLC_OK)
      rc = store_round_launch(ctx, ctx->rt_records.p, R.n_real, R.n, ch, image, R.o_fmap, R.o_span, d_arena, arena_bytes, d_cursor,
                              d_entries + R.first, st);
    if (rc != GLC_OK) return rc;
  }
  commit();
  return GLC_OK;
}

// What both pushes check of the lanes and build for the core.  `lens`: samples per channel per lane.
int stream_plan_lanes(glc_stream_enc *s, const std::string &w, const uint64_t *lens, uint64_t len_all, const uint8_t *finish,
                      std::vector<StreamLanePush> *act) {
  const uint64_t max_push = glc_stream_enc_max_push(static_cast<uint16_t>(s->ch));
  for (uint64_t i = 0; i < s->n; ++i) {
    const uint64_t n_new = lens ? lens[i] : len_all;
    const bool fin = finish && finish[i];
    if (n_new > max_push)
      return fail(s->ctx, GLC_EINVAL, w + ": lane " + std::to_string(i) + ": the chunk is larger than glc_stream_enc_max_push");
    if (!n_new && !fin) continue;
    StreamLanePush a{i, n_new, fin, {}};
    if (!glc::plan_stream_push(s->lanes[i].received, n_new, fin, &a.plan))
      return fail(s->ctx, GLC_EINVAL, w + ": lane " + std::to_string(i) +
                                          ": the reference encoder panics on a stream of <= 512 samples per channel");
    act->push_back(a);
  }
  return GLC_OK;
}

}  // namespace
}  // extern "C++"

int glc_plan_stream_push(uint64_t received, uint64_t n_new, int finish, glc_stream_push_plan *out) {
  if (!out) return GLC_EINVAL;
  *out = glc_stream_push_plan{0, 0, 0};
  if (!glc::plan_stream_push(received, n_new, finish != 0, out)) {
    glc::set_global_error("glc_plan_stream_push: a sum that wraps, or a finish at <= 512 samples per channel (the reference encoder panics)");
    return GLC_EINVAL;
  }
  return GLC_OK;
}

uint64_t glc_stream_enc_max_push(uint16_t channels) {
  // a push of n samples completes at most ceil(n / 1024) + 1 frames; with its junk slot and the round's slot in front
  // that is ceil(n / 1024) + 3 virtual frames of the encode_chunk_frames a round holds
  return channels ? (encode_chunk_frames(channels) - 4) * glc::kHop : 0;
}

int glc_stream_enc_open(glc_ctx *ctx, uint16_t channels, uint64_t n_streams, glc_stream_enc **out) {
  return stream_open(ctx, "glc_stream_enc_open", channels, n_streams, 2ull * glc::kFrame * channels * sizeof(float), out);
}

void glc_stream_enc_close(glc_stream_enc *s) { stream_close(s); }

int glc_stream_enc_reset(glc_stream_enc *s, uint64_t stream) {
  if (!s) return GLC_EINVAL;
  if (stream >= s->n) return fail(s->ctx, GLC_EINVAL, "glc_stream_enc_reset: no such stream");
  StreamLane &L = s->lanes[stream];
  L.received = 0, L.done = 0, L.finished = false, L.total = 0;
  L.blobs.clear();
  return GLC_OK;
}

// The checks of a device push, then the core.
static int stream_push_device_checked(glc_stream_enc *s, const char *who, const void *d_pcm, glc_pcm_format fmt, uint32_t bits,
                                      const glc_clip_layout *in, const uint8_t *finish, void *d_arena, uint64_t arena_bytes,
                                      uint64_t *d_cursor, glc_store_entry *d_entries, glc_stream_seg *segs, uint64_t *n_segs) {
  glc_ctx *ctx = s->ctx;
  const std::string w(who);
  if (!in || !d_pcm || !d_arena || !d_cursor || !d_entries || !segs || !n_segs) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (const char *bad = fmt_fault(fmt, bits)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  if (in->n_clips != s->n || in->channels != s->ch)
    return fail(ctx, GLC_EINVAL, w + ": the layout's n_clips and channels must be the session's");
  const RtbPcm pcm{d_pcm, fmt, bits};
  if (const char *bad = store_fill_misaligned(pcm, d_arena, d_cursor, d_entries)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  const RtbLayout li{in};
  return on_device(ctx, w, [&]() -> int {
    std::vector<StreamLanePush> act;
    if (const int rc = stream_plan_lanes(s, w, in->lengths, in->length, finish, &act)) return rc;
    for (uint64_t i = 0; i < s->n; ++i) {
      if (li.len(i) == 0) continue;  // a lane that brings nothing has no chunk to place
      if (const char *bad = stride_fault(li, i)) return fail(ctx, GLC_EINVAL, w + ": lane " + std::to_string(i) + ": " + bad);
    }
    if (const char *bad = store_fill_overlap(pcm, li, d_arena, arena_bytes, d_entries)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
    return stream_push_core(s, pcm, li, act, d_arena, arena_bytes, d_cursor, d_entries, segs, n_segs);
  });
}

int glc_stream_enc_push_device(glc_stream_enc *s, const void *d_pcm, glc_pcm_format fmt, uint32_t bits, const glc_clip_layout *in,
                               const uint8_t *finish, void *d_arena, uint64_t arena_bytes, uint64_t *d_cursor,
                               glc_store_entry *d_entries, glc_stream_seg *segs, uint64_t *n_segs) {
  if (!s) return GLC_EINVAL;
  if (const int rc = stream_mode_gate(s, "glc_stream_enc_push_device", 2)) return rc;
  const int rc = stream_push_device_checked(s, "glc_stream_enc_push_device", d_pcm, fmt, bits, in, finish, d_arena, arena_bytes, d_cursor,
                                            d_entries, segs, n_segs);
  if (rc == GLC_OK) s->mode = 2;
  return rc;
}

int glc_stream_enc_push(glc_stream_enc *s, const void *const *pcm, glc_pcm_format fmt, uint32_t bits, const uint64_t *n_samples,
                        const uint8_t *finish) {
  if (!s) return GLC_EINVAL;
  glc_ctx *ctx = s->ctx;
  const std::string w("glc_stream_enc_push");
  if (const int rc = stream_mode_gate(s, w, 1)) return rc;
  if (!pcm || !n_samples) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (const char *bad = fmt_fault(fmt, bits)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  const uint32_t ch = s->ch;
  const size_t elem = pcm_elem(fmt);
  const uint64_t max_push = glc_stream_enc_max_push(static_cast<uint16_t>(ch));
  return on_device(ctx, w, [&]() -> int {
    std::vector<uint64_t> left(s->n), lens(s->n);
    bool any = false;
    for (uint64_t i = 0; i < s->n; ++i) {
      const std::string lane = w + ": lane " + std::to_string(i);
      const StreamLane &L = s->lanes[i];
      const bool fin = finish && finish[i];
      if (n_samples[i] % ch) return fail(ctx, GLC_EINVAL, lane + ": n_samples is not a multiple of channels");
      if (n_samples[i] && !pcm[i]) return fail(ctx, GLC_EINVAL, lane + ": null samples");
      if (n_samples[i] && !aligned(pcm[i], elem)) return fail(ctx, GLC_EINVAL, lane + ": samples are not aligned");
      if ((n_samples[i] || fin) && L.finished) return fail(ctx, GLC_EINVAL, lane + ": the stream is finished and has not been taken");
      left[i] = n_samples[i] / ch;
      glc_stream_push_plan plan;
      if ((left[i] || fin) && !glc::plan_stream_push(L.received, left[i], fin, &plan))
        return fail(ctx, GLC_EINVAL, lane + ": the reference encoder panics on a stream of <= 512 samples per channel");
      any = any || left[i] || fin;
    }
    if (!any) {
      rt_forget_streams(ctx);
      s->mode = 1;
      return GLC_OK;
    }
    std::vector<uint8_t> fin_now(s->n);
    std::vector<uint64_t> at(s->n, 0);  // samples per channel of pcm[i] already pushed
    std::vector<glc_stream_seg> segs(s->n);
    std::vector<glc_store_entry> ents(s->n);
    for (bool more = true; more;) {
      more = false;
      uint64_t longest = 0, arena_need = 64;
      for (uint64_t i = 0; i < s->n; ++i) {
        lens[i] = std::min(left[i], max_push);
        fin_now[i] = finish && finish[i] && left[i] == lens[i] && !s->lanes[i].finished;
        if (left[i] > lens[i]) more = true;
        longest = std::max(longest, lens[i]);
        glc_stream_push_plan plan{};
        if ((lens[i] || fin_now[i]) && glc::plan_stream_push(s->lanes[i].received, lens[i], fin_now[i], &plan) && plan.n_frames)
          arena_need += glc::align64(glc::compact_layout(ch, plan.n_frames).bound);
      }
      const uint64_t stride = std::max<uint64_t>(longest * ch, 1);
      const size_t up_bytes = static_cast<size_t>(s->n * stride * elem);
      GLC_HIP(ctx, s->up.reserve(up_bytes));
      int rc = rt_reserve(ctx, s->d_pcm, up_bytes);
      if (rc == GLC_OK) rc = rt_reserve(ctx, s->arena, arena_need);
      if (rc == GLC_OK) rc = rt_reserve(ctx, s->d_meta, 64 + s->n * sizeof(glc_store_entry));
      if (rc != GLC_OK) return rc;
      for (uint64_t i = 0; i < s->n; ++i)
        if (lens[i])
          std::memcpy(static_cast<uint8_t *>(s->up.p) + i * stride * elem, static_cast<const uint8_t *>(pcm[i]) + at[i] * ch * elem,
                      lens[i] * ch * elem);
      uint64_t *d_cursor = static_cast<uint64_t *>(s->d_meta.p);
      glc_store_entry *d_entries = reinterpret_cast<glc_store_entry *>(static_cast<uint8_t *>(s->d_meta.p) + 64);
      GLC_HIP(ctx, hipMemcpyAsync(s->d_pcm.p, s->up.p, up_bytes, hipMemcpyHostToDevice, ctx->stream));
      GLC_HIP(ctx, hipMemsetAsync(d_cursor, 0, 8, ctx->stream));
      glc_clip_layout lay{s->n, static_cast<uint16_t>(ch), 0, stride, 0, 0, lens.data()};
      const RtbLayout li{&lay};
      const RtbPcm dp{s->d_pcm.p, fmt, bits};
      std::vector<StreamLanePush> act;
      rc = stream_plan_lanes(s, w, lens.data(), 0, fin_now.data(), &act);
      uint64_t n_segs = 0;
      std::vector<uint64_t> totals(s->n);
      for (uint64_t i = 0; i < s->n; ++i) totals[i] = s->lanes[i].received + lens[i];
      if (rc == GLC_OK) rc = stream_push_core(s, dp, li, act, s->arena.p, s->arena.cap, d_cursor, d_entries, segs.data(), &n_segs);
      if (rc != GLC_OK) return rc;
      s->mode = 1;
      for (uint64_t i = 0; i < s->n; ++i) {
        at[i] += lens[i], left[i] -= lens[i];
        if (fin_now[i]) s->lanes[i].finished = true, s->lanes[i].total = totals[i];
      }
      if (n_segs) {
        GLC_HIP(ctx, hipMemcpyAsync(ents.data(), d_entries, n_segs * sizeof(glc_store_entry), hipMemcpyDeviceToHost, ctx->stream));
        GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        uint64_t down_bytes = 0;
        for (uint64_t j = 0; j < n_segs; ++j) {
          if (!ents[j].stored || ents[j].offset + ents[j].bytes > s->arena.cap)
            return fail(ctx, GLC_EHIP, w + ": a segment did not fit the session's arena");
          down_bytes = std::max(down_bytes, ents[j].offset + ents[j].bytes);
        }
        GLC_HIP(ctx, s->down.reserve(down_bytes));
        GLC_HIP(ctx, hipMemcpyAsync(s->down.p, s->arena.p, down_bytes, hipMemcpyDeviceToHost, ctx->stream));
        GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t j = 0; j < n_segs; ++j) {
          StreamBlob b{segs[j].first_frame, segs[j].n_frames, std::vector<uint64_t>((ents[j].bytes + 7) / 8), ents[j].bytes};
          std::memcpy(b.words.data(), static_cast<const uint8_t *>(s->down.p) + ents[j].offset, ents[j].bytes);
          s->lanes[segs[j].stream].blobs.push_back(std::move(b));
        }
      } else {
        // the pinned chunks must have left before the next round of this loop, or the caller's next push, rewrites them
        GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
      }
    }
    return GLC_OK;
  });
}

int glc_stream_enc_segments(const glc_stream_enc *s, uint64_t stream, uint64_t *n_blobs) {
  if (!s) return GLC_EINVAL;
  if (!n_blobs || stream >= s->n) return fail(s->ctx, GLC_EINVAL, "glc_stream_enc_segments: null argument or no such stream");
  *n_blobs = s->lanes[stream].blobs.size();
  return GLC_OK;
}

int glc_stream_enc_segment(const glc_stream_enc *s, uint64_t stream, uint64_t k, const void **blob, uint64_t *bytes,
                           uint64_t *first_frame, uint64_t *n_frames) {
  if (!s) return GLC_EINVAL;
  if (stream >= s->n || k >= s->lanes[stream].blobs.size()) return fail(s->ctx, GLC_EINVAL, "glc_stream_enc_segment: no such segment");
  const StreamBlob &b = s->lanes[stream].blobs[k];
  if (blob) *blob = b.words.data();
  if (bytes) *bytes = b.bytes;
  if (first_frame) *first_frame = b.first_frame;
  if (n_frames) *n_frames = b.n_frames;
  return GLC_OK;
}

int glc_stream_enc_frames(glc_stream_enc *s, uint64_t stream, glc_frames **out) {
  if (!s) return GLC_EINVAL;
  if (!out || stream >= s->n) return fail(s->ctx, GLC_EINVAL, "glc_stream_enc_frames: null argument or no such stream");
  *out = nullptr;
  StreamLane &L = s->lanes[stream];
  if (!L.finished) return fail(s->ctx, GLC_EINVAL, "glc_stream_enc_frames: the stream is not finished");
  if (L.blobs.size() > 0xFFFFFFFFull) return fail(s->ctx, GLC_EINVAL, "glc_stream_enc_frames: too many segments");
  try {
    std::vector<const void *> blobs(L.blobs.size());
    std::vector<uint64_t> bytes(L.blobs.size());
    for (size_t k = 0; k < L.blobs.size(); ++k) blobs[k] = L.blobs[k].words.data(), bytes[k] = L.blobs[k].bytes;
    const int rc = glc::frames_from_compact(s->ctx->sample_rate, L.total * s->ch, static_cast<uint16_t>(s->ch), blobs.data(), bytes.data(),
                                            static_cast<uint32_t>(blobs.size()), /*trusted=*/true, out);
    if (rc != GLC_OK) return fail(s->ctx, rc, std::string("glc_stream_enc_frames: ") + glc_last_error(nullptr));
  } catch (const std::bad_alloc &) {
    return fail(s->ctx, GLC_ENOMEM, "glc_stream_enc_frames: host allocation failed");
  }
  L.finished = false, L.total = 0;
  L.blobs.clear();
  return GLC_OK;
}

// ------------------------------------------------------------------------------ streaming decode

struct glc_stream_dec : StreamSession {
  // lane_buf is the carry, [lane][2][ch][1024] floats: (a) the last hop's finished sums, (b) the last frame's second half
  std::vector<uint64_t> done;  // frames taken per lane
  void size_lanes(uint64_t k) { done.assign(k, 0); }
  DevBuf arena, d_entries, d_out;  // host pushes
  uint64_t carry_at(uint64_t lane) const { return lane * 2ull * glc::kHop * ch; }
};

extern "C++" {
namespace {

// What a push does with lane `lane`: frames [D, D + n) from segments [seg0, seg0 + nseg), and what that emits.
struct DecLanePush {
  uint64_t lane, D, n;
  bool fin;
  uint64_t seg0, nseg;
  glc_stream_dec_plan plan;
};

// The part of a lane's push that one round decodes: frames [D, D + n) in block slots [slot0, slot0 + n), the lane's
// two pseudo-slots at `pseudo` (D > 0), its samples from `before` samples per channel behind the lane's output start.
struct DecPiece {
  uint64_t lane, D, n, slot0, pseudo, before;
  bool fin;
  glc_stream_dec_plan plan;
};

// The core of both pushes: everything is validated.  Queues the planner and the rounds; updates the lanes.
template <typename T>
int stream_dec_core(glc_stream_dec *s, const std::vector<DecLanePush> &act, const glc_stream_seg *segs, uint64_t n_segs,
                    const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries, const uint64_t *total_len, T *d_out,
                    const RtbLayout &out) {
  glc_ctx *ctx = s->ctx;
  const uint32_t ch = s->ch;
  const uint64_t per_hop = uint64_t(glc::kHop) * ch;
  const size_t slot = static_cast<size_t>(ch) * glc::kFrame;
  // the items of the round packer, in lane order: a lane's segments, or ONE item of no frames for a finish that brings none
  struct Item {
    size_t a;      // index into act
    int64_t seg;   // index into segs, -1: none
    uint64_t frames;
  };
  std::vector<Item> items;
  for (size_t a = 0; a < act.size(); ++a) {
    for (uint64_t j = 0; j < act[a].nseg; ++j) items.push_back(Item{a, static_cast<int64_t>(act[a].seg0 + j), segs[act[a].seg0 + j].n_frames});
    if (!act[a].nseg) items.push_back(Item{a, -1, 0});
  }
  struct Round : RoundSpan {
    size_t o_desc = 0, o_load = 0, o_save = 0;
    uint64_t n_desc = 0, n_load = 0, n_save = 0, seg_first = 0, seg_n = 0;
    std::vector<DecPiece> pieces;
  };
  auto rounds = plan_rounds<Round>(items.size(), [&](uint64_t k) { return items[k].frames; }, kDecodeChunkFrames + 1, 0);
  for (const Round &R : rounds)
    if (R.lng) return fail(ctx, GLC_EHIP, "glc_stream_dec_push: internal: a segment does not fit a round");
  rt_forget_streams(ctx);
  ctx->cd_status_n = 0;
  auto commit = [&] {
    for (const DecLanePush &a : act) s->done[a.lane] = a.fin ? 0 : a.D + a.n;
  };
  if (rounds.empty()) return GLC_OK;  // nothing arrives and nothing finishes
  // the pieces: a lane that straddles two rounds is two consecutive pushes of it, the carry handed on through the
  // session's buffer by the first round's save and the second round's load
  std::vector<uint64_t> taken(act.size(), 0);
  TableOffsets offs;
  const size_t o_segs = offs.take(std::max<uint64_t>(n_segs, 1) * sizeof(glc::StreamDecSeg));
  uint64_t max_M = 0, max_slots = 0, max_frames = 0, seg_at = 0;
  for (Round &R : rounds) {
    uint64_t real = 0;
    R.seg_first = seg_at;
    for (uint64_t k = R.first; k < R.first + R.n; ++k) {
      const Item &it = items[k];
      const DecLanePush &a = act[it.a];
      if (R.pieces.empty() || R.pieces.back().lane != a.lane)
        R.pieces.push_back(DecPiece{a.lane, a.D + taken[it.a], 0, real, 0, glc::stream_dec_emitted(a.D + taken[it.a]) - a.plan.first_sample, false, {}});
      DecPiece &p = R.pieces.back();
      p.n += it.frames, taken[it.a] += it.frames, real += it.frames;
      if (it.seg >= 0) ++R.seg_n, ++seg_at;
      p.fin = a.fin && taken[it.a] == a.n && (k + 1 == items.size() || items[k + 1].a != it.a);
    }
    for (size_t q = 0; q < R.pieces.size(); ++q) {
      DecPiece &p = R.pieces[q];
      p.pseudo = R.n_real + 2 * q;
      glc::plan_stream_dec_push(p.D, p.n, p.fin, p.fin ? total_len[p.lane] : 0, &p.plan);  // cannot fail: the lane's plan passed
      const glc::Trim trim{glc::kHop / 2 + ch * p.plan.first_sample, ch * p.plan.n_samples};
      R.n_desc += count_hop_descs(trim, per_hop, 0, p.D + p.n + 1);
      if (p.D) ++R.n_load;
      if (!p.fin) ++R.n_save;
    }
    R.o_desc = offs.take(R.n_desc * sizeof(glc::HopDescStrided));
    R.o_load = offs.take(R.n_load * sizeof(glc::StreamCarry));
    R.o_save = offs.take(R.n_save * sizeof(glc::StreamCarry));
    max_M = std::max(max_M, R.n_real * ch);
    max_slots = std::max<uint64_t>(max_slots, R.n_real + 2 * R.pieces.size());
    max_frames = std::max(max_frames, R.n_real);
  }
  const size_t img_bytes = offs.size();
  // behind the image, written by the planner kernel: the directory and the verdicts
  const size_t o_dir = offs.take(std::max<uint64_t>(n_segs, 1) * sizeof(glc::CompactBlob));
  const size_t o_verdict = offs.take(std::max<uint64_t>(n_segs, 1) * sizeof(uint32_t));
  int rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_compact_bytes(static_cast<uint32_t>(max_M)));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->blocks, max_slots * slot * sizeof(float));
  if (rc == GLC_OK && max_frames) rc = reserve_d1_plan(ctx, max_frames, ch);
  TableImage &image = ctx->rtb_image;
  if (rc == GLC_OK) rc = image.begin(ctx, offs.size());
  if (rc == GLC_OK && n_segs) rc = rt_reserve(ctx, ctx->cd_status, n_segs * sizeof(glc::CompactStatus));
  if (rc != GLC_OK) return rc;
  const bool out_planes = out.planes();
  auto *seg_tab = image.host<glc::StreamDecSeg>(o_segs);
  for (const Round &R : rounds) {
    uint64_t row = 0, j = R.seg_first;
    for (uint64_t k = R.first; k < R.first + R.n; ++k) {
      if (items[k].seg < 0) continue;
      seg_tab[j++] = glc::StreamDecSeg{static_cast<uint32_t>(row), static_cast<uint32_t>(items[k].frames * ch)};
      row += items[k].frames * ch;
    }
    auto *desc = image.host<glc::HopDescStrided>(R.o_desc);
    auto *load = image.host<glc::StreamCarry>(R.o_load);
    auto *save = image.host<glc::StreamCarry>(R.o_save);
    for (const DecPiece &p : R.pieces) {
      const uint64_t nf = p.D + p.n;
      const glc::Trim trim{glc::kHop / 2 + ch * p.plan.first_sample, ch * p.plan.n_samples};
      const uint64_t dst = out.at(p.lane) + (out_planes ? p.before : p.before * ch);
      const int32_t slot_a = static_cast<int32_t>(p.pseudo), slot_b = slot_a + 1;
      if (trim.n) {
        const uint64_t h0 = trim.start / per_hop, h1 = (trim.start + trim.n - 1) / per_hop + 1;
        for (uint64_t h = h0; h < h1; ++h) {
          if (!glc::hop_desc(desc, nf, ch, trim, h, static_cast<int64_t>(p.slot0) - static_cast<int64_t>(p.D), dst, out_planes,
                             out.l->channel_stride))
            continue;
          // the hops that reach back behind the push: hop D - 1 is the carried sums alone - the second half of a slot
          // with no `cur`, so that D2 adds nothing to them -, hop D takes frame D - 1's second half from the carry
          if (p.D && h + 1 == p.D) desc->prev = slot_a, desc->cur = -1;
          if (p.D && h == p.D) desc->prev = slot_b;
          ++desc;
        }
      }
      if (p.D) *load++ = glc::StreamCarry{slot_a, -1, s->carry_at(p.lane)};
      if (!p.fin)  // n >= 1: a push that does not finish brings frames
        *save++ = glc::StreamCarry{p.n >= 2 ? static_cast<int32_t>(p.slot0 + p.n - 2) : (p.D ? slot_b : -1),
                                   static_cast<int32_t>(p.slot0 + p.n - 1), s->carry_at(p.lane)};
    }
    if (static_cast<uint64_t>(desc - image.host<glc::HopDescStrided>(R.o_desc)) != R.n_desc)
      return fail(ctx, GLC_EHIP, "glc_stream_dec_push: hop count arithmetic is inconsistent");
  }
  hipStream_t st = ctx->stream;
  rc = image.send(ctx, img_bytes);
  if (rc != GLC_OK) return rc;
  uint8_t *d_tab = static_cast<uint8_t *>(ctx->rtb_tab.p);
  auto *d_dir = reinterpret_cast<glc::CompactBlob *>(d_tab + o_dir);
  auto *d_verdict = reinterpret_cast<uint32_t *>(d_tab + o_verdict);
  if (n_segs)
    GLC_HIP(ctx, glc::launch_stream_dec_plan(reinterpret_cast<uintptr_t>(d_arena), arena_bytes, d_entries, image.dev<glc::StreamDecSeg>(o_segs),
                                             static_cast<uint32_t>(n_segs), d_dir, d_verdict, st));
  auto *d_status = static_cast<glc::CompactStatus *>(ctx->cd_status.p);
  float *blocks = static_cast<float *>(ctx->blocks.p);
  float *carry = static_cast<float *>(s->lane_buf.p);
  for (const Round &R : rounds) {
    const uint32_t M = static_cast<uint32_t>(R.n_real * ch);
    if (M) {
      glc::DecodeRows rows{};
      // pairs and raw planes are addressed from the arena: every usable blob lies inside it, 64-byte aligned
      GLC_HIP(ctx, glc::launch_rows_from_compact(d_dir + R.seg_first, glc::CompactBlob{}, static_cast<uint32_t>(R.seg_n), M, ch,
                                                 glc::R2Mode{false, 0u, d_verdict + R.seg_first}, d_arena, ctx->rt_rows.p,
                                                 d_status + R.seg_first, st, &rows));
      GLC_HIP(ctx, launch_d1_rows(ctx, rows, 0, M, ch, blocks, st));
    }
    GLC_HIP(ctx, glc::launch_stream_dec_carry(false, image.dev<glc::StreamCarry>(R.o_load), static_cast<uint32_t>(R.n_load), ch, blocks, carry, st));
    if (R.n_desc)
      GLC_HIP(ctx, glc::launch_overlap_add_strided(blocks, image.dev<glc::HopDescStrided>(R.o_desc), static_cast<uint32_t>(R.n_desc), ch,
                                                   out_planes, d_out, st));
    GLC_HIP(ctx, glc::launch_stream_dec_carry(true, image.dev<glc::StreamCarry>(R.o_save), static_cast<uint32_t>(R.n_save), ch, blocks, carry, st));
  }
  ctx->cd_status_n = n_segs;
  commit();
  return GLC_OK;
}

// What both pushes check of the segments and the lanes, and build for the core.  lens: the layout's, or null (the
// host push sizes its own output).
int stream_dec_plan_lanes(glc_stream_dec *s, const std::string &w, const glc_stream_seg *segs, uint64_t n_segs, const uint8_t *finish,
                          const uint64_t *total_len, std::vector<DecLanePush> *act) {
  glc_ctx *ctx = s->ctx;
  const uint64_t max_push = glc_stream_dec_max_push(static_cast<uint16_t>(s->ch));
  std::vector<DecLanePush> by_lane;
  uint64_t j = 0;
  for (uint64_t j0 = 0; j0 < n_segs; j0 = j) {
    const uint64_t lane = segs[j0].stream;
    const std::string name = w + ": segment " + std::to_string(j0);
    if (lane >= s->n) return fail(ctx, GLC_EINVAL, name + ": no such stream");
    if (!by_lane.empty() && lane <= by_lane.back().lane) return fail(ctx, GLC_EINVAL, name + ": the segments do not ascend by stream and frame");
    DecLanePush a{lane, s->done[lane], 0, false, j0, 0, {}};
    for (j = j0; j < n_segs && segs[j].stream == lane; ++j) {
      if (segs[j].n_frames == 0) return fail(ctx, GLC_EINVAL, w + ": segment " + std::to_string(j) + ": no frames");
      if (segs[j].first_frame != a.D + a.n)
        return fail(ctx, GLC_EINVAL, w + ": segment " + std::to_string(j) + ": it does not start where its lane's frames end");
      if (segs[j].n_frames > max_push - a.n)
        return fail(ctx, GLC_EINVAL, w + ": lane " + std::to_string(lane) + ": more frames than glc_stream_dec_max_push");
      a.n += segs[j].n_frames, ++a.nseg;
    }
    by_lane.push_back(a);
  }
  size_t at = 0;
  for (uint64_t i = 0; i < s->n; ++i) {
    const bool fin = finish && finish[i];
    DecLanePush a{i, s->done[i], 0, fin, 0, 0, {}};
    if (at < by_lane.size() && by_lane[at].lane == i) a = by_lane[at++], a.fin = fin;
    if (!a.n && !fin) continue;
    if (fin && !total_len) return fail(ctx, GLC_EINVAL, w + ": a finish without total_len");
    if (!glc::plan_stream_dec_push(a.D, a.n, fin, fin ? total_len[i] : 0, &a.plan))
      return fail(ctx, GLC_EINVAL, w + ": lane " + std::to_string(i) + ": total_len does not plan to the frames the lane has taken");
    act->push_back(a);
  }
  return GLC_OK;
}

template <typename T>
int stream_dec_push_device_checked(glc_stream_dec *s, const std::string &w, const void *d_arena, uint64_t arena_bytes,
                                   const glc_store_entry *d_entries, const glc_stream_seg *segs, uint64_t n_segs, const uint8_t *finish,
                                   const uint64_t *total_len, T *d_out, const glc_clip_layout *out) {
  glc_ctx *ctx = s->ctx;
  if (!out || !d_out || (n_segs && (!d_arena || !d_entries || !segs))) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (out->n_clips != s->n || out->channels != s->ch) return fail(ctx, GLC_EINVAL, w + ": the layout's n_clips and channels must be the session's");
  if (!aligned(d_arena, 64)) return fail(ctx, GLC_EINVAL, w + ": d_arena is not 64-byte aligned");
  if (!aligned(d_entries, 8)) return fail(ctx, GLC_EINVAL, w + ": d_entries must be 8-byte aligned");
  if (!aligned(d_out, sizeof(T))) return fail(ctx, GLC_EINVAL, w + ": output pointer not aligned to its sample size");
  if (n_segs > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": too many segments");
  const RtbLayout lo{out};
  return on_device(ctx, w, [&]() -> int {
    std::vector<DecLanePush> act;
    if (const int rc = stream_dec_plan_lanes(s, w, segs, n_segs, finish, total_len, &act)) return rc;
    size_t at = 0;
    for (uint64_t i = 0; i < s->n; ++i) {
      auto refuse = [&](const char *what) { return fail(ctx, GLC_EINVAL, w + ": lane " + std::to_string(i) + ": " + what); };
      uint64_t emits = 0;
      if (at < act.size() && act[at].lane == i) emits = act[at++].plan.n_samples;
      if (lo.len(i) != emits) return refuse("the layout's length is not what the push emits (glc_plan_stream_dec_push)");
      if (!emits) continue;  // a lane that emits nothing has no samples to place
      if (const char *bad = stride_fault(lo, i)) return refuse(bad);
    }
    if (n_segs) {  // a push without segments reads neither the arena nor the entries
      const ByteSpan all = span_of(d_out, lo, sizeof(T));
      if (overlaps(span_of(d_arena, arena_bytes), all)) return fail(ctx, GLC_EINVAL, w + ": the output extent overlaps the arena");
      if (overlaps(span_of(d_entries, n_segs * sizeof(glc_store_entry)), all)) return fail(ctx, GLC_EINVAL, w + ": the output extent overlaps the entries");
    }
    return stream_dec_core<T>(s, act, segs, n_segs, d_arena, arena_bytes, d_entries, total_len, d_out, lo);
  });
}

}  // namespace
}  // extern "C++"

int glc_plan_stream_dec_push(uint64_t frames_done, uint64_t n_frames, int finish, uint64_t total_len, glc_stream_dec_plan *out) {
  if (!out) return GLC_EINVAL;
  *out = glc_stream_dec_plan{0, 0};
  if (!glc::plan_stream_dec_push(frames_done, n_frames, finish != 0, total_len, out)) {
    glc::set_global_error("glc_plan_stream_dec_push: a sum that wraps, or a finish whose total_len does not plan to frames_done + n_frames frames");
    return GLC_EINVAL;
  }
  return GLC_OK;
}

uint64_t glc_stream_dec_max_push(uint16_t channels) {
  // every segment of a lane's push, with the slot the round packer counts for it, fits a decode round
  return channels ? kDecodeChunkFrames : 0;
}

int glc_stream_dec_open(glc_ctx *ctx, uint16_t channels, uint64_t n_streams, glc_stream_dec **out) {
  return stream_open(ctx, "glc_stream_dec_open", channels, n_streams, 2ull * glc::kHop * channels * sizeof(float), out);
}

void glc_stream_dec_close(glc_stream_dec *s) { stream_close(s); }

int glc_stream_dec_reset(glc_stream_dec *s, uint64_t stream) {
  if (!s) return GLC_EINVAL;
  if (stream >= s->n) return fail(s->ctx, GLC_EINVAL, "glc_stream_dec_reset: no such stream");
  s->done[stream] = 0;
  return GLC_OK;
}

int glc_stream_dec_frames_done(const glc_stream_dec *s, uint64_t stream, uint64_t *n) {
  if (!s) return GLC_EINVAL;
  if (!n || stream >= s->n) return fail(s->ctx, GLC_EINVAL, "glc_stream_dec_frames_done: null argument or no such stream");
  *n = s->done[stream];
  return GLC_OK;
}

int glc_stream_dec_push_device(glc_stream_dec *s, const void *d_arena, uint64_t arena_bytes, const glc_store_entry *d_entries,
                               const glc_stream_seg *segs, uint64_t n_segs, const uint8_t *finish, const uint64_t *total_len, void *d_out,
                               glc_pcm_format out_fmt, const glc_clip_layout *out) {
  if (!s) return GLC_EINVAL;
  const std::string w("glc_stream_dec_push_device");
  if (const int rc = stream_mode_gate(s, w, 2)) return rc;
  if (const char *bad = out_fmt_fault(out_fmt)) return fail(s->ctx, GLC_EINVAL, w + ": " + bad);
  const int rc = out_fmt == GLC_PCM_F32 ? stream_dec_push_device_checked(s, w, d_arena, arena_bytes, d_entries, segs, n_segs, finish, total_len,
                                                                         static_cast<float *>(d_out), out)
                                        : stream_dec_push_device_checked(s, w, d_arena, arena_bytes, d_entries, segs, n_segs, finish, total_len,
                                                                         static_cast<int16_t *>(d_out), out);
  if (rc == GLC_OK) s->mode = 2;
  return rc;
}

int glc_stream_dec_push(glc_stream_dec *s, const void *const *blobs, const uint64_t *blob_bytes, const glc_stream_seg *segs, uint64_t n_segs,
                        const uint8_t *finish, const uint64_t *total_len, void *const *pcm_out, glc_pcm_format out_fmt, uint64_t *n_out) {
  if (!s) return GLC_EINVAL;
  glc_ctx *ctx = s->ctx;
  const std::string w("glc_stream_dec_push");
  if (const int rc = stream_mode_gate(s, w, 1)) return rc;
  if (const char *bad = out_fmt_fault(out_fmt)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  if (!pcm_out || !n_out || (n_segs && (!blobs || !blob_bytes || !segs))) return fail(ctx, GLC_EINVAL, w + ": null argument");
  if (n_segs > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": too many segments");
  const uint32_t ch = s->ch;
  const size_t elem = pcm_elem(out_fmt);
  return on_device(ctx, w, [&]() -> int {
    std::vector<DecLanePush> act;
    if (const int rc = stream_dec_plan_lanes(s, w, segs, n_segs, finish, total_len, &act)) return rc;
    // the session's arena: the blobs back to back at multiples of 64, the entries behind them in the same pinned image
    std::vector<glc_store_entry> ents(n_segs);
    uint64_t arena_need = 64;
    for (uint64_t j = 0; j < n_segs; ++j) {
      if (!blobs[j]) return fail(ctx, GLC_EINVAL, w + ": segment " + std::to_string(j) + ": null blob");
      if (blob_bytes[j] > (1ull << 46)) return fail(ctx, GLC_EINVAL, w + ": segment " + std::to_string(j) + ": blob_bytes too large");
      ents[j] = glc_store_entry{arena_need - 64, blob_bytes[j], 0, 0, 1u};
      arena_need += glc::align64(blob_bytes[j]);
    }
    std::vector<uint64_t> lens(s->n, 0);
    uint64_t longest = 0;
    for (const DecLanePush &a : act) {
      if (a.plan.n_samples && !pcm_out[a.lane]) return fail(ctx, GLC_EINVAL, w + ": lane " + std::to_string(a.lane) + ": null output");
      lens[a.lane] = a.plan.n_samples, longest = std::max(longest, a.plan.n_samples);
    }
    for (uint64_t i = 0; i < s->n; ++i) n_out[i] = lens[i] * ch;
    const uint64_t stride = (std::max<uint64_t>(longest * ch, 1) + 3) / 4 * 4;
    const size_t ents_at = static_cast<size_t>(arena_need - 64), up_bytes = ents_at + n_segs * sizeof(glc_store_entry);
    const size_t out_bytes = static_cast<size_t>(s->n * stride * elem);
    GLC_HIP(ctx, s->up.reserve(std::max<size_t>(up_bytes, 64)));
    GLC_HIP(ctx, s->down.reserve(out_bytes));
    int rc = rt_reserve(ctx, s->arena, std::max<size_t>(up_bytes, 64));
    if (rc == GLC_OK) rc = rt_reserve(ctx, s->d_out, out_bytes);
    if (rc != GLC_OK) return rc;
    uint8_t *up = static_cast<uint8_t *>(s->up.p);
    for (uint64_t j = 0; j < n_segs; ++j) std::memcpy(up + ents[j].offset, blobs[j], blob_bytes[j]);
    if (n_segs) std::memcpy(up + ents_at, ents.data(), n_segs * sizeof(glc_store_entry));
    if (up_bytes) GLC_HIP(ctx, hipMemcpyAsync(s->arena.p, up, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    const auto *d_entries = reinterpret_cast<const glc_store_entry *>(static_cast<const uint8_t *>(s->arena.p) + ents_at);
    glc_clip_layout lay{s->n, static_cast<uint16_t>(ch), 0, stride, 0, 0, lens.data()};
    const RtbLayout lo{&lay};
    rc = out_fmt == GLC_PCM_F32 ? stream_dec_core<float>(s, act, segs, n_segs, s->arena.p, ents_at, d_entries, total_len,
                                                         static_cast<float *>(s->d_out.p), lo)
                                : stream_dec_core<int16_t>(s, act, segs, n_segs, s->arena.p, ents_at, d_entries, total_len,
                                                           static_cast<int16_t *>(s->d_out.p), lo);
    if (rc != GLC_OK) return rc;
    s->mode = 1;
    GLC_HIP(ctx, hipMemcpyAsync(s->down.p, s->d_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < s->n; ++i)
      if (lens[i]) std::memcpy(pcm_out[i], static_cast<const uint8_t *>(s->down.p) + i * stride * elem, lens[i] * ch * elem);
    return GLC_OK;
  });
}

int glc_debug_stream_dec_carry_device(glc_ctx *ctx, int save, int32_t prev, int32_t cur, uint16_t channels, float *d_blocks,
                                      uint64_t n_slots, float *d_carry) {
  const std::string w("glc_debug_stream_dec_carry_device");
  if (!ctx) return GLC_EINVAL;
  if (!d_blocks || !d_carry || channels == 0) return fail(ctx, GLC_EINVAL, w + ": null argument or channels == 0");
  if (!all_aligned(16, d_blocks, d_carry)) return fail(ctx, GLC_EINVAL, w + ": blocks and carry must be 16-byte aligned");
  const int64_t n = static_cast<int64_t>(std::min<uint64_t>(n_slots, 0x7FFFFFFFull));
  const bool ok = save ? (prev >= -1 && prev < n && cur >= 0 && cur < n) : (prev >= 0 && int64_t(prev) + 1 < n);
  if (!ok) return fail(ctx, GLC_EINVAL, w + ": a slot outside the blocks");
  DeviceGuard guard(ctx->device);
  DevBuf d_desc;
  GLC_HIP(ctx, d_desc.reserve(sizeof(glc::StreamCarry)));
  const glc::StreamCarry desc{prev, save ? cur : -1, 0ull};
  GLC_HIP(ctx, hipMemcpyAsync(d_desc.p, &desc, sizeof(desc), hipMemcpyHostToDevice, ctx->stream));
  GLC_HIP(ctx, glc::launch_stream_dec_carry(save != 0, static_cast<const glc::StreamCarry *>(d_desc.p), 1, channels, d_blocks, d_carry,
                                            ctx->stream));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GLC_OK;
}

uint64_t glc_ctx_resident_stream(const glc_ctx *ctx) { return ctx ? ctx->dec_uid : 0; }

int glc_decode_resident(glc_ctx *ctx, uint64_t stream_id, float *pcm_out, uint64_t cap, uint64_t *n_out) {
  if (!ctx || (!pcm_out && cap)) return fail(ctx, GLC_EINVAL, "glc_decode_resident: null argument");
  if (stream_id == 0 || ctx->dec_uid != stream_id)
    return fail(ctx, GLC_EINVAL, "glc_decode_resident: that stream is not resident on this context");
  ctx->stream_open = false;
  return decode_prepared_to_host(ctx, pcm_out, cap, n_out, "glc_decode_resident");
}

int glc_decode_device(glc_ctx *ctx, const glc_frames *in, float *d_all, uint64_t cap_all, uint64_t *start,
                      uint64_t *n_out) {
  if (!ctx || !in || !d_all) return fail(ctx, GLC_EINVAL, "glc_decode_device: null argument");
  ctx->stream_open = false;
  if (cap_all < (in->n_frames + 1) * static_cast<uint64_t>(glc::kHop) * in->channels)
    return fail(ctx, GLC_EINVAL, "glc_decode_device: output buffer too small");
  const glc::Trim trim = glc::gapless_trim(in->n_frames, in->channels, in->encoder_delay, in->original_length);
  if (start) *start = trim.start;
  if (n_out) *n_out = trim.n;
  int rc = decode_prepare(ctx, in);
  if (rc != GLC_OK) return rc;
  return decode_hops_prepared(ctx, 0, in->n_frames + 1, d_all);
}

int glc_decode_range_device(glc_ctx *ctx, const glc_frames *in, uint64_t hop_begin, uint64_t hop_end,
                            float *d_out, uint64_t cap) {
  return decode_range_device(ctx, in, hop_begin, hop_end, d_out, cap, "glc_decode_range_device");
}

int glc_decode_range_device_i16(glc_ctx *ctx, const glc_frames *in, uint64_t hop_begin, uint64_t hop_end,
                                int16_t *d_out, uint64_t cap) {
  return decode_range_device(ctx, in, hop_begin, hop_end, d_out, cap, "glc_decode_range_device_i16");
}

int glc_imdct_device(glc_ctx *ctx, const glc_frames *in, uint64_t frame_begin, uint64_t frame_end,
                     float *d_blocks) {
  if (!ctx || !in || !d_blocks) return fail(ctx, GLC_EINVAL, "glc_imdct_device: null argument");
  ctx->stream_open = false;
  if (frame_begin > frame_end || frame_end > in->n_frames)
    return fail(ctx, GLC_EINVAL, "glc_imdct_device: frame range out of bounds");
  int rc = decode_prepare(ctx, in);
  if (rc != GLC_OK) return rc;
  DeviceGuard guard(ctx->device);
  const uint32_t ch = ctx->dec_ch;
  return launch_d1(ctx, static_cast<uint32_t>(frame_begin * ch), static_cast<uint32_t>((frame_end - frame_begin) * ch), d_blocks);
}

int glc_debug_overlap_add_device(glc_ctx *ctx, const float *d_blocks, int64_t blk_frame0, uint64_t n_block_frames,
                                 uint64_t n_frames, uint16_t channels, uint64_t hop_begin, uint64_t hop_end, float *d_out,
                                 uint64_t cap) {
  if (!ctx) return GLC_EINVAL;
  if (!d_blocks || !d_out) return fail(ctx, GLC_EINVAL, "glc_debug_overlap_add_device: null argument");
  if (channels == 0) return fail(ctx, GLC_EINVAL, "glc_debug_overlap_add_device: channels == 0");
  if (hop_begin > hop_end || hop_end > n_frames + 1 || n_frames > 0xFFFFFFFFull)
    return fail(ctx, GLC_EINVAL, "glc_debug_overlap_add_device: hop range out of bounds");
  if (cap < (hop_end - hop_begin) * glc::kHop * channels)
    return fail(ctx, GLC_EINVAL, "glc_debug_overlap_add_device: output buffer too small");
  if (hop_begin < hop_end) {
    // frames the hops read: hop h takes frame h - 1 (h >= 1) and frame h (h < n_frames)
    const uint64_t first = hop_begin ? hop_begin - 1 : 0;
    const uint64_t last = std::min(hop_end, n_frames);  // one past the last frame read
    // d_blocks holds frames [blk_frame0, blk_frame0 + n_block_frames); -1 is the decode rounds' ring (slot 0 = carried frame)
    const int64_t held_end = blk_frame0 + static_cast<int64_t>(n_block_frames);
    if (blk_frame0 < -1 || n_block_frames > 0xFFFFFFFFull ||
        (first < last && (static_cast<int64_t>(first) < blk_frame0 || static_cast<int64_t>(last) > held_end)))
      return fail(ctx, GLC_EINVAL, "glc_debug_overlap_add_device: the hops read frames outside d_blocks");
  }
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, glc::launch_overlap_add(d_blocks, blk_frame0, n_frames, channels, hop_begin, hop_end, d_out, ctx->stream));
  return GLC_OK;
}

int glc_debug_compact_batch_device(glc_ctx *ctx, const void *d_records, const uint64_t *clip_frames, uint64_t n_clips,
                                   uint16_t channels, void *d_blob, uint64_t cap, glc_compact_info *info) {
  if (!ctx || !d_records || !clip_frames || !d_blob || !info)
    return fail(ctx, GLC_EINVAL, "glc_debug_compact_batch_device: null argument");
  if (channels == 0 || n_clips == 0) return fail(ctx, GLC_EINVAL, "glc_debug_compact_batch_device: no channels or no clips");
  for (uint64_t i = 0; i < n_clips; ++i)
    if (clip_frames[i] == 0 || clip_frames[i] > 0xFFFFFFFFull)
      return fail(ctx, GLC_EINVAL, "glc_debug_compact_batch_device: a clip of no frames, or of too many");
  if (n_clips > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, "glc_debug_compact_batch_device: too many clips");
  if (!all_aligned(8, d_records, d_blob))
    return fail(ctx, GLC_EINVAL, "glc_debug_compact_batch_device: d_records and d_blob must be 8-byte aligned");
  const BatchBlobLayout l = batch_blob_layout(channels, clip_frames, n_clips);
  if (cap < l.at.bound) return fail(ctx, GLC_EINVAL, "glc_debug_compact_batch_device: blob buffer too small");
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // earlier work may still read the pinned frame map
  const int rc = compact_batch_launch(ctx, d_records, clip_frames, n_clips, channels, l, static_cast<uint8_t *>(d_blob), ctx->stream);
  if (rc != GLC_OK) return rc;
  glc::CompactHeader h;
  GLC_HIP(ctx, hipMemcpyAsync(&h, d_blob, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  info->n_frames = h.n_frames;
  info->n_pairs = h.n_pairs;
  info->n_raw_rows = h.n_raw_rows;
  info->bytes = h.bytes;
  return GLC_OK;
}

extern "C++" {
namespace {
// The two R2 hooks: the window [first_frame, first_frame + frames) of one blob through R2 alone, its tables and status
// to the host.  `whole`: the window is the blob, and the launch compares the sums with the header's totals.
int debug_rows_from_compact(glc_ctx *ctx, const std::string &w, bool whole, const void *d_blob, uint64_t blob_bytes, uint64_t n_frames,
                            uint16_t channels, uint64_t first_frame, uint64_t frames, uint64_t *row_begin, uint32_t *row_cnt,
                            float *row_scale, int64_t *row_raw, uint64_t *row_raw_len, glc_compact_status *status) {
  if (!ctx) return GLC_EINVAL;
  if (channels == 0 || n_frames == 0 || n_frames * channels > 0xFFFFFFFFull) return fail(ctx, GLC_EINVAL, w + ": bad shape");
  if (frames == 0 || first_frame > n_frames || frames > n_frames - first_frame) return fail(ctx, GLC_EINVAL, w + ": the window leaves the blob");
  if (const char *bad = cd_blob_fault(d_blob, blob_bytes, channels, n_frames)) return fail(ctx, GLC_EINVAL, w + ": " + bad);
  DeviceGuard guard(ctx->device);
  const uint32_t M = static_cast<uint32_t>(frames * channels), front = static_cast<uint32_t>(first_frame * channels);
  rt_forget_streams(ctx);
  ctx->cd_status_n = 0;
  int rc = rt_reserve(ctx, ctx->rt_rows, glc::rows_from_compact_bytes(M));
  if (rc == GLC_OK) rc = rt_reserve(ctx, ctx->cd_status, sizeof(glc::CompactStatus));
  if (rc != GLC_OK) return rc;
  const glc::CompactBlob one{reinterpret_cast<uintptr_t>(d_blob), blob_bytes, 0u, static_cast<uint32_t>(n_frames * channels), {front, M}};
  glc::DecodeRows rows{};
  GLC_HIP(ctx, glc::launch_rows_from_compact(nullptr, one, 1, M, channels, glc::R2Mode{whole, front, nullptr}, d_blob, ctx->rt_rows.p,
                                             static_cast<glc::CompactStatus *>(ctx->cd_status.p), ctx->stream, &rows));
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (row_begin) GLC_HIP(ctx, hipMemcpy(row_begin, rows.row_begin, M * 8ull, hipMemcpyDeviceToHost));
  if (row_cnt) GLC_HIP(ctx, hipMemcpy(row_cnt, rows.row_cnt, M * 4ull, hipMemcpyDeviceToHost));
  if (row_scale) GLC_HIP(ctx, hipMemcpy(row_scale, rows.row_scale, M * 4ull, hipMemcpyDeviceToHost));
  if (row_raw) GLC_HIP(ctx, hipMemcpy(row_raw, rows.row_raw, M * 8ull, hipMemcpyDeviceToHost));
  if (row_raw_len) GLC_HIP(ctx, hipMemcpy(row_raw_len, rows.row_raw_len, M * 8ull, hipMemcpyDeviceToHost));
  ctx->cd_status_n = 1;
  return status ? glc_decode_compact_last_status(ctx, status, 1) : GLC_OK;
}
}  // namespace
}  // extern "C++"

int glc_debug_rows_from_compact(glc_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint64_t n_frames, uint16_t channels,
                                uint64_t *row_begin, uint32_t *row_cnt, float *row_scale, int64_t *row_raw,
                                uint64_t *row_raw_len, glc_compact_status *status) {
  return debug_rows_from_compact(ctx, "glc_debug_rows_from_compact", true, d_blob, blob_bytes, n_frames, channels, 0, n_frames, row_begin,
                                 row_cnt, row_scale, row_raw, row_raw_len, status);
}

int glc_debug_rows_from_compact_window(glc_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint64_t n_frames, uint16_t channels,
                                       uint64_t first_frame, uint64_t frames, uint64_t *row_begin, uint32_t *row_cnt,
                                       float *row_scale, int64_t *row_raw, uint64_t *row_raw_len, glc_compact_status *status) {
  return debug_rows_from_compact(ctx, "glc_debug_rows_from_compact_window", false, d_blob, blob_bytes, n_frames, channels, first_frame,
                                 frames, row_begin, row_cnt, row_scale, row_raw, row_raw_len, status);
}

int glc_debug_set_imdct_variant(glc_ctx *ctx, int variant) {
  if (!ctx || variant < 0 || variant > 6) return fail(ctx, GLC_EINVAL, "glc_debug_set_imdct_variant: variant must be 0..6");
  if (variant != ctx->d1_variant) ctx->plan_uid = 0;  // variants 5 / 6 deal the units differently: the kept order is not theirs
  ctx->d1_variant = variant;
  return GLC_OK;
}

int glc_debug_set_mdct_variant(glc_ctx *ctx, int variant) {
  if (!ctx || variant < 0 || variant > 4) return fail(ctx, GLC_EINVAL, "glc_debug_set_mdct_variant: variant must be 0..4");
  ctx->policy.k1_variant = variant;
  return GLC_OK;
}

int glc_debug_live_resources(uint64_t counts[4]) {
  if (!counts) return GLC_EINVAL;
  for (int k = 0; k < glc::kLiveKinds; ++k) counts[k] = glc::g_live[k].load(std::memory_order_relaxed);
  return GLC_OK;
}

int glc_debug_set_encode_screen(glc_ctx *ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return fail(ctx, GLC_EINVAL, "glc_debug_set_encode_screen: mode must be 0..2");
  ctx->policy.set_mode(mode);
  return GLC_OK;
}

int glc_debug_set_encode_repair(glc_ctx *ctx, int kind) {
  if (!ctx || kind < 0 || kind > 2) return fail(ctx, GLC_EINVAL, "glc_debug_set_encode_repair: kind must be 0..2");
  ctx->policy.repair_kind = kind;
  return GLC_OK;
}

int glc_debug_set_encode_edge(glc_ctx *ctx, int kind) {
  if (!ctx || kind < 0 || kind > 3) return fail(ctx, GLC_EINVAL, "glc_debug_set_encode_edge: kind must be 0..3");
  ctx->policy.edge_kind = kind;
  return GLC_OK;
}

int glc_debug_encode_edge_stats(glc_ctx *ctx, uint64_t *launches, uint64_t *rows) {
  if (!ctx || !launches || !rows) return fail(ctx, GLC_EINVAL, "glc_debug_encode_edge_stats: null argument");
  *launches = ctx->policy.edge_launches;
  *rows = ctx->policy.edge_rows;
  return GLC_OK;
}

int glc_debug_set_encode_bound(glc_ctx *ctx, int kind) {
  if (!ctx || kind < 0 || kind > 2) return fail(ctx, GLC_EINVAL, "glc_debug_set_encode_bound: kind must be 0..2");
  ctx->policy.bound_kind = kind;
  return GLC_OK;
}

int glc_debug_encode_matrix_bound(uint32_t *ne, uint32_t *pieces, uint32_t *products, uint32_t *k_block, uint32_t *seg_blocks,
                                  uint32_t *planes, double *kappa, double *split_eps, double *budget) {
  if (!ne || !pieces || !products || !k_block || !seg_blocks || !planes || !kappa || !split_eps || !budget) return GLC_EINVAL;
  using MB = glc::MatrixBound;
  *ne = MB::kNe, *pieces = MB::kPieces, *products = MB::kProducts, *k_block = MB::kKBlock, *seg_blocks = MB::kSegBlocks;
  *planes = MB::kGroups, *kappa = MB::kKappa, *split_eps = MB::kSplitEps, *budget = MB::kBudget;
  return GLC_OK;
}

int glc_debug_encode_bound_tap(glc_ctx *ctx, uint32_t rows, float *h, float *a) {
  if (!ctx || !h || !a || rows == 0 || rows != ctx->policy.tap_rows || !ctx->slot[0].screen_ws.p)
    return fail(ctx, GLC_EINVAL, "glc_debug_encode_bound_tap: no screened launch of that many rows on this context");
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t stride = (static_cast<uint64_t>(rows) + 255ull) / 256ull * 256ull;
  const uint32_t tap_planes = ctx->policy.tap_planes;
  std::vector<float> planes((tap_planes + 1ull) * stride);
  GLC_HIP(ctx, hipMemcpy(planes.data(), ctx->slot[0].screen_ws.p, planes.size() * 4, hipMemcpyDeviceToHost));
  for (uint32_t m = 0; m < rows; ++m) {
    float mx = 0.0f;
    for (uint32_t p = 0; p < tap_planes; ++p) mx = std::fmax(mx, planes[p * stride + m]);
    h[m] = mx;
    a[m] = planes[tap_planes * stride + m];
  }
  return GLC_OK;
}

int glc_debug_mfma_bf16(glc_ctx *ctx, const uint16_t *a, const uint16_t *b, const float *c, float *d) {
  if (!ctx || !a || !b || !c || !d) return fail(ctx, GLC_EINVAL, "glc_debug_mfma_bf16: null argument");
  DeviceGuard guard(ctx->device);
  DevBuf buf;
  GLC_HIP(ctx, buf.reserve(2 * 1024 + 2 * 4096));
  uint8_t *p = static_cast<uint8_t *>(buf.p);
  hipError_t e = hipMemcpy(p, a, 1024, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p + 1024, b, 1024, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p + 2048, c, 4096, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = glc::launch_debug_mfma_bf16(reinterpret_cast<const uint16_t *>(p), reinterpret_cast<const uint16_t *>(p + 1024),
                                    reinterpret_cast<const float *>(p + 2048), reinterpret_cast<float *>(p + 2048 + 4096), ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(d, p + 2048 + 4096, 4096, hipMemcpyDeviceToHost);
  GLC_HIP(ctx, e);
  return GLC_OK;
}

int glc_debug_encode_repair_stats(glc_ctx *ctx, uint64_t *launches_tiles, uint64_t *launches_latency) {
  if (!ctx || !launches_tiles || !launches_latency) return fail(ctx, GLC_EINVAL, "glc_debug_encode_repair_stats: null argument");
  *launches_tiles = ctx->policy.repair_launches[0];
  *launches_latency = ctx->policy.repair_launches[1];
  return GLC_OK;
}

int glc_debug_encode_screen_stats(glc_ctx *ctx, uint64_t *rows_screened, uint64_t *rows_repaired) {
  if (!ctx || !rows_screened || !rows_repaired) return fail(ctx, GLC_EINVAL, "glc_debug_encode_screen_stats: null argument");
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->stream_b) GLC_HIP(ctx, hipStreamSynchronize(ctx->stream_b));
  *rows_screened = ctx->policy.rows_screened;
  *rows_repaired = 0;
  if (ctx->screen_stat.p) {
    const volatile uint64_t *hs = static_cast<const volatile uint64_t *>(ctx->screen_stat.p);
    *rows_repaired = hs[2] + hs[4 + 2];  // per slot: the rows the serial repair took
  }
  if (ctx->edge_failed.p) {  // ... and the edge rows that failed, which the side stream took
    uint64_t e[2] = {0, 0};  // (the streams that write it have been waited for above)
    GLC_HIP(ctx, hipMemcpyAsync(e, ctx->edge_failed.p, sizeof e, hipMemcpyDeviceToHost, ctx->stream));
    GLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *rows_repaired += e[0] + e[1];
  }
  return GLC_OK;
}

int glc_debug_encode_screen_layout(uint32_t ne, uint32_t rows, uint32_t *hybrid_pairs, uint32_t *planes,
                                   uint64_t *workspace_bytes) {
  if (!hybrid_pairs || !planes || !workspace_bytes) return GLC_EINVAL;
  const uint32_t edge = 64u * ne;  // a last band that starts at column 64 ne
  glc::ScreenShape sh{};
  if (ne > 16 || !glc::encode_screen_shape(&edge, 1, &sh)) return GLC_EINVAL;
  *hybrid_pairs = sh.hp;
  *planes = sh.n_planes;
  *workspace_bytes = glc::encode_screen_bytes(rows, sh);
  return GLC_OK;
}

int glc_debug_clock_probe_begin(glc_ctx *ctx, uint32_t window_us) {
  if (!ctx || window_us == 0) return fail(ctx, GLC_EINVAL, "glc_debug_clock_probe_begin: bad argument");
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, ctx->probe_stream.ensure());
  GLC_HIP(ctx, ctx->probe_out.reserve(64));  // pinned: the wave writes its two counters straight to the host
  std::memset(ctx->probe_out.p, 0, 16);
  GLC_HIP(ctx, glc::launch_clock_probe(static_cast<uint64_t>(window_us) * 100ull, static_cast<uint64_t *>(ctx->probe_out.p),
                                       ctx->probe_stream));
  return GLC_OK;
}

int glc_debug_clock_probe_end(glc_ctx *ctx, float *ghz) {
  if (!ctx || !ghz || !ctx->probe_stream) return fail(ctx, GLC_EINVAL, "glc_debug_clock_probe_end: no probe running");
  DeviceGuard guard(ctx->device);
  GLC_HIP(ctx, hipStreamSynchronize(ctx->probe_stream));
  const uint64_t *o = static_cast<const uint64_t *>(ctx->probe_out.p);
  if (o[1] == 0) return fail(ctx, GLC_EHIP, "glc_debug_clock_probe_end: the probe reported nothing");
  *ghz = static_cast<float>(static_cast<double>(o[0]) / static_cast<double>(o[1]) * 0.1);
  return GLC_OK;
}

int glc_decode_stream_begin(glc_ctx *ctx, const glc_frames *in) {
  if (!ctx || !in) return fail(ctx, GLC_EINVAL, "glc_decode_stream_begin: null argument");
  ctx->stream_open = false;
  int rc = decode_prepare(ctx, in);
  if (rc != GLC_OK) return rc;
  {
    DeviceGuard guard(ctx->device);
    const size_t chunk = static_cast<size_t>(GLC_FRAMES_PER_CHUNK) + 1;
    GLC_HIP(ctx, ctx->blocks.reserve(chunk * in->channels * glc::kFrame * sizeof(float)));
    GLC_HIP(ctx, ctx->stream_out.reserve(2 * chunk * glc::kHop * in->channels * sizeof(float)));
  }
  rc = ensure_copy_objects(ctx);
  if (rc != GLC_OK) return rc;
  ctx->stream_buf = 0;
  ctx->stream_elem = 0;
  // the first chunk is on its way before the caller asks for it
  rc = round_launch(ctx, GLC_FRAMES_PER_CHUNK, true, static_cast<float *>(ctx->stream_out.p), ctx->ev_dec[0],
                    &ctx->stream_frames, &ctx->stream_last);
  if (rc != GLC_OK) return rc;
  ctx->stream_open = true;
  return GLC_OK;
}

int glc_decode_stream_next(glc_ctx *ctx, float *chunk, uint64_t cap, uint64_t *n_out, int *is_last) {
  return decode_stream_next(ctx, chunk, cap, n_out, is_last);
}

int glc_decode_stream_next_i16(glc_ctx *ctx, int16_t *chunk, uint64_t cap, uint64_t *n_out, int *is_last) {
  return decode_stream_next(ctx, chunk, cap, n_out, is_last);
}

}  // extern "C"
