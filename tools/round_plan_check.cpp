// round_plan_check.cpp - the round rule and the table offsets of the batch, store and stream drivers, and the rounds of
// one stream through the host encode, round trip and decode (csrc/glc_rounds.hpp, with the upload mark and the output
// span of a round from csrc/glc_common.h) on the host alone.  The greedy rule makes the rounds of a list unique, so the properties below
// pin pack_rounds without a second copy of its loop; tests/test_round_boundaries.py pins on the device that every
// driver sizes and addresses what it returns.  Plain C++, no HIP header: built by tests/test_round_plan.py with
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Werror tools/round_plan_check.cpp
// Exit status 0 and the line "round plan ok": every check held.
#include <algorithm>
#include <cstdio>
#include <initializer_list>

#include "../gapless-lossy-codec_amd/csrc/glc_common.h"
#include "../gapless-lossy-codec_amd/csrc/glc_rounds.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      if (++g_failed <= 20) std::printf("line %d (%s): %s does not hold\n", __LINE__, g_what, #cond);      \
    }                                                                                                     \
  } while (0)
static char g_what[96] = "";

using Frames = std::vector<uint64_t>;

static std::vector<RoundSpan> pack(const Frames &f, uint64_t budget, uint64_t front) {
  return pack_rounds(f.size(), [&](uint64_t i) { return f[i]; }, budget, front);
}

// Every property the drivers rely on, of the rounds of one list.
static void check_rounds(const Frames &f, uint64_t budget, uint64_t front) {
  const std::vector<RoundSpan> rounds = pack(f, budget, front);
  uint64_t next = 0;  // every item in exactly one round: the rounds are contiguous, in item order, and end at n
  for (size_t j = 0; j < rounds.size(); ++j) {
    const RoundSpan &r = rounds[j];
    CHECK(r.first == next);
    CHECK(r.n >= 1);
    CHECK(r.first + r.n <= f.size());
    if (r.n < 1 || r.first + r.n > f.size()) return;
    next = r.first + r.n;
    uint64_t real = 0, slots = 0;
    for (uint64_t i = r.first; i < next; ++i) real += f[i], slots += f[i] + 1;
    CHECK(r.n_real == real);
    const bool alone_too_long = r.n == 1 && front + f[r.first] + 1 > budget;
    CHECK(r.lng == alone_too_long);
    if (r.lng) {
      CHECK(r.V == slots);
    } else {
      CHECK(r.V == front + slots);
      CHECK(front + slots <= budget);
      // greedy: the round before, where it is a packed one, had no room for this round's first item
      if (j > 0 && !rounds[j - 1].lng) CHECK(rounds[j - 1].V + f[r.first] + 1 > budget);
    }
  }
  CHECK(next == f.size());
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;  // fixed seed: the same lists in every run
static uint64_t rnd(uint64_t below) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return below ? (g_rng >> 33) % below : 0;
}

static size_t count_lng(const std::vector<RoundSpan> &rounds) {
  size_t n = 0;
  for (const RoundSpan &r : rounds) n += r.lng ? 1 : 0;
  return n;
}

// The rounds of a host encode: what encode_pipeline relies on, and the shape DESIGN.md section 4 states.
static void check_encode_rounds(uint64_t n_frames, uint32_t ch, uint64_t chunk) {
  const uint64_t piece = 2048 / ch;  // ch <= 2048 here
  const std::vector<StreamRound> rounds = encode_stream_rounds(n_frames, ch, chunk);
  uint64_t next = 0;
  for (size_t j = 0; j < rounds.size(); ++j) {
    const StreamRound &r = rounds[j];
    const bool is_last = j + 1 == rounds.size();
    CHECK(r.f0 == next && r.nf >= 1);  // they tile [0, n_frames) in order, none empty
    next = r.f0 + r.nf;
    if (!is_last) {
      CHECK(r.nf == (j < 4 ? piece : chunk));  // four opening rounds while the stream lasts, then whole chunks
      CHECK(r.nf <= chunk);
    } else {
      CHECK(r.nf < (j < 4 ? piece : chunk) + piece / 2);  // what it took over is less than half a piece
      CHECK(r.nf >= piece / 2 || rounds.size() == 1);
    }
  }
  CHECK(next == n_frames && !rounds.empty());
}

// The upload marks of the rounds `rounds` of a stream of n_samples: what the uploader stage sends, and when.
static void check_upload_marks(const std::vector<StreamRound> &rounds, const glc_plan &plan, uint32_t ch, uint64_t n_samples) {
  uint64_t before = 0;
  for (size_t j = 0; j < rounds.size(); ++j) {
    const StreamRound &r = rounds[j];
    const uint64_t mark = glc::upload_mark(r.f0, r.nf, plan.per_channel, ch, n_samples);
    CHECK(mark >= before && mark <= n_samples);
    // the round's last frame reads per-channel samples up to 1024 f - 512 + 2048, its halo: every sample of the stream
    // in front of that is up, and so is the window frame_sample_window states
    const uint64_t reads_to = (r.f0 + r.nf - 1) * 1024 + 1536;
    CHECK(mark >= std::min<uint64_t>(n_samples, std::min<uint64_t>(reads_to, plan.per_channel) * ch));
    CHECK(mark >= std::min<uint64_t>(n_samples, glc::frame_sample_window(r.f0, r.f0 + r.nf, plan.per_channel).hi * ch));
    if (j + 1 == rounds.size()) CHECK(mark == n_samples);
    before = mark;
  }
}

// The output spans of the decode rounds of `round` frames of a stream, the bare tail hop with the last of them or,
// `tail_alone`, in a last round of no frames: they tile what the trim keeps, each inside its round's hops.
static void check_output_spans(uint64_t n_frames, uint64_t per_hop, const glc::Trim &trim, uint64_t round, bool tail_alone) {
  uint64_t at = trim.start;
  const uint64_t n_rounds = fixed_round_count(n_frames, round);
  for (uint64_t i = 0; i < n_rounds + (tail_alone ? 1 : 0); ++i) {
    const StreamRound r = i < n_rounds ? fixed_round(n_frames, round, i) : StreamRound{n_frames, 0};
    if (i < n_rounds) CHECK(r.f0 == i * round && r.nf >= 1 && r.nf <= round && (r.nf == round || r.f0 + r.nf == n_frames));
    const bool last = tail_alone ? i == n_rounds : i + 1 == n_rounds;
    const glc::OutSpan s = glc::decode_round_span(trim, per_hop, r.f0, r.nf, last);
    CHECK(s.lo == at && s.hi >= s.lo);
    if (s.hi > s.lo) CHECK(s.lo >= r.f0 * per_hop && s.hi <= (r.f0 + r.nf + (last ? 1 : 0)) * per_hop);
    at = s.hi;
  }
  CHECK(at == trim.start + trim.n);
}

int main() {
  // ---- one stream through the host encode, the round trip and the decode
  for (uint32_t ch : {1u, 2u, 3u, 6u, 8u}) {
    const uint64_t chunk = ch == 1 ? 8192 : 4096;
    std::snprintf(g_what, sizeof g_what, "encode_stream_rounds, %u channels", ch);
    for (uint64_t n = 1; n <= 4 * (2048 / ch) + 3 * chunk + 2048; ++n) check_encode_rounds(n, ch, chunk);
    CHECK(encode_stream_rounds(0, ch, chunk).empty());
    const uint64_t per_hop = 1024ull * ch;
    for (uint64_t T : {513ull, 1024ull, 1536ull, 1537ull, 5000ull, 2048ull * 1024, 4096ull * 1024 - 100, 4097ull * 1024 - 100,
                       3 * 4096ull * 1024 + 77, 20000ull * 1024 + 511})
      for (uint64_t ragged = 0; ragged < (ch > 1 ? 2u : 1u); ++ragged) {
        const uint64_t n_samples = T * ch - ragged;
        const glc_plan plan = glc::plan_encode(n_samples, static_cast<uint16_t>(ch));
        if (plan.n_frames == 0) continue;  // a ragged stream the encoder refuses
        std::snprintf(g_what, sizeof g_what, "marks and spans, %u channels, %llu samples", ch, (unsigned long long)n_samples);
        check_upload_marks(encode_stream_rounds(plan.n_frames, ch, chunk), plan, ch, n_samples);
        for (uint64_t round : {uint64_t(1), uint64_t(3), uint64_t(4096), plan.n_frames}) {
          if (plan.n_frames / round > 5000) continue;
          std::vector<StreamRound> fixed;
          for (uint64_t i = 0; i < fixed_round_count(plan.n_frames, round); ++i) fixed.push_back(fixed_round(plan.n_frames, round, i));
          check_upload_marks(fixed, plan, ch, n_samples);
          // the stream's own trim cuts the first hop (the delay) and the last; then trims that keep nothing, a single
          // sample, everything, and a stretch that begins and ends inside hops further in
          const uint64_t all = (plan.n_frames + 1) * per_hop;
          for (const glc::Trim &trim : {glc::gapless_trim(plan.n_frames, ch, plan.encoder_delay, n_samples), glc::Trim{0, all},
                                        glc::Trim{512, 0}, glc::Trim{all - 1, 1}, glc::Trim{all / 2 + 7, all / 4},
                                        glc::Trim{std::min(all, 3 * per_hop + 5), all - std::min(all, 3 * per_hop + 5)}})
            for (bool tail_alone : {false, true}) check_output_spans(plan.n_frames, per_hop, trim, round, tail_alone);
        }
      }
  }

  const struct {
    uint64_t budget, front;
  } cases[] = {{4096, 0}, {8192, 0}, {4097, 0}, {4096, 1}, {5, 0}, {5, 1}, {2, 0}};
  for (const auto &c : cases) {
    const uint64_t B = c.budget, F = c.front;
    std::snprintf(g_what, sizeof g_what, "budget %llu, front %llu", (unsigned long long)B, (unsigned long long)F);
    const uint64_t fits = B - F - 1;  // the most frames of an item that is not a round of its own
    // hand-written lists
    CHECK(pack({}, B, F).empty());
    {
      const auto r = pack({fits}, B, F);
      CHECK(r.size() == 1 && !r[0].lng && r[0].V == B && r[0].n_real == fits);
      check_rounds({fits}, B, F);
    }
    {
      const auto r = pack({fits + 1}, B, F);
      CHECK(r.size() == 1 && r[0].lng && r[0].n == 1 && r[0].V == fits + 2 && r[0].n_real == fits + 1);
      check_rounds({fits + 1}, B, F);
    }
    // a long item first, last, and between two small ones, which are not merged across it
    for (const Frames &f : {Frames{B, 0, 0}, Frames{0, 0, B}, Frames{0, B + 7, 0}}) {
      const auto r = pack(f, B, F);
      check_rounds(f, B, F);
      CHECK(count_lng(r) == 1);
      const bool two_small_fit = F + 2 <= B;  // two items of no frames in one round
      const bool between = f[1] != 0;
      CHECK(r.size() == (between || !two_small_fit ? 3u : 2u));
    }
    // items that fill a round to exactly the budget, then one more frame
    if (fits >= 1) {
      Frames f;  // `fits + 1` slots behind the front: items of 1 frame (2 slots) and, where that is odd, one of none
      for (uint64_t s = fits + 1; s >= 2 && f.size() < 4096; s -= 2) f.push_back(1);
      if ((fits + 1) % 2) f.push_back(0);
      uint64_t slots = 0;
      for (uint64_t v : f) slots += v + 1;
      if (F + slots == B) {  // (the largest budgets are filled with longer items below)
        CHECK(pack(f, B, F).size() == 1);
        check_rounds(f, B, F);
        f.back() += 1;  // (a lone item grown past the budget is one long round)
        CHECK(pack(f, B, F).size() == (f.size() == 1 ? 1u : 2u));
        check_rounds(f, B, F);
      }
    }
    if (B >= 4096) {  // 64 items of 63 frames fill 4096 slots; the other budgets get their remainder as a last item
      Frames f(64, 63);
      f.back() = 63 + B - F - 4096;
      CHECK(pack(f, B, F).size() == 1 && pack(f, B, F)[0].V == B);
      check_rounds(f, B, F);
      f.back() += 1;
      CHECK(pack(f, B, F).size() == 2 && pack(f, B, F)[1].n == 1);
      check_rounds(f, B, F);
    }
    // items of no frames: refused by the drivers, but the packer must neither divide nor wrap on them
    check_rounds(Frames(1000, 0), B, F);
    CHECK(pack(Frames(1000, 0), B, F).size() == (1000 + (B - F) - 1) / (B - F));
    // pseudo-random lists: short items, items about a round long, items far beyond one
    for (int t = 0; t < 3000; ++t) {
      Frames f(rnd(48));
      const uint64_t kind = rnd(4);
      for (uint64_t &v : f) {
        const uint64_t k = kind == 3 ? rnd(3) : kind;
        v = k == 0 ? rnd(B / 8 + 2) : k == 1 ? rnd(B + 2) : fits - (fits ? rnd(2) : 0) + rnd(3) * rnd(B);
      }
      check_rounds(f, B, F);
    }
  }

  // TableOffsets: tables on multiples of 256 that do not overlap; an empty table takes nothing
  std::snprintf(g_what, sizeof g_what, "TableOffsets");
  for (int t = 0; t < 2000; ++t) {
    TableOffsets offs;
    CHECK(offs.size() == 0 && offs.take(0) == 0 && offs.size() == 0);
    size_t end = 0;  // of the last table
    for (uint64_t k = rnd(12); k > 0; --k) {
      const size_t bytes = rnd(4) ? rnd(5000) : 256 * rnd(4), at = offs.take(bytes);
      CHECK(at % 256 == 0 && at >= end && at < end + 256);
      end = at + bytes;
      CHECK(offs.size() % 256 == 0 && offs.size() >= end && offs.size() < end + 256);
      const size_t here = offs.size();
      CHECK(offs.take(0) == here && offs.size() == here);
    }
  }
  if (g_failed) {
    std::printf("round plan: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("round plan ok\n");
  return 0;
}
