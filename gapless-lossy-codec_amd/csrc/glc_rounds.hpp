// glc_rounds.hpp — how the drivers of glc_api.hip cut a call into rounds (the batch, store and stream drivers their
// items, the host encode, round trip and decode their one stream), and where the tables of a call lie in its image.  Plain C++17 without a HIP type: a host program can include it alone
// (tools/round_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// Items [first, first + n) of a call, sent through one launch chain.  n_real: their frames.  V: the slots of the
// round's virtual stream - `front` + frames + 1 per item - or, of a long round, the item's frames + 1.
struct RoundSpan {
  uint64_t first = 0, n = 0, n_real = 0, V = 0;
  bool lng = false;  // ONE item that is more than a round: its driver sends it down the single-stream path
};

// THE round rule.  Whole items in order, frames_of(i) + 1 slots each - the one more is the junk
// frame that straddles two clips, or the tail hop of a decode - behind `front` slots that every round spends before its
// first item, at most `budget` slots together.  Greedy: an item joins the open round unless that would pass the budget,
// which closes the round first.  An item that does not fit a round of its own closes the open round and is a round to
// itself, flagged `lng`: the items around it are never merged across it.  No round is empty.
template <typename FramesOf>
std::vector<RoundSpan> pack_rounds(uint64_t n, FramesOf frames_of, uint64_t budget, uint64_t front) {
  std::vector<RoundSpan> rounds;
  RoundSpan cur{0, 0, 0, front, false};
  auto close = [&](uint64_t next) {
    if (cur.n) rounds.push_back(cur);
    cur = RoundSpan{next, 0, 0, front, false};
  };
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t frames = frames_of(i), cost = frames + 1;
    if (front + cost > budget) {
      close(i + 1);
      rounds.push_back(RoundSpan{i, 1, frames, cost, true});
      continue;
    }
    if (cur.V + cost > budget) close(i);
    cur.n += 1, cur.n_real += frames, cur.V += cost;
  }
  close(n);
  return rounds;
}

// Frames [f0, f0 + nf) of ONE stream, sent through one launch chain.
struct StreamRound {
  uint64_t f0 = 0, nf = 0;
};

// THE rounds of a host encode (glc_encode*).  The upload nothing hides is the first round's, and
// the kernels nothing hide are the last round's, so a stream opens with four rounds of `piece` frames - 2048 rows,
// 0.15 ms of PCIe each for stereo; at most 2048 rows because that is the size the round kernel of
// launch_mdct_forward (`beside`) is dealt one workgroup per CU for - before it goes on in rounds of `chunk`
// (encode_chunk_frames(ch)).  No round for a remainder of less than half a piece: the round before takes it.
// BASELINE config 2 (4096 stereo frames) is the four opening rounds.
// (Measured and dropped, round 3: cutting the END of a stream in halves - .. 2048, 1024, 512, 512 frames - so that
// the last, unhidden transform is a short one: 1.045 ms against 1.02 at config 2; a round costs the launcher and
// the collector more than the shorter tail returns.)
inline std::vector<StreamRound> encode_stream_rounds(uint64_t n_frames, uint32_t ch, uint64_t chunk) {
  const uint64_t piece = ch < 2048 ? 2048 / ch : 1, opening = 4 * piece;
  std::vector<StreamRound> rounds;
  for (uint64_t f = 0, nf = 0; f < n_frames; f += nf) {
    const uint64_t left = n_frames - f;
    nf = f < opening ? piece : chunk;
    if (nf > left) nf = left;
    if (left - nf < piece / 2) nf = left;
    rounds.push_back(StreamRound{f, nf});
  }
  return rounds;
}

// The fixed rounds of the round trip and the decode: `round` frames each (>= 1), a ragged last one.
inline uint64_t fixed_round_count(uint64_t n_frames, uint64_t round) { return (n_frames + round - 1) / round; }
inline StreamRound fixed_round(uint64_t n_frames, uint64_t round, uint64_t i) {
  const uint64_t f0 = i * round;
  return StreamRound{f0, n_frames - f0 < round ? n_frames - f0 : round};
}

// Where the tables of an image lie: every table starts on a multiple of 256 bytes, in the order it was taken.
struct TableOffsets {
  size_t end = 0;
  size_t take(size_t bytes) {
    const size_t at = end;
    end = (end + bytes + 255) / 256 * 256;
    return at;
  }
  size_t size() const { return end; }  // of the image: the aligned end of the last table
};
