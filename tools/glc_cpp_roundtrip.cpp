// glc_cpp_roundtrip.cpp — exercises include/glc.hpp (the C++ mirror of the reference's Encoder /
// Decoder API) the way tests/integration_tests.rs drives the Rust API: encode interleaved f32 PCM,
// save, load, decode both ways, and leave the artefacts on disk for the caller to compare.
//   glc_cpp_roundtrip <in.f32> <sample_rate> <channels> <out.glc> <out.f32>
//   ... <chunk_sample_frames> <stream_out.glc> [<stream_out.f32>]   the stream encoder (and decoder) instead
// Build: g++ -O2 -std=c++17 -Iinclude tools/glc_cpp_roundtrip.cpp -Lgapless-lossy-codec_amd -lglc_hip
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "glc.hpp"

int main(int argc, char **argv) {
  if (argc != 6 && argc != 8 && argc != 9) {
    std::fprintf(stderr, "usage: %s in.f32 sample_rate channels out.glc out.f32 [chunk_sample_frames stream_out.glc [stream_out.f32]]\n", argv[0]);
    return 2;
  }
  try {
    if (argc >= 8) {
      // the streaming encoder through the C++ mirror: the file in chunks of argv[6] sample frames, the finish as an
      // empty push; the segments' frame ranges tile the stream; the bytes go to argv[7] for the caller to compare
      std::ifstream in(argv[1], std::ios::binary);
      std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
      std::vector<float> pcm(raw.size() / sizeof(float));
      std::memcpy(pcm.data(), raw.data(), pcm.size() * sizeof(float));
      const uint32_t sr = static_cast<uint32_t>(std::atoi(argv[2]));
      const uint16_t ch = static_cast<uint16_t>(std::atoi(argv[3]));
      const uint64_t chunk = static_cast<uint64_t>(std::atoll(argv[6])) * ch;
      if (chunk == 0) return std::fprintf(stderr, "chunk_sample_frames must be positive\n"), 2;
      glc::StreamEncoder se(sr, ch, 2);  // lane 1 is the one in use, lane 0 stays idle
      uint64_t received = 0;
      for (uint64_t at = 0; at < pcm.size(); at += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, pcm.size() - at);
        const glc_stream_push_plan plan = glc::plan_stream_push(received, n / ch);
        const size_t before = se.segments(1).size();
        se.push(1, pcm.data() + at, n);
        if (se.segments(1).size() != before + (plan.n_frames ? 1 : 0)) return std::fprintf(stderr, "segments do not follow the plan\n"), 1;
        received += n / ch;
      }
      se.push(1, static_cast<const float *>(nullptr), 0, true);
      uint64_t next = 0;
      for (const glc::StreamEncoder::Segment &g : se.segments(1)) {
        if (g.first_frame != next) return std::fprintf(stderr, "segments do not tile the stream\n"), 1;
        next += g.n_frames;
      }
      if (!se.segments(0).empty()) return std::fprintf(stderr, "the idle lane has segments\n"), 1;
      if (argc == 9) {
        // the streaming decoder through the C++ mirror: the segments one push each as they were emitted, the finish with
        // the last one; every push emits what glc::plan_stream_dec_push says; the samples go to argv[8]
        glc::StreamDecoder sd(sr, ch, 2);  // lane 1 again
        const std::vector<glc::StreamEncoder::Segment> segs = se.segments(1);
        std::vector<float> played;
        for (size_t k = 0; k < segs.size(); ++k) {
          const bool last = k + 1 == segs.size();
          const glc_stream_dec_plan plan = glc::plan_stream_dec_push(sd.frames_done(1), segs[k].n_frames, last, received);
          const std::vector<float> got =
              sd.push(1, {glc::StreamDecoder::Segment{segs[k].first_frame, segs[k].n_frames, segs[k].blob, segs[k].bytes}}, last, received);
          if (got.size() != plan.n_samples * ch || plan.first_sample * ch != played.size())
            return std::fprintf(stderr, "a push does not emit what the plan says\n"), 1;
          played.insert(played.end(), got.begin(), got.end());
        }
        if (sd.frames_done(1) != 0 || sd.frames_done(0) != 0) return std::fprintf(stderr, "a finished lane is not fresh\n"), 1;
        std::ofstream out(argv[8], std::ios::binary);
        out.write(reinterpret_cast<const char *>(played.data()), static_cast<std::streamsize>(played.size() * sizeof(float)));
      }
      const glc::EncodedAudio e = se.encoded(1);
      if (e.n_frames() != next || !se.segments(1).empty()) return std::fprintf(stderr, "encoded(): wrong frame count\n"), 1;
      glc::save_encoded(e, argv[7]);
      return 0;
    }
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<float> pcm(raw.size() / sizeof(float));
    std::memcpy(pcm.data(), raw.data(), pcm.size() * sizeof(float));
    const uint32_t sr = static_cast<uint32_t>(std::atoi(argv[2]));
    const uint16_t ch = static_cast<uint16_t>(std::atoi(argv[3]));

    glc::Encoder encoder(sr);
    glc::EncodedAudio encoded = encoder.encode(pcm, ch);
    glc::save_encoded(encoded, argv[4]);

    glc::EncodedAudio loaded = glc::load_encoded(argv[4]);
    glc::Decoder decoder(ch, sr);
    std::vector<float> whole = decoder.decode(loaded);

    std::vector<float> streamed;
    size_t chunks = 0;
    bool saw_last = false;
    decoder.decode_streaming(loaded, [&](glc::AudioChunk &&c) {
      if (saw_last) throw glc::Error(GLC_EINVAL, "chunk after is_last");
      streamed.insert(streamed.end(), c.samples.begin(), c.samples.end());
      saw_last = c.is_last;
      ++chunks;
    });
    // Decoder::decode is the stream with the first encoder_delay values drained and the rest cut
    // to original_length (src/codec.rs:755-765)
    const glc::GaplessInfo gi = loaded.gapless_info();
    if (!saw_last || streamed.size() < gi.encoder_delay + whole.size() || whole.size() != gi.original_length ||
        std::memcmp(streamed.data() + gi.encoder_delay, whole.data(), whole.size() * sizeof(float)) != 0) {
      std::fprintf(stderr, "streaming decode differs from decode\n");
      return 1;
    }
    // structure walk through the accessors (EncodedFrame view)
    uint64_t nnz = 0, raw_frames = 0;
    for (uint64_t f = 0; f < loaded.n_frames(); ++f) {
      const glc::EncodedFrame fr = loaded.frame(f);
      raw_frames += fr.has_raw_pcm;
      for (const auto &l : fr.sparse_coeffs_per_channel) nnz += l.size();
    }
    // the structured bridge through the C++ mirror: frames() == frame(f) for every f; the nested vectors go
    // back in by pointer (from_frames) and serialise to the same bytes; the hooked encode hands out the same
    // frames in ascending contiguous ranges; a stream id makes the second decode a resident one
    {
      const std::vector<glc::EncodedFrame> all = loaded.frames();
      if (all.size() != loaded.n_frames()) return std::fprintf(stderr, "frames(): wrong count\n"), 1;
      for (uint64_t f = 0; f < loaded.n_frames(); ++f) {
        const glc::EncodedFrame one = loaded.frame(f);
        if (one.sparse_coeffs_per_channel != all[f].sparse_coeffs_per_channel || one.scale_factors != all[f].scale_factors ||
            one.has_raw_pcm != all[f].has_raw_pcm || one.raw_pcm != all[f].raw_pcm)
          return std::fprintf(stderr, "frames() differs from frame(%llu)\n", (unsigned long long)f), 1;
      }
      const glc::EncodedAudio again = glc::EncodedAudio::from_frames(loaded.header(), all, loaded.gapless_info(), 4711);
      if (again.to_bytes() != loaded.to_bytes() || again.stream_id() != 4711) return std::fprintf(stderr, "from_frames: bytes differ\n"), 1;
      std::vector<glc::EncodedFrame> hooked;
      uint64_t next = 0;
      bool ordered = true;
      const glc::EncodedAudio e2 = encoder.encode(pcm.data(), pcm.size(), ch, [&](uint64_t f0, std::vector<glc::EncodedFrame> &&part) {
        ordered = ordered && f0 == next;
        next = f0 + part.size();
        for (auto &fr : part) hooked.push_back(std::move(fr));
      });
      if (!ordered || hooked.size() != all.size() || e2.to_bytes() != loaded.to_bytes())
        return std::fprintf(stderr, "hooked encode: ranges or bytes differ\n"), 1;
      for (size_t f = 0; f < all.size(); ++f)
        if (hooked[f].sparse_coeffs_per_channel != all[f].sparse_coeffs_per_channel || hooked[f].scale_factors != all[f].scale_factors ||
            hooked[f].raw_pcm != all[f].raw_pcm)
          return std::fprintf(stderr, "hooked encode: frame %zu differs\n", f), 1;
      glc::Decoder d2(ch, sr);
      const std::vector<float> first = d2.decode(again);
      if (d2.resident_stream() != 4711) return std::fprintf(stderr, "stream id not resident\n"), 1;
      const std::vector<float> second = d2.decode_resident(4711, first.size());
      if (first != whole || second != whole) return std::fprintf(stderr, "bridge decodes differ\n"), 1;
      try {
        encoder.encode(pcm.data(), pcm.size(), ch, [](uint64_t, std::vector<glc::EncodedFrame> &&) { throw std::runtime_error("stop"); });
        return std::fprintf(stderr, "a throwing hook was swallowed\n"), 1;
      } catch (const std::runtime_error &) {
      }
    }
    // the integer batch calls through the C++ mirror: the decode narrowed to 16 bits and its first half as two
    // clips of one call - the bytes of the single integer encode, and of the same values in 24-bit containers;
    // decode_batch_i16 gives each stream the samples decode_i16 gives it alone
    if (whole.size() / 2 / ch > 512) {
      const std::vector<int16_t> q = decoder.decode_i16(loaded);
      const std::vector<std::vector<int16_t>> clips{q, std::vector<int16_t>(q.begin(), q.begin() + q.size() / 2 / ch * ch)};
      std::vector<std::vector<int32_t>> clips24(clips.size());
      for (size_t i = 0; i < clips.size(); ++i)
        for (int16_t v : clips[i]) clips24[i].push_back(static_cast<int32_t>(v) * 256);
      const std::vector<glc::EncodedAudio> b16 = encoder.encode_batch(clips, ch), b24 = encoder.encode_batch(clips24, 24, ch);
      std::vector<const glc::EncodedAudio *> ptrs;
      for (size_t i = 0; i < clips.size(); ++i) {
        if (b16[i].to_bytes() != encoder.encode(clips[i], ch).to_bytes() || b24[i].to_bytes() != b16[i].to_bytes())
          return std::fprintf(stderr, "integer encode_batch: clip %zu differs from the single encode\n", i), 1;
        ptrs.push_back(&b16[i]);
      }
      std::vector<uint64_t> off;
      const std::vector<int16_t> packed = decoder.decode_batch_i16(ptrs, off);
      for (size_t i = 0; i < ptrs.size(); ++i) {
        const std::vector<int16_t> one = decoder.decode_i16(b16[i]);
        if (off[i + 1] - off[i] != one.size() || std::memcmp(packed.data() + off[i], one.data(), one.size() * 2) != 0)
          return std::fprintf(stderr, "decode_batch_i16: stream %zu differs from decode_i16\n", i), 1;
      }
    }
    // src/audio.rs + src/flac.rs twins through the C++ mirror: export the decoded samples to FLAC and
    // WAV next to the output file and read both back (tests/test_export.rs)
    const std::string flac_path = std::string(argv[5]) + ".flac", wav_path = std::string(argv[5]) + ".wav";
    glc::export_to_flac(flac_path, whole, sr, ch);
    glc::export_to_wav(wav_path, whole, sr, ch);
    const glc::LoadedAudio from_flac = glc::load_audio_file_lossless(flac_path);
    const glc::LoadedAudio from_wav = glc::load_audio_file_lossless(wav_path);
    // FLAC frames whole sample-frames only (a ragged tail is hashed but not framed, src/flac.rs:960)
    const size_t framed = whole.size() / ch * ch;
    if (from_flac.sample_rate != sr || from_flac.channels != ch || from_flac.samples.size() != framed ||
        from_wav.samples.size() < framed ||
        std::memcmp(from_wav.samples.data(), from_flac.samples.data(), framed * sizeof(float)) != 0) {
      std::fprintf(stderr, "FLAC / WAV export does not read back\n");
      return 1;
    }
    try {
      glc::load_audio_file_lossless(std::string(argv[5]) + ".mp3");
      return 1;
    } catch (const glc::Error &e) {
      if (e.code != GLC_EINVAL) return 1;
    }
    std::ofstream out(argv[5], std::ios::binary);
    out.write(reinterpret_cast<const char *>(whole.data()), static_cast<std::streamsize>(whole.size() * sizeof(float)));
    const glc::AudioHeader h = loaded.header();
    const glc::GaplessInfo g = loaded.gapless_info();
    std::printf("{\"sample_rate\": %u, \"channels\": %u, \"total_samples\": %llu, \"encoder_delay\": %u, "
                "\"padding\": %u, \"original_length\": %llu, \"n_frames\": %llu, \"raw_frames\": %llu, "
                "\"nnz\": %llu, \"decoded\": %zu, \"chunks\": %zu}\n",
                h.sample_rate, h.channels, (unsigned long long)h.total_samples, g.encoder_delay, g.padding,
                (unsigned long long)g.original_length, (unsigned long long)loaded.n_frames(),
                (unsigned long long)raw_frames, (unsigned long long)nnz, whole.size(), chunks);
    // error behaviour: the reference panics on channels == 0; here it is an exception
    try {
      encoder.encode(pcm, 0);
      std::fprintf(stderr, "channels == 0 accepted\n");
      return 1;
    } catch (const glc::Error &e) {
      if (e.code != GLC_EINVAL) return 1;
    }
    return 0;
  } catch (const glc::Error &e) {
    std::fprintf(stderr, "glc::Error %d: %s\n", e.code, e.what());
    return 1;
  }
}
