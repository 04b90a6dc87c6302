// glc_cli.cpp — command-line twin of the reference's `glc` binary (src/main.rs) for the paths
// this repository implements: `glc file.wav|file.flac ...` encodes to .glc (encode_file,
// src/main.rs:21-52) and `glc -d file.glc ... [--wav] [--flac-level N]` decodes to FLAC (default)
// or 16-bit WAV (decode_file, :55-113; argument handling :354-583).  It uses only the C ABI of
// libglc_hip.so.  Playback (-p) and the GUI stay with the reference.
// More than one valid file: the files go through glc_encode_batch_int / glc_decode_batch_i16 in groups, with
// one context per sample rate for the whole run (a context costs tens of milliseconds, a short clip a fraction
// of one); what is printed, written and returned is what the per-file loop gives (encode_many / decode_many).
// Build: g++ -O2 -std=c++17 -Iinclude tools/glc_cli.cpp -Lgapless-lossy-codec_amd -lglc_hip \
//        -Wl,-rpath,'$ORIGIN/../gapless-lossy-codec_amd' -o build/glc
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "glc.h"

static std::string with_ext(const std::string &path, const char *ext) {
  const size_t slash = path.find_last_of('/');
  const size_t dot = path.find_last_of('.');
  const std::string stem = (dot != std::string::npos && (slash == std::string::npos || dot > slash)) ? path.substr(0, dot) : path;
  return stem + "." + ext;
}

static std::string lower_ext(const std::string &path) {
  const size_t slash = path.find_last_of('/');
  const size_t dot = path.find_last_of('.');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return "";
  std::string e = path.substr(dot + 1);
  for (char &c : e) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
  return e;
}

static bool exists(const std::string &p) {
  FILE *f = std::fopen(p.c_str(), "rb");
  if (f) std::fclose(f);
  return f != nullptr;
}

static std::string file_name(const std::string &path) {
  const size_t slash = path.find_last_of('/');
  return slash == std::string::npos ? path : path.substr(slash + 1);
}

static long file_size(const std::string &p) {
  FILE *f = std::fopen(p.c_str(), "rb");
  if (!f) return -1;
  std::fseek(f, 0, SEEK_END);
  long n = std::ftell(f);
  std::fclose(f);
  return n;
}

static int encode_file(const std::string &in) {
  std::printf("Loading: \"%s\"\n", file_name(in).c_str());
  void *pcm = nullptr;
  glc_pcm_format fmt = GLC_PCM_F32;
  uint64_t n = 0;
  uint32_t sr = 0, bits = 0;
  uint16_t ch = 0;
  // load_audio_file_lossless, src/audio.rs:19-36 (by lower-cased extension), as the integers the file
  // holds: they are widened to the loader's floats on the device (glc_encode_int)
  const int lrc = glc_audio_load_pcm(in.c_str(), &pcm, &fmt, &bits, &n, &sr, &ch);
  if (lrc != GLC_OK) {
    std::fprintf(stderr, "Error encoding file: %s\n", glc_last_error(nullptr));
    return 1;
  }
  std::printf("Encoding: %u Hz, %u channels, %llu samples\n", sr, ch, static_cast<unsigned long long>(n));
  glc_ctx *ctx = nullptr;
  glc_frames *fr = nullptr;
  int rc = glc_ctx_create(0, sr, &ctx);
  if (rc == GLC_OK) rc = glc_encode_int(ctx, pcm, fmt, bits, n, ch, &fr);
  glc_free(pcm);
  if (rc != GLC_OK) {
    std::fprintf(stderr, "Error encoding file: %s\n", glc_last_error(ctx));
    glc_ctx_destroy(ctx);
    return 1;
  }
  const std::string out = with_ext(in, "glc");
  rc = glc_save(fr, out.c_str());
  glc_frames_free(fr);
  glc_ctx_destroy(ctx);
  if (rc != GLC_OK) {
    std::fprintf(stderr, "Error encoding file: %s\n", glc_last_error(nullptr));
    return 1;
  }
  const long a = file_size(in), b = file_size(out);
  std::printf("Saved: \"%s\" (%ld bytes, %.1f%% of original)\n", file_name(out).c_str(), b, 100.0 * b / a);
  return 0;
}

static int decode_file(const std::string &in, bool wav, unsigned flac_level) {
  std::printf("Loading: \"%s\"\n", file_name(in).c_str());
  glc_frames *fr = nullptr;
  if (glc_load(in.c_str(), &fr) != GLC_OK) {
    std::fprintf(stderr, "Error decoding file: %s\n", glc_last_error(nullptr));
    return 1;
  }
  glc_info info;
  glc_frames_info(fr, &info);
  std::printf("Decoding: %u Hz, %u channels\n", info.sample_rate, info.channels);
  glc_ctx *ctx = nullptr;
  int rc = glc_ctx_create(0, info.sample_rate, &ctx);
  // both outputs are 16-bit (convert_f32_to_i16, src/audio.rs:11-16, src/flac.rs:955-958): narrowed on the device
  std::vector<int16_t> pcm(glc_decoded_len(fr));
  uint64_t n = 0;
  if (rc == GLC_OK) rc = glc_decode_i16(ctx, fr, pcm.data(), pcm.size(), &n);
  glc_frames_free(fr);
  if (rc != GLC_OK) {
    std::fprintf(stderr, "Error decoding file: %s\n", glc_last_error(ctx));
    glc_ctx_destroy(ctx);
    return 1;
  }
  glc_ctx_destroy(ctx);
  std::printf("Decoded %llu samples\n", static_cast<unsigned long long>(n));
  const std::string out = with_ext(in, wav ? "wav" : "flac");
  rc = wav ? glc_wav_save16_i16(out.c_str(), pcm.data(), n, info.sample_rate, info.channels)
           : glc_flac_save_i16(out.c_str(), pcm.data(), n, info.sample_rate, info.channels, static_cast<uint8_t>(flac_level));
  if (rc != GLC_OK) {
    std::fprintf(stderr, "Error decoding file: %s\n", glc_last_error(nullptr));
    return 1;
  }
  if (wav) std::printf("Saved: \"%s\" (WAV)\n", file_name(out).c_str());
  else std::printf("Saved: \"%s\" (FLAC, level %u)\n", file_name(out).c_str(), flac_level);
  return 0;
}

// ---- many files --------------------------------------------------------------------------------------------

// PCM bytes (loaded for an encode / decoded, 2 per sample) that a run over many files holds in host memory
// before it converts and writes what it has: `glc *.wav` over a directory of any size stays within this
// plus one file.
constexpr uint64_t kHeldPcmBudget = 256ull << 20;

static std::string fmt_line(const char *f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt_line(const char *f, ...) {
  char buf[4608];
  va_list ap;
  va_start(ap, f);
  const int n = std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  if (n < 0) return std::string();
  if (static_cast<size_t>(n) < sizeof buf) return std::string(buf, static_cast<size_t>(n));
  std::string big(static_cast<size_t>(n) + 1, '\0');
  va_start(ap, f);
  std::vsnprintf(&big[0], big.size(), f, ap);
  va_end(ap);
  big.resize(static_cast<size_t>(n));
  return big;
}

// One context per sample rate for the whole run; a rate whose context could not be made keeps its message.
struct Contexts {
  struct Entry {
    glc_ctx *ctx = nullptr;
    std::string error;
  };
  std::map<uint32_t, Entry> by_rate;
  Entry &get(uint32_t sr) {
    auto it = by_rate.find(sr);
    if (it != by_rate.end()) return it->second;
    Entry e;
    if (glc_ctx_create(0, sr, &e.ctx) != GLC_OK) e.error = glc_last_error(nullptr), e.ctx = nullptr;
    return by_rate.emplace(sr, e).first->second;
  }
  ~Contexts() {
    for (auto &kv : by_rate) glc_ctx_destroy(kv.second.ctx);
  }
};

// What one argument has to say and to write, kept until every argument in front of it has had its turn: the
// lines of a file appear together and in argument order, as the per-file loop prints them.
struct Item {
  std::string path, out, err;  // stdout / stderr text so far
  bool failed = false, pending = false;  // pending: loaded, waiting for its group's batch call
  // encode
  void *pcm = nullptr;
  glc_pcm_format fmt = GLC_PCM_F32;
  uint32_t sr = 0, bits = 0;
  uint16_t ch = 0;
  uint64_t n = 0;
  // decode
  glc_frames *fr = nullptr;       // decode: the loaded stream; encode: the result
  const int16_t *dec = nullptr;   // the stream's span in its group's buffer
  void fail(const char *what, const char *msg) {
    err += fmt_line("Error %s file: %s\n", what, msg);
    failed = true, pending = false;
  }
};

static void emit(const Item &it) {
  std::fputs(it.out.c_str(), stdout);
  std::fputs(it.err.c_str(), stderr);
}

// `glc f1 f2 ...`, src/main.rs:546-581 around encode_file: keep going, true if any file failed
static bool encode_many(const std::vector<std::string> &args) {
  Contexts contexts;
  std::vector<Item> items(args.size());
  size_t done = 0;  // items [0, done) are finished and printed
  uint64_t held = 0;
  bool failed = false;
  auto flush = [&](size_t end) {  // convert what is loaded, then finish items [done, end) in argument order
    // one batch call per (sample rate, channels, format, bits): what glc_encode_batch_int shares
    std::map<std::tuple<uint32_t, uint16_t, int, uint32_t>, std::vector<size_t>> groups;
    for (size_t i = done; i < end; ++i)
      if (items[i].pending && !items[i].fr) groups[std::make_tuple(items[i].sr, items[i].ch, static_cast<int>(items[i].fmt), items[i].bits)].push_back(i);
    for (auto &g : groups) {
      Item &first = items[g.second[0]];
      Contexts::Entry &c = contexts.get(first.sr);
      bool batched = false;
      if (c.ctx && g.second.size() > 1) {
        std::vector<const void *> pcm;
        std::vector<uint64_t> n;
        for (size_t i : g.second) pcm.push_back(items[i].pcm), n.push_back(items[i].n);
        std::vector<glc_frames *> fr(pcm.size(), nullptr);
        batched = glc_encode_batch_int(c.ctx, pcm.data(), first.fmt, first.bits, n.data(), pcm.size(), first.ch, fr.data()) == GLC_OK;
        for (size_t k = 0; batched && k < fr.size(); ++k) items[g.second[k]].fr = fr[k];
      }
      // alone in its group, or the batch call failed as a whole: every file through the single call, which
      // reports for that file what it always reported
      for (size_t i : g.second) {
        Item &it = items[i];
        if (!c.ctx) it.fail("encoding", c.error.c_str());
        else if (!batched && glc_encode_int(c.ctx, it.pcm, it.fmt, it.bits, it.n, it.ch, &it.fr) != GLC_OK)
          it.fail("encoding", glc_last_error(c.ctx));
      }
    }
    for (size_t i = done; i < end; ++i) {
      Item &it = items[i];
      glc_free(it.pcm);
      it.pcm = nullptr;
      if (it.pending && !it.failed) {  // written in argument order: two inputs may name one output
        const std::string out = with_ext(it.path, "glc");
        if (glc_save(it.fr, out.c_str()) != GLC_OK) {
          it.fail("encoding", glc_last_error(nullptr));
        } else {
          const long a = file_size(it.path), b = file_size(out);
          it.out += fmt_line("Saved: \"%s\" (%ld bytes, %.1f%% of original)\n", file_name(out).c_str(), b, 100.0 * b / a);
        }
      }
      glc_frames_free(it.fr);
      it.fr = nullptr;
      it.pending = false;
      failed |= it.failed;
      emit(it);
      it.out.clear(), it.err.clear();
    }
    done = end;
    held = 0;
  };
  for (size_t i = 0; i < args.size(); ++i) {
    Item &it = items[i];
    it.path = args[i];
    if (!exists(it.path)) {
      it.err = fmt_line("Error: File not found: \"%s\"\n", it.path.c_str());
      it.failed = true;
      continue;
    }
    if (lower_ext(it.path) != "wav" && lower_ext(it.path) != "flac") {
      it.err = fmt_line("Error: Unsupported file type: \"%s\"\nSupported formats: WAV, FLAC\n", it.path.c_str());
      it.failed = true;
      continue;
    }
    it.out = fmt_line("Loading: \"%s\"\n", file_name(it.path).c_str());
    if (glc_audio_load_pcm(it.path.c_str(), &it.pcm, &it.fmt, &it.bits, &it.n, &it.sr, &it.ch) != GLC_OK) {
      it.fail("encoding", glc_last_error(nullptr));
      continue;
    }
    it.out += fmt_line("Encoding: %u Hz, %u channels, %llu samples\n", it.sr, it.ch, static_cast<unsigned long long>(it.n));
    glc_plan plan;
    if (glc_plan_encode(it.n, it.ch, &plan) != GLC_OK || plan.n_frames == 0) {
      // a file the batch call would refuse must not take its group down: the single call says why
      Contexts::Entry &c = contexts.get(it.sr);
      if (!c.ctx) it.fail("encoding", c.error.c_str());
      else if (glc_encode_int(c.ctx, it.pcm, it.fmt, it.bits, it.n, it.ch, &it.fr) != GLC_OK) it.fail("encoding", glc_last_error(c.ctx));
      else it.pending = true;  // (not reached: the plan and the call agree)
      glc_free(it.pcm);
      it.pcm = nullptr;
      continue;
    }
    it.pending = true;
    held += it.n * (it.fmt == GLC_PCM_S16 ? 2u : 4u);
    if (held > kHeldPcmBudget) flush(i + 1);
  }
  flush(items.size());
  return failed;
}

// `glc -d g1 g2 ...`, src/main.rs:364-456 around decode_file, for the files that passed the argument checks
static bool decode_many(const std::vector<std::string> &files, bool wav, unsigned flac_level) {
  Contexts contexts;
  std::vector<Item> items(files.size());
  size_t done = 0;
  uint64_t held = 0;
  bool failed = false;
  std::vector<std::vector<int16_t>> buffers;  // one per group of a flush
  auto flush = [&](size_t end) {
    // one batch call per channel count (what glc_decode_batch_i16 shares; sample rates may differ inside a
    // call), on the context of the group's first file
    std::map<uint16_t, std::vector<size_t>> groups;
    for (size_t i = done; i < end; ++i)
      if (items[i].pending) groups[items[i].ch].push_back(i);
    buffers.clear();
    for (auto &g : groups) {
      Contexts::Entry &c = contexts.get(items[g.second[0]].sr);
      std::vector<const glc_frames *> in;
      uint64_t total = 0;
      for (size_t i : g.second) in.push_back(items[i].fr), total += glc_decoded_len(items[i].fr);
      buffers.emplace_back(total);
      int16_t *buf = buffers.back().data();
      std::vector<uint64_t> off(in.size() + 1, 0);
      // both outputs are 16-bit (convert_f32_to_i16, src/audio.rs:11-16, src/flac.rs:955-958): narrowed on the device
      const bool batched = c.ctx && in.size() > 1 && glc_decode_batch_i16(c.ctx, in.data(), in.size(), buf, total, off.data()) == GLC_OK;
      uint64_t at = 0;
      for (size_t k = 0; k < in.size(); ++k) {
        Item &it = items[g.second[k]];
        const uint64_t len = glc_decoded_len(it.fr);
        it.dec = buf + at;
        it.n = len;
        // alone in its group, or the batch call failed as a whole (one malformed stream does that): every
        // file through the single call, which reports for that file what it always reported
        if (!c.ctx) it.fail("decoding", c.error.c_str());
        else if (!batched && glc_decode_i16(c.ctx, it.fr, buf + at, len, &it.n) != GLC_OK) it.fail("decoding", glc_last_error(c.ctx));
        at += len;
      }
    }
    for (size_t i = done; i < end; ++i) {
      Item &it = items[i];
      glc_frames_free(it.fr);
      it.fr = nullptr;
      if (it.pending && !it.failed) {
        it.out += fmt_line("Decoded %llu samples\n", static_cast<unsigned long long>(it.n));
        const std::string out = with_ext(it.path, wav ? "wav" : "flac");
        const int rc = wav ? glc_wav_save16_i16(out.c_str(), it.dec, it.n, it.sr, it.ch)
                           : glc_flac_save_i16(out.c_str(), it.dec, it.n, it.sr, it.ch, static_cast<uint8_t>(flac_level));
        if (rc != GLC_OK) it.fail("decoding", glc_last_error(nullptr));
        else if (wav) it.out += fmt_line("Saved: \"%s\" (WAV)\n", file_name(out).c_str());
        else it.out += fmt_line("Saved: \"%s\" (FLAC, level %u)\n", file_name(out).c_str(), flac_level);
      }
      it.pending = false;
      failed |= it.failed;
      emit(it);
      it.out.clear(), it.err.clear();
    }
    buffers.clear();
    done = end;
    held = 0;
  };
  for (size_t i = 0; i < files.size(); ++i) {
    Item &it = items[i];
    it.path = files[i];
    it.out = fmt_line("Loading: \"%s\"\n", file_name(it.path).c_str());
    if (glc_load(it.path.c_str(), &it.fr) != GLC_OK) {
      it.fail("decoding", glc_last_error(nullptr));
      continue;
    }
    glc_info info;
    glc_frames_info(it.fr, &info);
    it.sr = info.sample_rate, it.ch = info.channels;
    it.out += fmt_line("Decoding: %u Hz, %u channels\n", info.sample_rate, info.channels);
    it.pending = true;
    held += glc_decoded_len(it.fr) * 2;
    if (held > kHeldPcmBudget) flush(i + 1);
  }
  flush(items.size());
  return failed;
}

static void print_usage() {
  std::fprintf(stderr,
               "Usage:\n"
               "  glc <file.wav|file.flac> ...                    Encode audio files to .glc (MI355X)\n"
               "  glc -d <file.glc> ... [--wav] [--flac-level N]  Decode .glc files\n"
               "\n"
               "Options:\n"
               "  -d, --decode       Decode .glc files to FLAC (default) or WAV\n"
               "      --wav          Output WAV format instead of FLAC\n"
               "      --flac-level   Set FLAC compression level 0-8 (default: 5)\n"
               "\n"
               "Playback (-p) and the GUI are not part of this build; use the reference binary.\n");
}

int main(int argc, char **argv) {
  if (argc < 2) {  // the reference launches its GUI here, or prints the usage without the ui feature
    print_usage();
    return 1;
  }
  const std::string first = argv[1];
  if (first == "-h" || first == "--help") {
    print_usage();
    return 1;
  }
  if (first == "-p" || first == "--play") {
    std::fprintf(stderr, "Error: playback stays with the reference binary\n");
    return 1;
  }
  bool failed = false;
  if (first == "-d" || first == "--decode") {  // src/main.rs:364-456
    if (argc < 3) {
      std::fprintf(stderr, "Error: -d requires at least one .glc file\n");
      print_usage();
      return 1;
    }
    bool wav = false;
    unsigned level = 5;
    std::vector<std::string> files;
    for (int i = 2; i < argc; ++i) {
      const std::string a = argv[i];
      if (a == "--wav") {
        wav = true;
      } else if (a == "--flac-level") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "Error: --flac-level requires a value (0-8)\n");
          return 1;
        }
        const std::string v = argv[++i];  // `parse::<u8>()`: optional '+', digits, <= 255
        size_t k = (!v.empty() && v[0] == '+') ? 1 : 0;
        bool ok = k < v.size() && v.size() - k <= 3;
        for (size_t j = k; ok && j < v.size(); ++j) ok = std::isdigit(static_cast<unsigned char>(v[j])) != 0;
        const unsigned long parsed = ok ? std::strtoul(v.c_str() + k, nullptr, 10) : 256;
        if (parsed > 255) {
          std::fprintf(stderr, "Error: Invalid FLAC level, must be 0-8\n");
          return 1;
        }
        if (parsed > 8) {
          std::fprintf(stderr, "Error: FLAC level must be 0-8\n");
          return 1;
        }
        level = static_cast<unsigned>(parsed);
      } else if (!exists(a)) {
        std::fprintf(stderr, "Error: File not found: \"%s\"\n", a.c_str());
        failed = true;
      } else if (lower_ext(a) != "glc") {
        std::fprintf(stderr, "Error: Not a .glc file: \"%s\"\n", a.c_str());
        failed = true;
      } else {
        files.push_back(a);
      }
    }
    if (files.empty()) {
      std::fprintf(stderr, "Error: No valid .glc files to decode\n");
      return 1;
    }
    if (files.size() > 1) return (decode_many(files, wav, level) || failed) ? 1 : 0;
    for (const std::string &f : files) failed |= decode_file(f, wav, level) != 0;
    return failed ? 1 : 0;
  }
  size_t valid = 0;
  for (int i = 1; i < argc; ++i) valid += exists(argv[i]) && (lower_ext(argv[i]) == "wav" || lower_ext(argv[i]) == "flac");
  if (valid > 1) return encode_many(std::vector<std::string>(argv + 1, argv + argc)) ? 1 : 0;
  for (int i = 1; i < argc; ++i) {  // src/main.rs:546-581: keep going, exit 1 if any file failed
    const std::string a = argv[i];
    if (!exists(a)) {
      std::fprintf(stderr, "Error: File not found: \"%s\"\n", a.c_str());
      failed = true;
    } else if (lower_ext(a) != "wav" && lower_ext(a) != "flac") {
      std::fprintf(stderr, "Error: Unsupported file type: \"%s\"\nSupported formats: WAV, FLAC\n", a.c_str());
      failed = true;
    } else {
      failed |= encode_file(a) != 0;
    }
  }
  return failed ? 1 : 0;
}
