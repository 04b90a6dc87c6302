// glc_tables.cpp — host-side generation of the codec's constant tables.
//
// Replaces MdctTables::new (src/codec.rs:326-356) and PerceptualWeights::new /
// compute_critical_bands (src/codec.rs:102-183) of the reference.  The tables are part of the
// codec's definition: the cosine table is evaluated at f32-rounded angles of up to 8037 rad with
// the system libm's cosf (which is not correctly rounded), so a device-side or "exact" cosine
// would define a different transform.  They are therefore built once on the
// host, in binary32 with contraction off, and uploaded.
#include <cmath>
#include <cstring>

#include "glc_common.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace glc {

namespace {
constexpr float kPi = 3.14159265358979323846f;  // std::f32::consts::PI

// Piecewise perceptual weight of one bin, src/codec.rs:107-132.
float bin_weight(uint32_t k, float sr) {
  const float n = static_cast<float>(kHop);
  const float hz = (static_cast<float>(k) / (2.0f * n)) * sr;
  float w;
  if (hz < 100.0f)
    w = 0.3f + (hz / 100.0f) * 0.4f;
  else if (hz < 200.0f)
    w = 0.7f + ((hz - 100.0f) / 100.0f) * 0.3f;
  else if (hz < 5000.0f)
    w = 1.0f;
  else if (hz < 10000.0f)
    w = 1.0f - ((hz - 5000.0f) / 5000.0f) * 0.3f;
  else
    w = 0.7f - std::fmin((hz - 10000.0f) / 12000.0f, 1.0f) * 0.5f;
  return std::fmax(w, 0.2f);
}
}  // namespace

void build_host_tables(uint32_t sample_rate, HostTables &t) {
  t.sample_rate = sample_rate;
  const float n = static_cast<float>(kHop);

  // --- MdctTables::new ---------------------------------------------------------------
  t.cos_table.resize(static_cast<size_t>(kHop) * kFrame);
  t.cos_table_t.resize(static_cast<size_t>(kHop) * kFrame);
  const float pi_over_n = kPi / n;
  std::vector<float> pre(kFrame);  // (PI/n) * (i + 0.5 + n/2), rounded after each op
  for (uint32_t i = 0; i < kFrame; ++i) {
    const float shifted = (static_cast<float>(i) + 0.5f) + n / 2.0f;
    pre[i] = pi_over_n * shifted;
  }
  for (uint32_t k = 0; k < kHop; ++k) {
    const float kk = static_cast<float>(k) + 0.5f;
    float *row = &t.cos_table[static_cast<size_t>(k) * kFrame];
    for (uint32_t i = 0; i < kFrame; ++i) {
      const float angle = pre[i] * kk;
      const float c = cosf(angle);
      row[i] = c;
      t.cos_table_t[static_cast<size_t>(i) * kHop + k] = c;
    }
  }
  t.window.resize(kFrame);
  for (uint32_t i = 0; i < kFrame; ++i) {
    const float x = kPi * (static_cast<float>(i) + 0.5f);
    t.window[i] = sinf(x / static_cast<float>(kFrame));
  }
  t.norm = sqrtf(2.0f / n);

  // --- PerceptualWeights::new --------------------------------------------------------
  const float sr = static_cast<float>(sample_rate);
  t.weights.resize(kHop);
  for (uint32_t k = 0; k < kHop; ++k) t.weights[k] = bin_weight(k, sr);

  t.edges.clear();
  t.edges.push_back(0);
  const float nyquist = sr / 2.0f;
  for (float f = 0.0f; f < nyquist && t.edges.size() < 50;) {
    const uint32_t bin = static_cast<uint32_t>((f / nyquist) * n);
    if (bin > t.edges.back() && bin < kHop) t.edges.push_back(bin);
    f += f < 500.0f ? 50.0f : f < 2000.0f ? 100.0f : f < 8000.0f ? 250.0f : 500.0f;
  }
  t.edges.push_back(kHop);

  // --- frame-invariant parts of compute_masking_thresholds (src/codec.rs:218-228) -----
  const size_t nb = t.edges.size() - 1;
  t.band_pf.assign(nb, 0.f);
  t.band_len.assign(nb, 1.f);
  t.band_of.assign(kHop, 0);
  for (size_t b = 0; b < nb; ++b) {
    const uint32_t lo = t.edges[b], hi = t.edges[b + 1];
    float acc = 0.0f;
    for (uint32_t i = lo; i < hi; ++i) {
      acc = acc + t.weights[i];
      t.band_of[i] = static_cast<uint16_t>(b);
    }
    const float len = static_cast<float>(hi - lo);
    const float avg = acc / len;
    t.band_len[b] = len;
    t.band_pf[b] = 1.0f / std::fmax(avg, 0.1f);
  }
  t.indiv.resize(kHop);
  for (uint32_t k = 0; k < kHop; ++k) t.indiv[k] = 1.0f / std::fmax(t.weights[k], 0.1f);
  t.cf = std::fmax(1.0f - kQuality, 0.01f);
  t.noise_floor = powf(10.0f, kNoiseFloorDb / 20.0f);  // src/codec.rs:277
}

uint16_t bf16_round_nearest_even(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

void build_bound_table_image(const HostTables &t, uint32_t c0, std::vector<uint16_t> &out) {
  const uint32_t tiles = (kHop - c0) / 32;
  out.assign(static_cast<size_t>(kFrame / 16) * tiles * 2 * 64 * 8, 0);
  size_t at = 0;
  for (uint32_t kb = 0; kb < kFrame / 16; ++kb)
    for (uint32_t tile = 0; tile < tiles; ++tile)
      for (uint32_t piece = 0; piece < 2; ++piece)
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (uint32_t e = 0; e < 8; ++e) {
            const uint32_t k = c0 + tile * 32 + lane % 32, i = kb * 16 + 8 * (lane / 32) + e;
            const float v = t.cos_table[static_cast<size_t>(k) * kFrame + i];
            const uint16_t h1 = bf16_round_nearest_even(v);
            uint32_t hb = static_cast<uint32_t>(h1) << 16;
            float t1;
            std::memcpy(&t1, &hb, 4);
            out[at++] = piece == 0 ? h1 : bf16_round_nearest_even(v - t1);  // v - t1 is exact in f32
          }
}

}  // namespace glc
