// weight_pack_reference.h -- the FROZEN reference of the packed weight forms: the host packers and roundings the library had before its packed forms were stated
// once in sigmarl_amd/csrc/sigmaenv_pack.h (scatter loops over the SOURCE elements, where the product gathers by DESTINATION slot), word for word as they stood
// there.  tests/test_weight_load_host.py and tests/test_gradient_check.py hold the product's per-slot functions to them in stand-alone host programs.
//
// This file is never edited to follow the library: a layout or rounding that changes in the product must fail against it, and is then a decision about the
// weights every existing handle holds, not a test to adapt.
#ifndef WEIGHT_PACK_REFERENCE_H
#define WEIGHT_PACK_REFERENCE_H
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// the weight scale of the split form, as mlp32s_pack names it; pinned here, whoever defined it
#ifndef MLP32S_SW
#define MLP32S_SW 256.0f
#endif
static_assert(MLP32S_SW == 256.0f, "the split form's weight scale is 2^8");

namespace ref {

// ---- split form: fp32 -> (hi, lo) fp16 fragments ---------------------------------------------------------------------------------------
static uint16_t f32_to_f16_rne(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  u &= 0x7FFFFFFFu;
  if (u >= 0x7F800000u) return (uint16_t)(sign | (u > 0x7F800000u ? 0x7E00u : 0x7C00u));
  if (u >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 rounds to infinity
  if (u < 0x38800000u) {                                     // below 2^-14: subnormal result, in units of 2^-24
    if (u < 0x33000000u) return sign;                        // below 2^-25
    const int e = (int)(u >> 23), shift = 126 - e;           // 14 .. 24
    const uint32_t mant = (u & 0x7FFFFFu) | 0x800000u;
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
  }
  const uint32_t r = u + 0xFFFu + ((u >> 13) & 1u);
  return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}
static float f16_to_f32(uint16_t hv) {
  const uint32_t sign = (uint32_t)(hv & 0x8000u) << 16, e = (hv >> 10) & 31u, mant = hv & 0x3FFu;
  float out;
  if (e == 0) {
    out = std::ldexp((float)mant, -24);
    uint32_t u;
    std::memcpy(&u, &out, 4);
    u |= sign;
    std::memcpy(&out, &u, 4);
    return out;
  }
  const uint32_t u = sign | (e == 31 ? 0x7F800000u | (mant << 13) : ((e + 112u) << 23) | (mant << 13));
  std::memcpy(&out, &u, 4);
  return out;
}

// input feature of k slot (kb, hh, j8) of a layer: natural order for the input layer, the accumulator order of the previous layer's tiles otherwise (a lane's
// registers j = 8 hh .. 8 hh + 7 are one fragment of k block 2 t + h)
static inline int mlp32s_feature_of_slot(bool chained, int kb, int hh, int j8) {
  if (!chained) return 16 * kb + 8 * hh + j8;
  const int j = 8 * hh + j8;
  return 32 * (kb >> 1) + (j & 3) + 8 * (j >> 2) + 4 * (kb & 1);
}

// torch.nn.Linear weight [F, K] -> split fragments.  hidden: [F / 32][KB][hi | lo][64 lanes][8]; output layer (F <= 32): [KB][hi | lo][64 lanes][8]
static std::vector<uint16_t> mlp32s_pack(const float* w, int F, int K, bool chained, bool output_layer) {
  const int KB = (K + 15) / 16, Fp = output_layer ? 32 : (F + 63) / 64 * 64;
  std::vector<uint16_t> out((size_t)Fp * KB * 16 * 2, 0);
  for (int f = 0; f < F; ++f)
    for (int kb = 0; kb < KB; ++kb)
      for (int hh = 0; hh < 2; ++hh)
        for (int j8 = 0; j8 < 8; ++j8) {
          const int k = mlp32s_feature_of_slot(chained, kb, hh, j8);
          if (k >= K) continue;
          const float v = w[(size_t)f * K + k] * MLP32S_SW;
          const uint16_t hi = f32_to_f16_rne(v), lo = f32_to_f16_rne(v - f16_to_f32(hi));
          const int lane = hh * 32 + (f & 31);
          size_t frag_hi;
          if (output_layer) frag_hi = ((size_t)kb * 2) * 64 + lane;
          else frag_hi = (((size_t)(f >> 5) * KB + kb) * 2) * 64 + lane;
          out[frag_hi * 8 + j8] = hi;
          out[(frag_hi + 64) * 8 + j8] = lo;
        }
  return out;
}

// ---- bf16 form of the fast actor -----------------------------------------------------------------------------------------------------------
static uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);  // NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// torch.nn.Linear weight [F, K] (row-major) -> [K/32][4][Fp][8] bf16 with the k-slot order of the MFMA chaining; `chained`: the
// input is the previous layer's accumulator layout (k slot (kb, g, j) <-> feature 16 (2 kb + (j >> 2)) + 4 g + (j & 3)), else natural
// (k slot (kb, g, j) <-> feature 32 kb + 8 g + j).  Fp = F padded to a multiple of 16, K padded to a multiple of 32 with zeros.
static std::vector<uint16_t> pack_layer(const float* w, int F, int K, bool chained) {
  const int Fp = (F + 15) / 16 * 16, KB = (K + 31) / 32;
  std::vector<uint16_t> out((size_t)KB * 4 * Fp * 8, 0);
  for (int kb = 0; kb < KB; ++kb)
    for (int g = 0; g < 4; ++g)
      for (int f = 0; f < F; ++f)
        for (int j = 0; j < 8; ++j) {
          const int k = chained ? 16 * (2 * kb + (j >> 2)) + 4 * g + (j & 3) : 32 * kb + 8 * g + j;
          if (k < K) out[(((size_t)kb * 4 + g) * Fp + f) * 8 + j] = f32_to_bf16_rne(w[(size_t)f * K + k]);
        }
  return out;
}

// ---- exact form: the loop of sigmaenv_mlp32_create, layer l of (weights, biases) ---------------------------------------------------------
static void exact_pack_ref(const float* const* weights, const float* const* biases, int l, int K, int F, std::vector<float>& wt_out, std::vector<float>& bp_out) {
    const int Kp = (K + 7) / 8 * 8, Fp = (F + 31) / 32 * 32, KQ = Kp / 8;
    // packed [Fp / 32][KQ][2][32][4]: weight (feature 32 ft + mm, k = 8 kq + 2 u + hh) at ((((ft KQ + kq) 2 + hh) 32 + mm) 4 + u
    std::vector<float> wt((size_t)Kp * Fp, 0.0f), bp(Fp, 0.0f);
    for (int f = 0; f < F; ++f) {
      bp[f] = biases[l][f];
      const int ft = f >> 5, mm = f & 31;
      for (int k = 0; k < K; ++k) {
        const int kq = k >> 3, u = (k & 7) >> 1, hh = k & 1;
        wt[((((size_t)ft * KQ + kq) * 2 + hh) * 32 + mm) * 4 + u] = weights[l][(size_t)f * K + k];
      }
    }
    wt_out = wt; bp_out = bp;
}

// ---- exact form of the transposed weight, from the layout alone: [Kp / 32][FQ][2][32][4] with Fp = F padded to 8 (FQ = Fp / 8), Kp = K padded to 32; weight
// (feature f = 8 fq + 2 u + hh, k = 32 kt + mm) at ((((kt FQ + fq) 2 + hh) 32 + mm) 4 + u; padding zeros
static std::vector<float> exact_t_pack_ref(const float* w, int F, int K) {
  const int Fp = (F + 7) / 8 * 8, Kp = (K + 31) / 32 * 32, FQ = Fp / 8;
  std::vector<float> tw((size_t)Fp * Kp, 0.0f);
  for (int f = 0; f < F; ++f)
    for (int k = 0; k < K; ++k) {
      const int fq = f >> 3, u = (f & 7) >> 1, hh = f & 1, kt = k >> 5, mm = k & 31;
      tw[((((size_t)kt * FQ + fq) * 2 + hh) * 32 + mm) * 4 + u] = w[(size_t)f * K + k];
    }
  return tw;
}
}  // namespace ref
#endif  // WEIGHT_PACK_REFERENCE_H
