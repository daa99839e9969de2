// sigmaenv_pack.h -- the packed forms of the device networks' weights, stated ONCE: for every form "what word goes into destination slot i".  The *_create entry
// points loop over these functions on the host (sigmaenv_mlp32_create, sigmaenv_actor_create), the pack kernels of sigmaenv_load.inc / sigmaenv_grad.inc loop over
// them on the device (sigmaenv_mlp32_load_device, sigmaenv_actor_load_device): a created handle and a loaded one hold the same words because they run the same text.
// The forms: the exact fp32 MFMA fragments (sigmaenv_mlp32.inc), the exact fragments of W^T (sigmaenv_grad.inc), the split hi / lo fp16 fragments
// (sigmaenv_mlp32s.inc), the bf16 form of the fast actor (sigmaenv_actor.inc).
//
// Plain C++: no HIP include and no other file of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone (tests/test_weight_load_host.py and tests/test_gradient_check.py hold every function here, slot by slot, to
// the frozen packers of tests/weight_pack_reference.h).
//
// Roundings in integer arithmetic -- no hardware conversion, so the words do not depend on the compiler's target, a kernel's denormal or rounding mode; the two fp32
// operations of the split (w * 2^8, v - hi) are single IEEE operations on both sides (-ffp-contract=off; fp32 denormals are not flushed in this build).
#ifndef SIGMAENV_PACK_H
#define SIGMAENV_PACK_H
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define MLP32S_SW 256.0f   /* weight scale of the split form */
#define MLP32S_SX 256.0f   /* scale of the hidden activations */
#define MLP32S_SX0 16.0f   /* scale of the input rows */
#define MLP32_H 256        /* hidden width of a sigmaenv_mlp32 */
#define ACT_H 256          /* hidden width of a sigmaenv_actor */

// ---- the roundings ------------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_HD uint32_t load_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
SIGMA_HD float load_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

SIGMA_HD uint16_t load_f16_rne(float f) {
  uint32_t u = load_bits(f);
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
SIGMA_HD float load_f16_to_f32(uint16_t hv) {
  const uint32_t sign = (uint32_t)(hv & 0x8000u) << 16, e = (hv >> 10) & 31u, mant = hv & 0x3FFu;
  if (e == 0) return load_float(load_bits((float)mant * 5.9604644775390625e-08f) | sign);  // mant 2^-24: exact, a normal fp32 number (or zero)
  return load_float(sign | (e == 31 ? 0x7F800000u | (mant << 13) : ((e + 112u) << 23) | (mant << 13)));
}
SIGMA_HD uint16_t load_bf16_rne(float f) {
  uint32_t u = load_bits(f);
  if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);  // NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// a weight -> the (hi, lo) halves of the split form: hi = fp16(w 2^8), lo = fp16(w 2^8 - hi)
SIGMA_HD void load_split(float w, uint16_t& hi, uint16_t& lo) {
  const float v = w * MLP32S_SW;
  hi = load_f16_rne(v);
  lo = load_f16_rne(v - load_f16_to_f32(hi));
}
// the range of the split form: |w| < 255 (a NaN is outside)
SIGMA_HD bool load_out_of_range(float w) { return !((w < 0.0f ? -w : w) < 255.0f); }

// ---- the maps: (layer shape, destination slot) -> source index in the torch.nn.Linear weight [F][K], or -1: the slot is padding (zero) ---------------------------------
// exact form [Fp / 32][KQ][2][32][4], Kp = K padded to 8, Fp = F padded to 32: slot ((((ft KQ + kq) 2 + hh) 32 + mm) 4 + u holds weight (feature 32 ft + mm,
// k = 8 kq + 2 u + hh)
SIGMA_HD int load_exact_kp(int K) { return (K + 7) / 8 * 8; }
SIGMA_HD int load_exact_fp(int F) { return (F + 31) / 32 * 32; }
SIGMA_HD int load_exact_slots(int F, int K) { return load_exact_kp(K) * load_exact_fp(F); }
SIGMA_HD int load_exact_src(int F, int K, int d) {
  const int KQ = (K + 7) / 8;
  const int u = d & 3, mm = (d >> 2) & 31, hh = (d >> 7) & 1, q = d >> 8, ft = q / KQ, kq = q - ft * KQ;
  const int f = 32 * ft + mm, k = 8 * kq + 2 * u + hh;
  return f < F && k < K ? f * K + k : -1;
}
// the exact form of the TRANSPOSED weight (sigmaenv_grad.inc: delta W contracts over the features): [Kp / 32][FQ][2][32][4], Fp = F padded to 8, Kp = K padded to 32;
// slot ((((kt FQ + fq) 2 + hh) 32 + mm) 4 + u holds weight (feature f = 8 fq + 2 u + hh, k = 32 kt + mm) -- load_exact_src with the two indices' roles exchanged
SIGMA_HD int load_exact_t_slots(int F, int K) { return ((F + 7) / 8 * 8) * ((K + 31) / 32 * 32); }
SIGMA_HD int load_exact_t_src(int F, int K, int d) {
  const int FQ = (F + 7) / 8;
  const int u = d & 3, mm = (d >> 2) & 31, hh = (d >> 7) & 1, q = d >> 8, kt = q / FQ, fq = q - kt * FQ;
  const int k = 32 * kt + mm, f = 8 * fq + 2 * u + hh;
  return f < F && k < K ? f * K + k : -1;
}
// split form: (hi, lo) PAIRS; hidden layer [F / 32 tiles][KB][hi | lo][64 lanes][8], output layer (F <= 32) [KB][hi | lo][64 lanes][8].  Pair
// p = ((tile KB + kb) 64 + lane) 8 + j8 (output layer: tile = 0) has its hi half at 16-bit slot load_split_hi_slot(p), its lo half 512 slots (64 fragments) further;
// feature 32 tile + (lane & 31).  k slot (kb, hh = lane >> 5, j8) -> input feature: natural order (16 kb + 8 hh + j8) for the input layer, otherwise (chained) the
// accumulator order of the previous layer's tiles, 32 (kb >> 1) + (j & 3) + 8 (j >> 2) + 4 (kb & 1) with j = 8 hh + j8 (a lane's registers j = 8 hh .. 8 hh + 7 are
// one fragment of k block 2 t + h)
SIGMA_HD int load_split_kb(int K) { return (K + 15) / 16; }
SIGMA_HD int load_split_rows(int F, bool output_layer) { return output_layer ? 32 : (F + 63) / 64 * 64; }
SIGMA_HD int load_split_pairs(int F, int K, bool output_layer) { return load_split_rows(F, output_layer) * load_split_kb(K) * 16; }
SIGMA_HD int load_split_biases(bool output_layer) { return output_layer ? 32 : MLP32_H; }
SIGMA_HD int load_split_hi_slot(int p) { return ((p >> 9) << 10) | (p & 511); }
SIGMA_HD int load_split_src(int F, int K, bool chained, int p) {
  const int KB = (K + 15) / 16;
  const int j8 = p & 7, lane = (p >> 3) & 63, q = p >> 9, tile = q / KB, kb = q - tile * KB, hh = lane >> 5;
  const int j = 8 * hh + j8;
  const int k = chained ? 32 * (kb >> 1) + (j & 3) + 8 * (j >> 2) + 4 * (kb & 1) : 16 * kb + 8 * hh + j8;
  const int f = 32 * tile + (lane & 31);
  return f < F && k < K ? f * K + k : -1;
}
// bf16 form of the actor kernel [K / 32][4][Fp][8], Fp = F padded to 16, K to 32: slot (((kb 4 + g) Fp + f) 8 + j.  k slot (kb, g, j) -> input feature: natural order
// (32 kb + 8 g + j) for the input layer, otherwise (chained) the previous layer's accumulator layout, 16 (2 kb + (j >> 2)) + 4 g + (j & 3)
SIGMA_HD int load_bf16_slots(int F, int K) { return ((K + 31) / 32) * 4 * ((F + 15) / 16 * 16) * 8; }
SIGMA_HD int load_bf16_src(int F, int K, bool chained, int d) {
  const int Fp = (F + 15) / 16 * 16;
  const int j = d & 7, q = d >> 3, r = q / Fp, f = q - r * Fp, g = r & 3, kb = r >> 2;
  const int k = chained ? 16 * (2 * kb + (j >> 2)) + 4 * g + (j & 3) : 32 * kb + 8 * g + j;
  return f < F && k < K ? f * K + k : -1;
}

// ---- one layer of a sigmaenv_mlp32: both forms and both bias vectors ------------------------------------------------------------------------------------------------
// Lane index ranges: [0, n_exact) exact slots, then n_pairs split pairs (0 when the network holds no usable split form), then the exact biases [fp_exact], then the
// split biases [fp_split].  The pointers are host memory (create) or device memory (load).
struct Mlp32Layer {
  const float *w, *b;  // the source in torch.nn.Linear layout: [F][K], [F]
  float *ew, *eb;      // exact form
  uint16_t* sw;        // split form
  float* sb;
  int F, K, chained, output_layer;
  int n_exact, n_pairs, fp_exact, fp_split;
  float bscale;        // MLP32S_SW times the scale of the layer's inputs
  uint32_t* range;     // the load kernel's: |= 1 when a weight is outside the split form's range
};
// the shape of layer l of a network dims[0] -> .. -> dims[n_layers] (pointers: null).  split_fits: the split kernel takes the input width; a network that is
// exact-only by its width never reads its split form, which is then not written
SIGMA_HD Mlp32Layer pack_mlp32_layer(const int32_t* dims, int l, int n_layers, bool split_fits) {
  Mlp32Layer a{};
  a.K = dims[l]; a.F = dims[l + 1];
  a.chained = l > 0; a.output_layer = l + 1 == n_layers;
  a.n_exact = load_exact_slots(a.F, a.K); a.fp_exact = load_exact_fp(a.F);
  a.n_pairs = split_fits ? load_split_pairs(a.F, a.K, a.output_layer != 0) : 0;
  a.fp_split = split_fits ? load_split_biases(a.output_layer != 0) : 0;
  a.bscale = MLP32S_SW * (l == 0 ? MLP32S_SX0 : MLP32S_SX);
  return a;
}
SIGMA_HD int pack_mlp32_lanes(const Mlp32Layer& a) { return a.n_exact + a.n_pairs + a.fp_exact + a.fp_split; }
// writes what lane index i owns; true: it saw a weight outside the split form's range (the exact slots read every source weight exactly once)
SIGMA_HD bool pack_mlp32_slot(const Mlp32Layer& a, int i) {
  if (i < a.n_exact) {
    const int s = load_exact_src(a.F, a.K, i);
    const float v = s >= 0 ? a.w[s] : 0.0f;
    a.ew[i] = v;
    return s >= 0 && load_out_of_range(v);
  }
  if (i < a.n_exact + a.n_pairs) {
    const int p = i - a.n_exact, s = load_split_src(a.F, a.K, a.chained != 0, p), d = load_split_hi_slot(p);
    uint16_t hi = 0, lo = 0;
    if (s >= 0) load_split(a.w[s], hi, lo);
    a.sw[d] = hi; a.sw[d + 512] = lo;
  } else if (i < a.n_exact + a.n_pairs + a.fp_exact) {
    const int f = i - a.n_exact - a.n_pairs;
    a.eb[f] = f < a.F ? a.b[f] : 0.0f;
  } else {
    const int f = i - a.n_exact - a.n_pairs - a.fp_exact;
    a.sb[f] = f < a.F ? a.b[f] * a.bscale : 0.0f;
  }
  return false;
}
// the transposed exact form of one layer: slot i of tw
SIGMA_HD void pack_mlp32_t_slot(const float* w, float* tw, int F, int K, int i) {
  const int s = load_exact_t_src(F, K, i);
  tw[i] = s >= 0 ? w[s] : 0.0f;
}

// ---- one layer of a sigmaenv_actor: n_slots bf16 slots, then nb biases (the first F from b, zeros behind) --------------------------------------------------------------
struct ActorLayer {
  const float *w, *b;  // the source in torch.nn.Linear layout: [F][K], [F]
  uint16_t* pw;
  float* pb;
  int F, K, chained, n_slots, nb;
};
// the shape of layer l = 0 .. 3 of the actor D -> 256 -> 256 -> 256 -> 4 (pointers: null); the last layer's biases are padded to one tile of 16
SIGMA_HD ActorLayer pack_actor_layer(int D, int l) {
  ActorLayer a{};
  a.K = l == 0 ? D : ACT_H; a.F = l == 3 ? 4 : ACT_H;
  a.chained = l > 0;
  a.n_slots = load_bf16_slots(a.F, a.K); a.nb = l == 3 ? 16 : ACT_H;
  return a;
}
SIGMA_HD void pack_actor_slot(const ActorLayer& a, int i) {
  if (i < a.n_slots) {
    const int s = load_bf16_src(a.F, a.K, a.chained != 0, i);
    a.pw[i] = s >= 0 ? load_bf16_rne(a.w[s]) : (uint16_t)0;
  } else {
    const int f = i - a.n_slots;
    a.pb[f] = f < a.F ? a.b[f] : 0.0f;
  }
}
#endif  // SIGMAENV_PACK_H
