// sigmaenv_load.inc -- a network's weights refreshed ON THE DEVICE from a learner's tensors (included by sigmaenv.hip after sigmaenv_mlp32.inc / sigmaenv_actor.inc;
// the contracts are in include/sigmaenv.h, sigmaenv_mlp32_load_device / sigmaenv_actor_load_device).
//
// What it restates: the host packers of sigmaenv_mlp32_create (the exact-fp32 fragment layout [Fp / 32][KQ][2][32][4] of its loop, the split hi / lo fp16 fragments
// of mlp32s_pack with the k order of mlp32s_feature_of_slot) and of sigmaenv_actor_create (pack_layer: bf16 [K / 32][4][Fp][8]) as index maps from a DESTINATION
// slot to its source element (or "zero": padding), plus the roundings of f32_to_f16_rne / f16_to_f32 / f32_to_bf16_rne in the same integer arithmetic -- no hardware
// conversion, so the words do not depend on the kernel's denormal or rounding mode; the two fp32 operations of the split (w * 2^8, v - hi) are single IEEE operations
// on both sides (-ffp-contract=off; fp32 denormals are not flushed in this build).  A loaded handle holds word for word what *_create makes from the same numbers
// (tests/test_weight_load_host.py loops every map over every slot against the host packers; tests/test_gpu_weight_load.py compares the networks' outputs).
//
// Mapping.  The whole job is 1 - 2 MB: nothing to tune.  One launch per layer, one lane per destination slot (grid-stride): consecutive lanes store consecutive
// words, padding slots are written as zeros like every other slot (no slot of a packed buffer keeps an old value), the source is gathered with 4-byte loads
// (torch.nn.Linear layout, 4-byte alignment suffices).  The exact pack reads every source weight exactly once: it also reduces the split form's range predicate
// (the one of sigmaenv_mlp32_create: !(|w| < 255), so a NaN is out of range) into one device word with a vector atomic OR.
//
// SIGMAENV_LOAD_MAPS_ONLY: the maps alone, for a stand-alone host program (SIGMA_HD, MLP32S_SW / SX / SX0 defined by the includer).
#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

// ---- the roundings (bit for bit f32_to_f16_rne, f16_to_f32 of sigmaenv_mlp32s.inc and f32_to_bf16_rne of sigmaenv_actor.inc) ---------------------------------------
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
// a weight -> the (hi, lo) halves of the split form (mlp32s_pack's three lines)
SIGMA_HD void load_split(float w, uint16_t& hi, uint16_t& lo) {
  const float v = w * MLP32S_SW;
  hi = load_f16_rne(v);
  lo = load_f16_rne(v - load_f16_to_f32(hi));
}
// the range of the split form as sigmaenv_mlp32_create tests it (a NaN is outside)
SIGMA_HD bool load_out_of_range(float w) { return !((w < 0.0f ? -w : w) < 255.0f); }

// ---- the maps: (layer shape, destination slot) -> source index in the torch.nn.Linear weight [F][K], or -1: the slot is padding (zero) ---------------------------------
// exact form, Kp = K padded to 8, Fp = F padded to 32: slot ((((ft KQ + kq) 2 + hh) 32 + mm) 4 + u holds weight (feature 32 ft + mm, k = 8 kq + 2 u + hh)
SIGMA_HD int load_exact_slots(int F, int K) { return ((K + 7) / 8 * 8) * ((F + 31) / 32 * 32); }
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
// split form: (hi, lo) PAIRS.  Pair p = ((tile KB + kb) 64 + lane) 8 + j8 (output layer: tile = 0) has its hi half at 16-bit slot load_split_hi_slot(p), its lo half
// 512 slots (64 fragments) further; feature 32 tile + (lane & 31), k slot (kb, hh = lane >> 5, j8) -> input feature as mlp32s_feature_of_slot
SIGMA_HD int load_split_rows(int F, bool output_layer) { return output_layer ? 32 : (F + 63) / 64 * 64; }
SIGMA_HD int load_split_pairs(int F, int K, bool output_layer) { return load_split_rows(F, output_layer) * ((K + 15) / 16) * 16; }
SIGMA_HD int load_split_hi_slot(int p) { return ((p >> 9) << 10) | (p & 511); }
SIGMA_HD int load_split_src(int F, int K, bool chained, int p) {
  const int KB = (K + 15) / 16;
  const int j8 = p & 7, lane = (p >> 3) & 63, q = p >> 9, tile = q / KB, kb = q - tile * KB, hh = lane >> 5;
  const int j = 8 * hh + j8;
  const int k = chained ? 32 * (kb >> 1) + (j & 3) + 8 * (j >> 2) + 4 * (kb & 1) : 16 * kb + 8 * hh + j8;
  const int f = 32 * tile + (lane & 31);
  return f < F && k < K ? f * K + k : -1;
}
// bf16 form of the actor kernel (pack_layer): slot (((kb 4 + g) Fp + f) 8 + j, Fp = F padded to 16, K to 32
SIGMA_HD int load_bf16_slots(int F, int K) { return ((K + 31) / 32) * 4 * ((F + 15) / 16 * 16) * 8; }
SIGMA_HD int load_bf16_src(int F, int K, bool chained, int d) {
  const int Fp = (F + 15) / 16 * 16;
  const int j = d & 7, q = d >> 3, r = q / Fp, f = q - r * Fp, g = r & 3, kb = r >> 2;
  const int k = chained ? 16 * (2 * kb + (j >> 2)) + 4 * g + (j & 3) : 32 * kb + 8 * g + j;
  return f < F && k < K ? f * K + k : -1;
}

#ifndef SIGMAENV_LOAD_MAPS_ONLY
namespace load {

// one layer of a sigmaenv_mlp32: both forms and both bias vectors.  Lane index ranges: [0, n_exact) exact slots, then n_pairs split pairs (0 when the network holds
// no usable split form), then the exact biases [fp_exact], then the split biases [fp_split]
struct Mlp32Layer {
  const float *w, *b;  // the learner's tensors: [F][K], [F]
  float *ew, *eb;      // exact form
  uint16_t* sw;        // split form
  float* sb;
  int F, K, chained, output_layer;
  int n_exact, n_pairs, fp_exact, fp_split;
  float bscale;        // MLP32S_SW times the scale of the layer's inputs
  uint32_t* range;     // |= 1 when a weight is outside the split form's range
};

__global__ void __launch_bounds__(256) sigmaenv_load_mlp32_kernel(Mlp32Layer a) {
  sigma_poison_lds();
  const int total = a.n_exact + a.n_pairs + a.fp_exact + a.fp_split;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < a.n_exact) {
      const int s = load_exact_src(a.F, a.K, i);
      const float v = s >= 0 ? a.w[s] : 0.0f;
      a.ew[i] = v;
      if (s >= 0 && load_out_of_range(v)) atomicOr(a.range, 1u);
    } else if (i < a.n_exact + a.n_pairs) {
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
  }
}

// one layer of a sigmaenv_actor: n_slots bf16 slots, then nb biases (the first F from b, zeros behind)
__global__ void __launch_bounds__(256) sigmaenv_load_actor_kernel(const float* __restrict__ w, const float* __restrict__ b, uint16_t* __restrict__ pw, float* __restrict__ pb, int F, int K,
                                                                  int chained, int n_slots, int nb) {
  sigma_poison_lds();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots + nb; i += gridDim.x * blockDim.x) {
    if (i < n_slots) {
      const int s = load_bf16_src(F, K, chained != 0, i);
      pw[i] = s >= 0 ? load_bf16_rne(w[s]) : (uint16_t)0;
    } else {
      const int f = i - n_slots;
      pb[f] = f < F ? b[f] : 0.0f;
    }
  }
}

static int check_pointers(sigmaenv_t* h, const char* what, const float* const* weights_dev, const float* const* biases_dev, int n) {
  if (!weights_dev || !biases_dev) { h->err = std::string(what) + ": null pointer array"; return SIGMAENV_EINVAL; }
  for (int l = 0; l < n; ++l)
    if (!weights_dev[l] || !biases_dev[l] || ((uintptr_t)weights_dev[l] & 3) || ((uintptr_t)biases_dev[l] & 3)) {
      h->err = std::string(what) + ": layer " + std::to_string(l) + ": a null tensor or one that is not 4-byte aligned";
      return SIGMAENV_EINVAL;
    }
  return SIGMAENV_OK;
}

static inline int grid_for(int total) { return (total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024; }

}  // namespace load

static int mlp32_grad_load(sigmaenv_t* h, sigmaenv_mlp32* m, const float* const* weights_dev);  // sigmaenv_grad.inc: the transposed forms, same stream

extern "C" int sigmaenv_mlp32_load_device(sigmaenv_t* h, sigmaenv_mlp32* m, const float* const* weights_dev, const float* const* biases_dev) {
  if (!h) return SIGMAENV_EINVAL;
  if (!m || !m->range_word) { h->err = "mlp32_load_device: null network handle"; return SIGMAENV_EINVAL; }
  const int n = m->w.n_layers;
  if (int rc = load::check_pointers(h, "mlp32_load_device", weights_dev, biases_dev, n)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(m->range_word, 0, 4, h->stream));
  for (int l = 0; l < n; ++l) {
    const int K = m->dims[l], F = m->dims[l + 1];
    const bool last = l + 1 == n;
    load::Mlp32Layer a{};
    a.w = weights_dev[l]; a.b = biases_dev[l];
    a.ew = const_cast<float*>(m->w.w[l]); a.eb = const_cast<float*>(m->w.b[l]);
    a.sw = reinterpret_cast<uint16_t*>(const_cast<f16x8_t*>(m->ws.w[l])); a.sb = const_cast<float*>(m->ws.b[l]);
    a.F = F; a.K = K; a.chained = l > 0; a.output_layer = last;
    a.n_exact = load_exact_slots(F, K); a.fp_exact = m->w.Fp[l];
    // a network that is exact-only by its input width never reads its split form: not written
    a.n_pairs = m->split_fits ? load_split_pairs(F, K, last) : 0;
    a.fp_split = m->split_fits ? (last ? 32 : MLP32_H) : 0;
    a.bscale = MLP32S_SW * (l == 0 ? MLP32S_SX0 : MLP32S_SX);
    a.range = m->range_word;
    hipLaunchKernelGGL(load::sigmaenv_load_mlp32_kernel, dim3(load::grid_for(a.n_exact + a.n_pairs + a.fp_exact + a.fp_split)), dim3(256), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
  }
  if (const int rc = mlp32_grad_load(h, m, weights_dev)) return rc;
  // the one host wait: the range word decides which form the next forward launches
  uint32_t bad = 0;
  HIPCHK(h, hipMemcpyAsync(&bad, m->range_word, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  m->split_ok = m->split_fits && bad == 0;
  m->mode = (m->requested == SIGMAENV_MLP32_SPLIT && m->split_ok) ? SIGMAENV_MLP32_SPLIT : SIGMAENV_MLP32_EXACT;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_actor_load_device(sigmaenv_t* h, sigmaenv_actor* a, const float* const* weights_dev, const float* const* biases_dev) {
  if (!h) return SIGMAENV_EINVAL;
  if (!a) { h->err = "actor_load_device: null network handle"; return SIGMAENV_EINVAL; }
  if (int rc = load::check_pointers(h, "actor_load_device", weights_dev, biases_dev, 4)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const __bf16* pw[4] = {a->w.w1, a->w.w2, a->w.w3, a->w.w4};
  const float* pb[4] = {a->w.b1, a->w.b2, a->w.b3, a->w.b4};
  for (int l = 0; l < 4; ++l) {
    const int K = l == 0 ? a->D : ACT_H, F = l == 3 ? 4 : ACT_H;
    const int n_slots = load_bf16_slots(F, K), nb = l == 3 ? 16 : ACT_H;  // (sigmaenv_actor_create: the last layer's biases are padded to 16)
    hipLaunchKernelGGL(load::sigmaenv_load_actor_kernel, dim3(load::grid_for(n_slots + nb)), dim3(256), 0, h->stream, weights_dev[l], biases_dev[l],
                       reinterpret_cast<uint16_t*>(const_cast<__bf16*>(pw[l])), const_cast<float*>(pb[l]), F, K, l > 0 ? 1 : 0, n_slots, nb);
    HIPCHK(h, hipGetLastError());
  }
  return SIGMAENV_OK;
}
#endif  // SIGMAENV_LOAD_MAPS_ONLY
