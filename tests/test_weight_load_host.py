"""Host parts of the on-device weight refresh (sigmaenv_mlp32_load_device / sigmaenv_actor_load_device, sigmarl_amd/csrc/sigmaenv_load.inc; Mlp32.load / Actor.load):
the ABI, the refusals that happen before any device call, and the packed forms of sigmarl_amd/csrc/sigmaenv_pack.h -- the per-slot functions, index maps and roundings
that *_create loops over on the host and the pack kernels on the device -- against the frozen packers of tests/weight_pack_reference.h, word for word, in a
stand-alone host program.  No GPU needed."""
import os
import re
import types

import pytest
import torch

import host_program
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sigmarl_amd", "csrc")


def test_load_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ("mlp32_load_device", "actor_load_device"):
        assert "sigmaenv_" + name in capi.exported_symbols()
        assert name in capi._PRODUCT_ONLY
        assert f"int sigmaenv_{name}(sigmaenv_t* h, " in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_load.inc" in src and "sigmaenv_pack.h" in src  # sigmaenv_build_id() covers the pack kernels and the packed forms they write
    assert '#include "sigmaenv_load.inc"' in open(os.path.join(CSRC, "sigmaenv.hip")).read()


def _fake_env():
    return types.SimpleNamespace(B=4, N=3, D=5, device=torch.device("cuda", 0), parameters=None, lib=None, h=None, stream=None)


def _pairs(dims, **kw):
    return [(torch.zeros(dims[l + 1], dims[l], **kw), torch.zeros(dims[l + 1], **kw)) for l in range(len(dims) - 1)]


@pytest.mark.parametrize("which", ["mlp32", "actor"])
def test_load_refuses_bad_sources_before_any_device_call(which):
    """CPU tensors, float64, a wrong layer count, a transposed weight, a wrong bias length: TypeError / ValueError from the argument check -- the fake env has no
    library and no handle, so anything that went further would fail differently."""
    from sigmarl_amd.actor import Actor, Mlp32

    dims = [32, 256, 256, 256, 4]
    env = _fake_env()
    if which == "mlp32":
        net = types.SimpleNamespace(_keep=(dims, None, None))
        load = lambda src: Mlp32.load(net, env, src)  # noqa: E731
    else:
        net = types.SimpleNamespace(obs_dim=32)
        load = lambda src: Actor.load(net, env, src)  # noqa: E731
    good = _pairs(dims, device="meta")  # (shapes and dtype right, not CUDA memory: refused as well, but only for that)
    with pytest.raises(TypeError, match="CUDA"):
        load(_pairs(dims))                                   # host memory
    with pytest.raises(TypeError, match="CUDA"):
        load(good)
    with pytest.raises(TypeError, match="float32"):
        load(_pairs(dims, dtype=torch.float64))
    with pytest.raises(TypeError):
        load(3)
    with pytest.raises(ValueError, match="layers"):
        load(_pairs(dims[1:]))                               # three layers
    with pytest.raises(ValueError, match="layers"):
        load(torch.nn.Sequential(torch.nn.Linear(32, 256), torch.nn.Linear(256, 4)))
    # shape refusals need tensors that pass the device check: is_cuda / device are what the check reads
    def cuda_like(*shape, dtype=torch.float32):
        class T(torch.Tensor):
            is_cuda = True
            device = torch.device("cuda", 0)
        return torch.zeros(*shape, dtype=dtype).as_subclass(T)

    ok = [(cuda_like(dims[l + 1], dims[l]), cuda_like(dims[l + 1])) for l in range(4)]
    transposed = list(ok)
    transposed[0] = (cuda_like(dims[0], dims[1]), ok[0][1])
    with pytest.raises(ValueError, match="layer 0 weight"):
        load(transposed)
    short = list(ok)
    short[3] = (ok[3][0], cuda_like(3))
    with pytest.raises(ValueError, match="layer 3 bias"):
        load(short)
    wrong_dtype = list(ok)
    wrong_dtype[1] = (cuda_like(256, 256, dtype=torch.float64), ok[1][1])
    with pytest.raises(TypeError, match="layer 1 weight"):
        load(wrong_dtype)


PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define SIGMA_HD static inline
#include "sigmaenv_pack.h"
#include "weight_pack_reference.h"

static std::vector<float> special_values(bool huge) {
  std::vector<float> s = {0.0f, -0.0f,
    1e-7f, -3e-8f, 2.0e-9f, -2.0e-9f, 1e-10f,                       /* times 2^8: fp16 subnormals, and below the smallest one */
    (1.0f + 0x1p-11f) / 256.0f, -(1.0f + 3 * 0x1p-11f) / 256.0f,    /* exact fp16 ties of w 2^8 (to even: down, up) */
    0x1p-33f, 3 * 0x1p-33f, -0x1p-33f,                              /* ties among the fp16 subnormals (2^-25, 3 2^-25) */
    1.0f + 0x1p-8f, -(1.0f + 3 * 0x1p-8f),                          /* exact bf16 ties */
    254.999f, -254.999f, 1e-40f, -1e-40f, 1.4e-45f, -1.4e-45f,      /* the edge of the split range, fp32 subnormals */
    0.3333333f, -1.0f, 65504.0f / 256.0f, 100.0f};
  if (huge) { s.push_back(3e38f); s.push_back(-3e38f); s.push_back(300.0f); s.push_back(INFINITY); s.push_back(NAN); }
  return s;
}
static std::vector<float> make_weights(int F, int K, bool huge, uint32_t seed) {
  std::vector<float> w((size_t)F * K);
  uint32_t x = seed * 2654435761u + 12345u;
  const float bound = 1.0f / std::sqrt((float)K);
  for (auto& v : w) { x = x * 1664525u + 1013904223u; v = ((float)(x >> 8) / 8388608.0f - 1.0f) * bound; }
  const std::vector<float> s = special_values(huge);
  for (size_t i = 0; i < s.size(); ++i) {  /* spread over the matrix: first and last elements, and strided positions in between */
    w[(i * 7919u) % w.size()] = s[i];
    w[w.size() - 1 - (i * 104729u) % w.size()] = s[s.size() - 1 - i];
  }
  return w;
}
static long bad = 0, zero_sign = 0;
template <class T> static void compare(const char* form, int F, int K, int chained, const std::vector<T>& got, const std::vector<T>& ref) {
  if (got.size() != ref.size()) { printf("SIZE %s F=%d K=%d chained=%d: %zu slots, the packer has %zu\n", form, F, K, chained, got.size(), ref.size()); ++bad; return; }
  for (size_t i = 0; i < got.size(); ++i) {
    if (std::memcmp(&got[i], &ref[i], sizeof(T)) == 0) continue;
    uint32_t a = 0, b = 0;
    std::memcpy(&a, &got[i], sizeof(T)); std::memcpy(&b, &ref[i], sizeof(T));
    const uint32_t signbit = 1u << (8 * sizeof(T) - 1);
    if ((a & ~signbit) == 0 && (b & ~signbit) == 0) { ++zero_sign; printf("ZEROSIGN %s F=%d K=%d chained=%d slot %zu: %x, the packer has %x\n", form, F, K, chained, i, a, b); continue; }
    if (++bad <= 20) printf("MISMATCH %s F=%d K=%d chained=%d slot %zu: %x, the packer has %x\n", form, F, K, chained, i, a, b);
  }
}
static std::vector<float> in_range_weights(int F, int K, uint32_t seed) {  /* make_weights with every value outside the split range replaced */
  std::vector<float> w = make_weights(F, K, false, seed);
  for (auto& v : w) if (!(std::fabs(v) < 255.0f)) v = 0.5f;
  return w;
}
static bool range_ref(const std::vector<float>& w) {  /* the predicate as sigmaenv_mlp32_create wrote it, OR-ed over a layer's weights */
  bool out = false;
  for (float v : w) if (!(std::fabs(v) < 255.0f)) out = true;
  return out;
}
/* one layer (K -> F; chained: not the input layer) through the product's shape function and per-slot function, every lane index, against the reference packers;
   returns the range flag OR-ed over the lanes */
static bool mlp32_layer(int F, int K, int chained, bool output_layer, bool split_fits, const std::vector<float>& w, const std::vector<float>& b, long& slots) {
  int32_t dims[4] = {1, 1, 1, 1};
  dims[chained] = K; dims[chained + 1] = F;
  Mlp32Layer a = pack_mlp32_layer(dims, chained, chained + (output_layer ? 1 : 2), split_fits);
  if (a.F != F || a.K != K || a.chained != chained || (a.output_layer != 0) != output_layer) { printf("SHAPE F=%d K=%d chained=%d\n", F, K, chained); ++bad; }
  const float* wp[1] = {w.data()};
  const float* bp[1] = {b.data()};
  std::vector<float> ref_w, ref_b, ref_sb((size_t)(output_layer ? 32 : 256), 0.0f);
  ref::exact_pack_ref(wp, bp, 0, K, F, ref_w, ref_b);
  const std::vector<uint16_t> ref_s = ref::mlp32s_pack(w.data(), F, K, chained != 0, output_layer);
  for (int f = 0; f < F; ++f) ref_sb[f] = b[f] * (chained ? 65536.0f : 4096.0f);  /* 2^8 times the scale of the layer's inputs: 2^4 for the input rows, 2^8 behind a tanh */
  std::vector<float> ew((size_t)a.n_exact, 7.0f), eb((size_t)a.fp_exact, 7.0f), sb(ref_sb.size(), 7.0f);
  std::vector<uint16_t> sw(ref_s.size(), (uint16_t)0xDEAD);
  a.w = w.data(); a.b = b.data(); a.ew = ew.data(); a.eb = eb.data(); a.sw = sw.data(); a.sb = sb.data();
  if (split_fits && ((size_t)a.n_pairs * 2 != sw.size() || (size_t)a.fp_split != sb.size())) { printf("SIZE split F=%d K=%d: %d pairs, %d biases\n", F, K, a.n_pairs, a.fp_split); ++bad; return false; }
  if (!split_fits && (a.n_pairs != 0 || a.fp_split != 0)) { printf("SIZE unsplit F=%d K=%d\n", F, K); ++bad; return false; }
  bool flag = false;
  for (int i = 0, n = pack_mlp32_lanes(a); i < n; ++i) flag |= pack_mlp32_slot(a, i);
  compare("exact", F, K, chained, ew, ref_w);
  compare("exact bias", F, K, chained, eb, ref_b);
  if (split_fits) {
    compare("split", F, K, chained, sw, ref_s);
    compare("split bias", F, K, chained, sb, ref_sb);
  } else {  /* a network that is exact-only by its width: its split form is not touched */
    compare("unsplit", F, K, chained, sw, std::vector<uint16_t>(sw.size(), (uint16_t)0xDEAD));
    compare("unsplit bias", F, K, chained, sb, std::vector<float>(sb.size(), 7.0f));
  }
  slots += (long)(ew.size() + eb.size() + sw.size() + sb.size());
  return flag;
}
static void actor_layer(ActorLayer a, const std::vector<float>& w, const std::vector<float>& b, long& slots) {
  const std::vector<uint16_t> ref = ref::pack_layer(w.data(), a.F, a.K, a.chained != 0);
  std::vector<float> ref_b((size_t)a.nb, 0.0f);
  for (int f = 0; f < a.F; ++f) ref_b[f] = b[f];
  std::vector<uint16_t> pw((size_t)a.n_slots, (uint16_t)0xDEAD);
  std::vector<float> pb((size_t)a.nb, 7.0f);
  a.w = w.data(); a.b = b.data(); a.pw = pw.data(); a.pb = pb.data();
  for (int i = 0; i < a.n_slots + a.nb; ++i) pack_actor_slot(a, i);
  compare("bf16", a.F, a.K, a.chained, pw, ref);
  compare("bf16 bias", a.F, a.K, a.chained, pb, ref_b);
  slots += (long)(pw.size() + pb.size());
}
int main() {
  const int Ks[] = {1, 7, 32, 35, 256, 512, 595}, Fs[] = {256, 4, 2, 1};
  long slots = 0;
  uint32_t seed = 1;
  for (int K : Ks)
    for (int F : Fs) {
      const bool output_layer = F != 256;
      for (int chained = 0; chained < 2; ++chained) {
        { /* exact + split form and both bias vectors, with inf / NaN / 3e38 / 300 planted, then without; the range flag is the predicate OR-ed over the weights */
          for (int huge = 1; huge >= 0; --huge) {
            const std::vector<float> w = make_weights(F, K, huge != 0, seed++), b = make_weights(F, 1, true, seed++);
            const bool flag = mlp32_layer(F, K, chained, output_layer, true, w, b, slots);
            if (flag != range_ref(w) || (huge && w.size() >= 128 && !flag)) {  /* (a smaller matrix: the planted values overwrite one another) */ printf("RANGE F=%d K=%d chained=%d huge=%d: flag %d\n", F, K, chained, huge, (int)flag); ++bad; }
          }
          /* every weight inside the range: no flag; then a single NaN: flagged */
          std::vector<float> w = in_range_weights(F, K, seed++);
          const std::vector<float> b = make_weights(F, 1, false, seed++);
          if (mlp32_layer(F, K, chained, output_layer, true, w, b, slots) || range_ref(w)) { printf("RANGE F=%d K=%d chained=%d: flagged inside the range\n", F, K, chained); ++bad; }
          w[w.size() / 2] = NAN;
          if (!mlp32_layer(F, K, chained, output_layer, true, w, b, slots) || !range_ref(w)) { printf("RANGE F=%d K=%d chained=%d: a single NaN is not flagged\n", F, K, chained); ++bad; }
          if (K == 595) mlp32_layer(F, K, chained, output_layer, false, w, b, slots);
        }
        { /* bf16 form: pack_layer; biases padded to whole tiles of 16 */
          ActorLayer a{};
          a.F = F; a.K = K; a.chained = chained; a.n_slots = load_bf16_slots(F, K); a.nb = (F + 15) / 16 * 16;
          actor_layer(a, make_weights(F, K, true, seed++), make_weights(F, 1, true, seed++), slots);
        }
      }
    }
  /* the actor's own four layers, shapes from the function sigmaenv_actor_create and sigmaenv_actor_load_device share */
  for (int D = 8; D <= 32; D += 8)
    for (int l = 0; l < 4; ++l) {
      const ActorLayer a = pack_actor_layer(D, l);
      if (a.K != (l == 0 ? D : 256) || a.F != (l == 3 ? 4 : 256) || a.nb != (l == 3 ? 16 : 256) || a.chained != (l > 0) || a.n_slots != load_bf16_slots(a.F, a.K)) {
        printf("SHAPE actor D=%d layer %d\n", D, l); ++bad; continue;
      }
      actor_layer(a, make_weights(a.F, a.K, true, seed++), make_weights(a.F, 1, true, seed++), slots);
    }
  /* the roundings alone on many bit patterns (every exponent, mantissa edges), and the range predicate as sigmaenv_mlp32_create wrote it */
  long words = 0;
  for (uint32_t e = 0; e < 256; ++e)
    for (uint32_t sgn = 0; sgn < 2; ++sgn)
      for (uint32_t mi = 0; mi < 4096; ++mi) {
        const uint32_t mant = mi < 2048 ? mi * 4099u % 0x800000u : 0x7FFFFFu - (mi - 2048) * 2053u;
        const uint32_t u = (sgn << 31) | (e << 23) | (mant & 0x7FFFFFu);
        float f; std::memcpy(&f, &u, 4);
        ++words;
        if (load_f16_rne(f) != ref::f32_to_f16_rne(f)) { if (++bad <= 20) printf("MISMATCH f16 of %08x: %x, the packer has %x\n", u, load_f16_rne(f), ref::f32_to_f16_rne(f)); }
        if (load_bf16_rne(f) != ref::f32_to_bf16_rne(f)) { if (++bad <= 20) printf("MISMATCH bf16 of %08x\n", u); }
        if (load_out_of_range(f) != !(std::fabs(f) < 255.0f)) { if (++bad <= 20) printf("MISMATCH range of %08x\n", u); }
      }
  for (uint32_t hv = 0; hv < 65536; ++hv) {
    const float a = load_f16_to_f32((uint16_t)hv), b = ref::f16_to_f32((uint16_t)hv);
    if (std::memcmp(&a, &b, 4) != 0) { if (++bad <= 20) printf("MISMATCH f16 -> f32 of %04x\n", hv); }
  }
  printf("%ld slots, %ld bit patterns compared: %ld mismatches, %ld zeros of the other sign\n", slots, words, bad, zero_sign);
  return bad || zero_sign ? 1 : 0;
}
"""


@pytest.mark.skipif(host_program.compiler() is None, reason="no host C++ compiler")
def test_index_maps_and_roundings_equal_the_host_packers(tmp_path):
    """Every destination slot of every form, K in {1, 7, 32, 35, 256, 512, 595} x F in {256, 4, 2, 1} (F < 256: the output layer's layout), chained and unchained:
    the program includes sigmaenv_pack.h alone of the library, builds each layer's descriptor with the shape functions *_create and *_load_device use, runs the
    per-slot function they loop over across every lane index into buffers pre-filled with 0xDEAD / 7.0f, and compares exact weights, split words, bf16 words and all
    three bias vectors (padding and the split form's bias scale included) with the frozen packers of tests/weight_pack_reference.h.  The range flag returned over a
    layer is !(|w| < 255) OR-ed over its weights: with 3e38, 300, inf, NaN planted, without them, with every weight inside the range (no flag), and with a single NaN.
    Weights: the default initialisation range with +-0, values whose 2^8-fold is an fp16 subnormal (or below), exact fp16 / bf16 ties, 254.999, fp32 subnormals.
    Then 2 M bit patterns through each rounding and all 65536 fp16 patterns.  A zero of the other sign is reported slot by slot and fails like any other
    difference: there is none.  Built with AddressSanitizer + UBSan where the compiler has them."""
    out = host_program.build_and_run(tmp_path, "maps_check", PROGRAM)
    assert " 0 mismatches, 0 zeros of the other sign" in out


def test_each_layout_map_is_stated_in_the_pack_header_only():
    """The destination-slot maps are defined AND used in sigmaenv_pack.h alone: every other source of the library reaches a packed form through the header's per-slot
    functions, and the scatter packers the header replaced have not come back."""
    for name in sorted(os.listdir(CSRC)):
        if name == "sigmaenv_pack.h" or not name.endswith((".h", ".inc", ".hip")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for word in ("load_exact_src", "load_split_src", "load_bf16_src", "load_exact_t_src",
                     "f32_to_f16_rne", "f16_to_f32", "mlp32s_feature_of_slot", "mlp32s_pack", "f32_to_bf16_rne", "pack_layer", "mlp32_pack_transposed", "mlp32_grad_create"):
            assert not re.search(r"\b" + word + r"\b", text), f"{name} names {word}"
    pack = open(os.path.join(CSRC, "sigmaenv_pack.h")).read()
    for word in ("load_exact_src", "load_split_src", "load_bf16_src", "load_exact_t_src"):
        assert len(re.findall(r"SIGMA_HD int " + word + r"\(", pack)) == 1
    assert "hip" not in pack.replace("sigmaenv.hip", "") and pack.count("#include") == 1  # plain C++: <stdint.h> and nothing of the library
