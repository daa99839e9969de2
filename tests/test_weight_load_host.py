"""Host parts of the on-device weight refresh (sigmaenv_mlp32_load_device / sigmaenv_actor_load_device, sigmarl_amd/csrc/sigmaenv_load.inc; Mlp32.load / Actor.load):
the ABI, the refusals that happen before any device call, and the index maps + roundings of the pack kernels -- the `__host__ __device__` functions the kernels loop
over -- against the host packers of sigmaenv_mlp32_create / sigmaenv_actor_create, word for word, in a stand-alone host program.  No GPU needed."""
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

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
    assert "sigmaenv_load.inc" in src  # sigmaenv_build_id() covers the pack kernels
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


def _between(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


MAIN = r"""
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
int main() {
  const int Ks[] = {1, 7, 32, 35, 256, 512, 595}, Fs[] = {256, 4, 2, 1};
  long slots = 0;
  uint32_t seed = 1;
  for (int K : Ks)
    for (int F : Fs) {
      const bool output_layer = F != 256;
      { /* exact form: the loop of sigmaenv_mlp32_create */
        const std::vector<float> w = make_weights(F, K, true, seed++), b = make_weights(F, 1, true, seed++);
        const float* wp[1] = {w.data()};
        const float* bp[1] = {b.data()};
        std::vector<float> ref_w, ref_b;
        exact_pack_ref(wp, bp, 0, K, F, ref_w, ref_b);
        std::vector<float> got((size_t)load_exact_slots(F, K));
        for (int d = 0; d < (int)got.size(); ++d) { const int s = load_exact_src(F, K, d); got[d] = s >= 0 ? w[s] : 0.0f; }
        compare("exact", F, K, 0, got, ref_w);
        slots += (long)got.size();
      }
      for (int chained = 0; chained < 2; ++chained) {
        { /* split form: mlp32s_pack */
          const std::vector<float> w = make_weights(F, K, false, seed++);
          const std::vector<uint16_t> ref = mlp32s_pack(w.data(), F, K, chained != 0, output_layer);
          std::vector<uint16_t> got((size_t)load_split_pairs(F, K, output_layer) * 2, (uint16_t)0xDEAD);
          for (int p = 0; p < load_split_pairs(F, K, output_layer); ++p) {
            const int s = load_split_src(F, K, chained != 0, p), d = load_split_hi_slot(p);
            uint16_t hi = 0, lo = 0;
            if (s >= 0) load_split(w[s], hi, lo);
            if (d < 0 || (size_t)d + 512 >= got.size()) { printf("RANGE split F=%d K=%d pair %d -> slot %d\n", F, K, p, d); ++bad; continue; }
            got[d] = hi; got[d + 512] = lo;
          }
          compare("split", F, K, chained, got, ref);
          slots += (long)got.size();
        }
        { /* bf16 form: pack_layer */
          const std::vector<float> w = make_weights(F, K, true, seed++);
          const std::vector<uint16_t> ref = pack_layer(w.data(), F, K, chained != 0);
          std::vector<uint16_t> got((size_t)load_bf16_slots(F, K));
          for (int d = 0; d < (int)got.size(); ++d) { const int s = load_bf16_src(F, K, chained != 0, d); got[d] = s >= 0 ? load_bf16_rne(w[s]) : (uint16_t)0; }
          compare("bf16", F, K, chained, got, ref);
          slots += (long)got.size();
        }
      }
    }
  /* the roundings alone on many bit patterns (every exponent, mantissa edges), and the range predicate as sigmaenv_mlp32_create writes it */
  long words = 0;
  for (uint32_t e = 0; e < 256; ++e)
    for (uint32_t sgn = 0; sgn < 2; ++sgn)
      for (uint32_t mi = 0; mi < 4096; ++mi) {
        const uint32_t mant = mi < 2048 ? mi * 4099u % 0x800000u : 0x7FFFFFu - (mi - 2048) * 2053u;
        const uint32_t u = (sgn << 31) | (e << 23) | (mant & 0x7FFFFFu);
        float f; std::memcpy(&f, &u, 4);
        ++words;
        if (load_f16_rne(f) != f32_to_f16_rne(f)) { if (++bad <= 20) printf("MISMATCH f16 of %08x: %x, the packer has %x\n", u, load_f16_rne(f), f32_to_f16_rne(f)); }
        if (load_bf16_rne(f) != f32_to_bf16_rne(f)) { if (++bad <= 20) printf("MISMATCH bf16 of %08x\n", u); }
        if (load_out_of_range(f) != !(std::fabs(f) < 255.0f)) { if (++bad <= 20) printf("MISMATCH range of %08x\n", u); }
      }
  for (uint32_t hv = 0; hv < 65536; ++hv) {
    const float a = load_f16_to_f32((uint16_t)hv), b = f16_to_f32((uint16_t)hv);
    if (std::memcmp(&a, &b, 4) != 0) { if (++bad <= 20) printf("MISMATCH f16 -> f32 of %04x\n", hv); }
  }
  printf("%ld slots, %ld bit patterns compared: %ld mismatches, %ld zeros of the other sign\n", slots, words, bad, zero_sign);
  return bad || zero_sign ? 1 : 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None, reason="no host C++ compiler")
def test_index_maps_and_roundings_equal_the_host_packers(tmp_path):
    """Every destination slot of every form, K in {1, 7, 32, 35, 256, 512, 595} x F in {256, 4, 2, 1} (F < 256: the output layer's layout), chained and unchained:
    the map + conversion functions of sigmaenv_load.inc give the words of the host packers -- whose own text (mlp32s_pack with its roundings, pack_layer, the loop
    of sigmaenv_mlp32_create) is taken from the library's sources, so the program holds no GPU code.  Weights: the default initialisation range with +-0, values
    whose 2^8-fold is an fp16 subnormal (or below), exact fp16 / bf16 ties, 254.999, fp32 subnormals and (exact, bf16) 3e38, 300, inf, NaN planted.  A zero of the
    other sign is reported slot by slot and fails like any other difference: there is none.  Built with AddressSanitizer + UBSan where the compiler has them."""
    mlp32 = open(os.path.join(CSRC, "sigmaenv_mlp32.inc")).read()
    mlp32s = open(os.path.join(CSRC, "sigmaenv_mlp32s.inc")).read()
    actor = open(os.path.join(CSRC, "sigmaenv_actor.inc")).read()
    scales = "\n".join(re.findall(r"^#define MLP32S_S(?:W|X|X0) .*$", mlp32s, flags=re.M))
    assert scales.count("#define") == 3
    split_host = mlp32s[mlp32s.index("static uint16_t f32_to_f16_rne(float f) {"):]
    assert "mlp32s_pack(" in split_host and "__global__" not in split_host
    bf16_host = _between(actor, "static uint16_t f32_to_bf16_rne(float f) {", 'extern "C" void sigmaenv_actor_destroy')
    assert "pack_layer(" in bf16_host
    exact_loop = _between(mlp32, "    const int Kp = (K + 7) / 8 * 8, Fp = (F + 31) / 32 * 32, KQ = Kp / 8;", "    void *dw = nullptr, *db = nullptr;")
    assert "wt[" in exact_loop and "hip" not in exact_loop
    src = tmp_path / "maps_check.cpp"
    src.write_text("#include <cmath>\n#include <cstdint>\n#include <cstdio>\n#include <cstring>\n#include <vector>\n" + scales + "\n" + split_host + "\n" + bf16_host
                   + "\nstatic void exact_pack_ref(const float* const* weights, const float* const* biases, int l, int K, int F, std::vector<float>& wt_out, "
                   "std::vector<float>& bp_out) {\n" + exact_loop + "    wt_out = wt; bp_out = bp;\n}\n"
                   "#define SIGMA_HD static inline\n#define SIGMAENV_LOAD_MAPS_ONLY\n#include \"sigmaenv_load.inc\"\n" + MAIN)
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = tmp_path / "maps_check"
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:  # (a compiler without the sanitizer runtimes: the comparison itself does not need them)
        subprocess.check_call(base)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert " 0 mismatches, 0 zeros of the other sign" in run.stdout
