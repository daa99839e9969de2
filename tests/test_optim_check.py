"""The optimiser step's arithmetic on the host (no GPU): sigmarl_amd/csrc/sigmaenv_optim.h compiled ALONE into a stand-alone program (tests/host_program.py: with
AddressSanitizer + UBSan where the compiler has them) against tests/optim_check.py -- the header's norm and element update equal the float32 twin bit for bit and
hold the derived float64 bounds, and every planted defect of the twin misses a bound.

Cases: tensors of 1, 4, 1023, 1024, 1025 and 1280 elements (one element, a short chunk, one below / exactly / one past a chunk, a second short chunk) in one network
and a second network that brings the partials to 270 (past the 256 lanes of the second-level sum); t = 1 (fresh moments) and t = 1000; all-zero gradients; a total
norm just below and just above max_grad_norm; a small norm under a small max_grad_norm (where the 1e-6 of the coefficient matters)."""
import struct

import numpy as np
import pytest

import host_program
import optim_check as oc

SMALL = [1280, 1, 1025, 4, 1023, 1024]
BIG = [131072, 256, 65541, 256, 65536, 256, 1024, 4]  # 128 + 1 + 65 + 1 + 64 + 1 + 1 + 1 = 262 chunks
SIZES = [SMALL, BIG]


def cases():
    c = {
        "t1_fresh_clipped": oc.make_case(SIZES, 1, t=1, fresh=True, grad_norm=3.0),
        "t1000_clipped": oc.make_case(SIZES, 2, t=1000, grad_norm=3.0),
        "t1000_unclipped": oc.make_case(SIZES, 3, t=1000, grad_norm=0.25),
        "t1_zero_grad": oc.make_case(SIZES, 4, t=1, fresh=True, zero_grad=True),
        "t1000_zero_grad": oc.make_case(SIZES, 5, t=1000, zero_grad=True),
        "just_below": oc.make_case(SIZES, 6, t=7, grad_norm=1.0 - 3e-6),
        "just_above": oc.make_case(SIZES, 7, t=7, grad_norm=1.0 + 3e-6),
        "small_norm_clipped": oc.make_case(SIZES, 8, t=1000, grad_norm=2e-3, max_grad_norm=1e-3),
        "one_small_network": oc.make_case([SMALL], 9, t=1, fresh=True, grad_norm=0.5),
    }
    return c


PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_optim.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  rd(in, &n_cases, 4);
  for (int c = 0; c < n_cases; ++c) {
    double hp[5];
    int64_t t = 0;
    int32_t nt = 0;
    rd(in, hp, sizeof hp); rd(in, &t, 8); rd(in, &nt, 4);
    std::vector<int32_t> n(nt);
    rd(in, n.data(), 4 * (size_t)nt);
    std::vector<std::vector<float>> g(nt), p(nt), m(nt), v(nt);
    std::vector<float> partial;
    for (int i = 0; i < nt; ++i) {
      for (std::vector<float>* x : {&g[i], &p[i], &m[i], &v[i]}) { x->resize(n[i]); rd(in, x->data(), 4 * (size_t)n[i]); }
      const int chunks = optim_chunks(n[i]);
      for (int k = 0; k < chunks; ++k) {
        const int off = k * OPTIM_CHUNK, len = n[i] - off < OPTIM_CHUNK ? n[i] - off : OPTIM_CHUNK;
        partial.push_back(optim_chunk_sumsq(g[i].data() + off, len));
      }
    }
    const float norm = optim_total_norm(optim_total_sumsq(partial.data(), (int)partial.size()));
    const OptimScalars sc = optim_scalars(hp[0], hp[1], hp[2], hp[3], hp[4], t);
    const float coef = optim_clip_coef(norm, sc.max_grad_norm);
    fwrite(&norm, 4, 1, out); fwrite(&coef, 4, 1, out);
    for (int i = 0; i < nt; ++i) {
      for (int e = 0; e < n[i]; ++e) optim_adam(sc, coef, g[i][e], p[i][e], m[i][e], v[i][e]);
      for (std::vector<float>* x : {&p[i], &m[i], &v[i]}) fwrite(x->data(), 4, (size_t)n[i], out);
    }
  }
  fclose(in); fclose(out);
  printf("ok %%d cases\n", (int)n_cases);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    """every case through the header compiled alone: {name: a ``step`` result}"""
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("optim_header")
    cs = cases()
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for case in cs.values():
            flat = [t for net in case["nets"] for t in net]
            f.write(struct.pack("<5dqi", case["lr"], case["beta1"], case["beta2"], case["eps"], case["max_grad_norm"], case["t"], len(flat)))
            f.write(np.asarray([t["g"].size for t in flat], np.int32).tobytes())
            for t in flat:
                for k in ("g", "p", "m", "v"):
                    f.write(np.ascontiguousarray(t[k], np.float32).tobytes())
    stdout = host_program.build_and_run(tmp, "optim_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(cs)} cases" in stdout
    raw = np.fromfile(tmp / "out.bin", np.float32)
    res, at = {}, 0
    for name, case in cs.items():
        r = {"total_norm": raw[at], "coef": raw[at + 1], "nets": []}
        at += 2
        for net in case["nets"]:
            rn = []
            for t in net:
                n = t["g"].size
                rn.append({"p": raw[at:at + n], "m": raw[at + n:at + 2 * n], "v": raw[at + 2 * n:at + 3 * n]})
                at += 3 * n
            r["nets"].append(rn)
        res[name] = r
    assert at == raw.size
    return cs, res


NAMES = ["t1_fresh_clipped", "t1000_clipped", "t1000_unclipped", "t1_zero_grad", "t1000_zero_grad", "just_below", "just_above",
         "small_norm_clipped", "one_small_network"]


def test_the_cases_cover_what_they_claim():
    cs = cases()
    assert list(cs) == NAMES
    assert oc.n_partials(cs["t1000_clipped"]) == 270 > 256 and oc.n_partials(cs["one_small_network"]) == 8
    f = lambda n: float(oc.step(cs[n], np.float64)["coef"])  # noqa: E731
    assert f("t1000_clipped") < 0.5 and f("t1000_unclipped") == 1.0 and f("just_below") == 1.0 and 1.0 - 1e-5 < f("just_above") < 1.0
    n32 = lambda n: float(oc.step(cs[n], np.float32)["total_norm"])  # noqa: E731
    assert n32("just_below") < 1.0 < n32("just_above")


@pytest.mark.parametrize("name", NAMES)
def test_header_equals_the_twin_bit_for_bit_and_holds_the_fp64_bounds(header_results, name):
    cs, res = header_results
    case, got = cs[name], res[name]
    twin = oc.step(case, np.float32)
    assert oc.same_bits(got, twin)
    worst = oc.compare(got, case)
    print(name, worst)
    assert all(w <= 1.0 for w in worst.values()), worst


@pytest.mark.parametrize("name", ["t1_zero_grad", "t1000_zero_grad"])
def test_zero_gradients(header_results, name):
    """norm 0, coefficient 1; with fresh moments no parameter moves; never a NaN from 0 / (0 + eps)"""
    cs, res = header_results
    case, got = cs[name], res[name]
    assert got["total_norm"] == 0.0 and got["coef"] == 1.0
    for net, gn in zip(case["nets"], got["nets"]):
        for t, r in zip(net, gn):
            assert all(np.isfinite(r[k]).all() for k in oc.KEYS)
            if name == "t1_zero_grad":
                assert np.array_equal(r["p"].view(np.uint32), t["p"].view(np.uint32)) and not r["m"].any() and not r["v"].any()


@pytest.mark.parametrize("defect", oc.DEFECTS)
def test_every_planted_defect_misses_a_bound(defect):
    """on the inputs above (t = 1 and t = 1000; clipped, unclipped and the small norm): the defective twin is outside a bound in at least one case, the sound twin
    inside all of them in every case"""
    cs = cases()
    missed = []
    for name in ("t1_fresh_clipped", "t1000_clipped", "t1000_unclipped", "small_norm_clipped"):
        assert all(w <= 1.0 for w in oc.compare(oc.step(cs[name], np.float32), cs[name]).values())
        worst = oc.compare(oc.step(cs[name], np.float32, defect=defect), cs[name])
        if any(w > 1.0 for w in worst.values()):
            missed.append(name)
    print(defect, missed)
    assert missed, defect


def test_a_non_finite_gradient_poisons_every_parameter_as_torch_does():
    case = oc.make_case([SMALL], 11, t=3, grad_norm=2.0)
    case["nets"][0][2]["g"][5] = np.nan
    r = oc.step(case, np.float32)
    assert np.isnan(r["coef"]) and all(np.isnan(t["p"]).all() for t in r["nets"][0])
