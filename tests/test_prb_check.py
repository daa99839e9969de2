"""The prioritized buffer's arithmetic on the host (no GPU): sigmarl_amd/csrc/sigmaenv_prb.h compiled ALONE into a stand-alone program (tests/host_program.py: with
AddressSanitizer + UBSan where the compiler has them) against tests/prb_check.py -- the header's levels, total, q_min, indices, x_m and td equal the float32 twin bit
for bit, every index is admissible against float64 prefix sums, and every planted defect of the twin misses a bar.

Sizes: len = 1, 2, 255, 256, 257 (the second level appears), 65536, 65537 (the third level appears), 65792; capacity 512 with len 300 (the tail unfilled); M = 1, 64,
65, 512.  Leaves: random, all equal, one leaf 10^4 times the rest, the mass in the last leaf of a chunk and the first of the next, one NaN leaf (the index is still in
[0, len): nothing else is asserted about it); u forced to its extremes 2^-25 and 1.0."""
import struct

import numpy as np
import pytest

import host_program
import prb_check as pc

f32 = np.float32


def sample_cases():
    """{name: (capacity, len, leaves [len], M, forced u or None)}"""
    cs = {}
    for k, (length, M) in enumerate([(1, 1), (2, 64), (255, 65), (256, 512), (257, 64), (65536, 65), (65537, 512), (65792, 64)]):
        cs[f"random_len{length}_M{M}"] = (length, length, pc.twin_priority(pc.make_td("random", length, 10 + k)), M, None)
    cs["tail_cap512_len300"] = (512, 300, pc.twin_priority(pc.make_td("random", 300, 30)), 512, None)
    for length in (257, 65537):
        for kind in ("all_equal", "one_huge", "chunk_edge", "nan_leaf"):
            cs[f"{kind}_len{length}"] = (length, length, pc.twin_priority(pc.make_td(kind, length, 40)), 512, None)
    ext = np.tile(np.asarray([2.0 ** -25, 1.0], f32), 32)
    cs["u_extremes_len65537"] = (65537, 65537, pc.twin_priority(pc.make_td("random", 65537, 50)), 64, ext)
    cs["u_extremes_tail"] = (512, 300, pc.twin_priority(pc.make_td("random", 300, 51)), 64, ext)
    cs["u_extremes_chunk_edge"] = (257, 257, pc.twin_priority(pc.make_td("chunk_edge", 257, 52)), 64, ext)
    return cs


def refresh_cases():
    return {
        "n2_m1": pc.make_refresh_case(40, 2, 1, 1),
        "n4_m64": pc.make_refresh_case(300, 4, 64, 2),
        "n2_m257": pc.make_refresh_case(100, 2, 257, 3),
        "n4_m16640": pc.make_refresh_case(5000, 4, 16640, 4),
        "duplicates": pc.make_refresh_case(300, 4, 64, 5, dup=True),
        "out_of_range": pc.make_refresh_case(300, 4, 64, 6, out_of_range=True),
        "all_equal": pc.make_refresh_case(300, 2, 64, 7, equal=True),
        "done_all": pc.make_refresh_case(300, 4, 64, 8, done_all=True),
    }


SEED, COUNTER = 0x1234567890ABCDEF, 77

PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_prb.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_sample = 0, n_refresh = 0;
  rd(in, &n_sample, 4); rd(in, &n_refresh, 4);
  for (int c = 0; c < n_sample; ++c) {
    int32_t capacity, len, M, forced;
    rd(in, &capacity, 4); rd(in, &len, 4); rd(in, &M, 4); rd(in, &forced, 4);
    std::vector<float> leaves((size_t)capacity, 0.0f), u((size_t)M);
    std::vector<uint32_t> words((size_t)M);
    rd(in, leaves.data(), 4 * (size_t)len);
    rd(in, words.data(), 4 * (size_t)M);
    rd(in, u.data(), 4 * (size_t)M);
    int n[PRB_MAX_LEVELS + 1];
    const int L = prb_level_sizes(capacity, n);
    n[L] = 1;
    std::vector<std::vector<float>> sum(L + 1), mn(L + 1);
    sum[0] = leaves; mn[0] = leaves;
    for (int k = 0; k < L; ++k) {
      sum[k + 1].resize(n[k + 1]); mn[k + 1].resize(n[k + 1]);
      for (int w = 0; w < n[k + 1]; ++w) {
        // (prb_node reads only entries below `valid`)
        prb_node(sum[k].data(), k == 0 ? len : n[k], w, &sum[k + 1][w], &mn[k + 1][w]);
        float s2, m2;
        prb_node(mn[k].data(), k == 0 ? len : n[k], w, &s2, &m2);
        mn[k + 1][w] = m2;
      }
    }
    const int32_t L32 = L;
    fwrite(&L32, 4, 1, out);
    for (int k = 1; k <= L; ++k) { fwrite(sum[k].data(), 4, sum[k].size(), out); fwrite(mn[k].data(), 4, mn[k].size(), out); }
    PrbLevels lv;
    lv.n_levels = L;
    for (int k = 0; k < L; ++k) lv.sum[k] = sum[k].data();
    const float total = sum[L][0];
    for (int m = 0; m < M; ++m) {
      const float um = forced ? u[m] : prb_uniform(words[m]);
      const float mass = um * total;
      const int32_t idx = prb_descend(lv, len, mass);
      fwrite(&idx, 4, 1, out); fwrite(&mass, 4, 1, out);
    }
  }
  for (int c = 0; c < n_refresh; ++c) {
    int32_t F, N, M;
    float td_gamma;
    rd(in, &F, 4); rd(in, &N, 4); rd(in, &M, 4); rd(in, &td_gamma, 4);
    std::vector<float> reward((size_t)F * N), done((size_t)F), v((size_t)M), vn((size_t)M), x((size_t)M, NAN), td((size_t)M, NAN);
    std::vector<int32_t> index((size_t)M);
    rd(in, reward.data(), 4 * reward.size()); rd(in, done.data(), 4 * done.size()); rd(in, index.data(), 4 * index.size());
    rd(in, v.data(), 4 * v.size()); rd(in, vn.data(), 4 * vn.size());
    float lo = INFINITY, hi = -INFINITY;
    for (int m = 0; m < M; ++m) {
      const int f = index[m];
      if (f < 0 || f >= F) continue;
      x[m] = prb_x(reward.data() + (size_t)f * N, N, done[f], v[m], vn[m], td_gamma);
      lo = x[m] < lo ? x[m] : lo; hi = x[m] > hi ? x[m] : hi;
    }
    for (int m = 0; m < M; ++m)
      if (index[m] >= 0 && index[m] < F) td[m] = prb_norm(x[m], lo, hi);
    fwrite(x.data(), 4, x.size(), out); fwrite(td.data(), 4, td.size(), out);
  }
  fclose(in); fclose(out);
  printf("ok %%d %%d cases\n", (int)n_sample, (int)n_refresh);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    """every case through the header compiled alone"""
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("prb_header")
    sc, rc = sample_cases(), refresh_cases()
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<ii", len(sc), len(rc)))
        for capacity, length, leaves, M, u in sc.values():
            f.write(struct.pack("<iiii", capacity, length, M, int(u is not None)))
            f.write(np.ascontiguousarray(leaves, f32).tobytes())
            f.write(pc.ph.rng_u32(SEED, COUNTER, np.arange(M, dtype=np.uint32), np.uint32(0), pc.DRAW).astype(np.uint32).tobytes())
            f.write((np.zeros(M, f32) if u is None else np.ascontiguousarray(u, f32)).tobytes())
        for case in rc.values():
            F, N = case["reward"].shape
            f.write(struct.pack("<iiif", F, N, case["index"].size, float(case["td_gamma"])))
            for k in ("reward", "done", "index", "v", "vn"):
                f.write(np.ascontiguousarray(case[k]).tobytes())
    stdout = host_program.build_and_run(tmp, "prb_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(sc)} {len(rc)} cases" in stdout
    raw = np.fromfile(tmp / "out.bin", np.uint32)
    at, res_s, res_r = 0, {}, {}
    for name, (capacity, length, leaves, M, u) in sc.items():
        n = pc.level_sizes(capacity) + [1]
        assert raw[at] == len(n) - 1
        at += 1
        sums, mins = [], []
        for k in range(1, len(n)):
            sums.append(raw[at:at + n[k]].view(f32))
            mins.append(raw[at + n[k]:at + 2 * n[k]].view(f32))
            at += 2 * n[k]
        im = raw[at:at + 2 * M].reshape(M, 2)
        at += 2 * M
        res_s[name] = {"sum": sums, "min": mins, "index": im[:, 0].view(np.int32).astype(np.int64), "mass": im[:, 1].copy().view(f32)}
    for name, case in rc.items():
        M = case["index"].size
        res_r[name] = (raw[at:at + M].view(f32), raw[at + M:at + 2 * M].view(f32))
        at += 2 * M
    assert at == raw.size
    return sc, res_s, rc, res_r


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def twin_sample(case, defect=None):
    capacity, length, leaves, M, u = case
    lv = pc.build(leaves, length, capacity)
    idx, mass, uu = pc.sample(lv, length, SEED, COUNTER, M, u=u, defect=defect)
    return lv, idx, mass, uu


@pytest.mark.parametrize("name", list(sample_cases()))
def test_header_levels_and_indices_equal_the_twin_and_are_admissible(header_results, name):
    sc, res, _, _ = header_results
    capacity, length, leaves, M, u = sc[name]
    got = res[name]
    lv, idx, mass, uu = twin_sample(sc[name])
    assert np.all((got["index"] >= 0) & (got["index"] < length))
    if name.startswith("nan_leaf"):
        return  # (the index is in [0, len): nothing else is asserted)
    want_s, want_m = lv["sum"][1:] + [np.asarray([lv["total"]], f32)], lv["min"][1:] + [np.asarray([lv["q_min"]], f32)]
    assert len(want_s) == len(got["sum"])
    for k in range(len(want_s)):
        assert np.array_equal(bits(got["sum"][k]), bits(want_s[k])), (name, "sum", k + 1)
        assert np.array_equal(bits(got["min"][k]), bits(want_m[k])), (name, "min", k + 1)
    assert np.array_equal(bits(got["mass"]), bits(mass)) and np.array_equal(got["index"], idx)
    ok = pc.admissible(leaves, length, got["index"], uu, lv["total"], len(lv["n"]))
    assert ok.all(), (name, np.flatnonzero(~ok)[:8])
    assert float(lv["q_min"]) == float(np.min(leaves[:length]))  # exact in any order
    assert abs(float(lv["total"]) - float(np.sum(leaves[:length].astype(np.float64)))) <= pc.rounding_count(len(lv["n"])) * float(np.spacing(lv["total"])) / 2


def test_the_u_extremes_land_on_the_first_and_the_last_filled_leaf(header_results):
    sc, res, _, _ = header_results
    for name in ("u_extremes_len65537", "u_extremes_tail", "u_extremes_chunk_edge"):
        length, idx = sc[name][1], res[name]["index"]
        assert np.all(idx[0::2] == 0) and np.all(idx[1::2] == length - 1), name


@pytest.mark.parametrize("name", list(refresh_cases()))
def test_header_x_and_td_equal_the_twin_and_hold_the_fp64_bounds(header_results, name):
    _, _, rc, res = header_results
    case, (x, td) = rc[name], res[name]
    tx, ttd = pc.twin_refresh(case)
    assert np.array_equal(bits(x), bits(tx)) and np.array_equal(bits(td), bits(ttd))
    rx, rtd = pc.ref_refresh(case)
    ok = ~np.isnan(rx)
    assert np.array_equal(ok, (case["index"] >= 0) & (case["index"] < case["len"]))
    assert np.all(np.abs(x[ok] - rx[ok]) <= pc.x_bound(case)[ok]) and np.all(np.abs(td[ok] - rtd[ok]) <= pc.td_bound(case, rx)[ok])
    if name == "all_equal":  # the range floor acts: every td is the clamp's lower end
        assert np.all(td[ok] == f32(1e-3))
    if name == "out_of_range":
        assert (~ok).sum() == 2


def test_distribution_of_the_fixed_seed():
    """len 8, priorities 1 .. 8, M = 65536: every leaf's count within 5 binomial standard deviations of M q_f / total -- a fixed generator: a fact, not a chance"""
    q = np.arange(1, 9, dtype=f32)
    lv = pc.build(q, 8)
    assert float(lv["total"]) == 36.0 and float(lv["q_min"]) == 1.0
    M = 65536
    idx, _, _ = pc.sample(lv, 8, SEED, COUNTER, M)
    counts = np.bincount(idx, minlength=8)
    p = q.astype(np.float64) / 36.0
    sd = np.sqrt(M * p * (1 - p))
    print(counts, (counts - M * p) / sd)
    assert np.all(np.abs(counts - M * p) <= 5 * sd)


def _sampling_bars(case, defect):
    capacity, length, leaves, M, u = case
    lv, idx, mass, uu = twin_sample(case, defect)
    inside = bool(np.all((idx >= 0) & (idx < length)))
    return inside and bool(pc.admissible(leaves, length, idx, uu, lv["total"], len(lv["n"])).all())


def _refresh_bars(case, defect):
    """True when every bar holds: x and td within their float64 bounds, the priorities of td and the weights within POW_HOST_ULP, weight <= 1"""
    x, td = pc.twin_refresh(case, defect)
    rx, rtd = pc.ref_refresh(case)
    ok = ~np.isnan(rx)
    good = np.all(np.abs(x[ok] - rx[ok]) <= pc.x_bound(case)[ok]) and np.all(np.abs(td[ok] - rtd[ok]) <= pc.td_bound(case, rx)[ok])
    q = pc.twin_priority(td[ok], defect=defect)
    good = good and np.all(pc.ulp_of(q, pc.ref_priority(td[ok])) <= pc.POW_HOST_ULP)
    sound_q = pc.twin_priority(td[ok])
    w = pc.twin_weight(sound_q, sound_q.min(), defect=defect)
    good = good and np.all(pc.ulp_of(w, pc.ref_weight(sound_q, sound_q.min())) <= pc.POW_HOST_ULP) and np.all(w <= 1.0)
    return bool(good)


@pytest.mark.parametrize("defect", pc.DEFECTS)
def test_every_planted_defect_misses_a_bar(defect):
    """the sound twin is inside every bar on every case; the defective twin misses one on at least one case"""
    if defect in ("upper_bound", "no_clamp", "r_not_reduced"):
        sc = sample_cases()
        names = [n for n in sc if not n.startswith("nan_leaf") and sc[n][1] <= 65537 and ("len65536" not in n)]
        assert all(_sampling_bars(sc[n], None) for n in names)
        missed = [n for n in names if not _sampling_bars(sc[n], defect)]
    else:
        rc = refresh_cases()
        names = [n for n in rc if n != "n4_m16640"]
        assert all(_refresh_bars(rc[n], None) for n in names)
        missed = [n for n in names if not _refresh_bars(rc[n], defect)]
    print(defect, missed)
    assert missed, defect
