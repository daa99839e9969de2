"""The backward pass's yardstick (tests/gradient_check.py) on the host: a numpy float32 twin of sigmaenv_grad.inc -- the same formulas, the same tile- and
range-ordered sums, every product rounded separately -- passes both layers of the criterion, the planted defects fail it; at the four row counts where the partition
changes a narrower twin passes both layers, the one-row probes and the exact dyadic sum, and two faults of the partition that no earlier size can show fail them;
the row partition is what the header states; the transposed packed form of the weights (sigmaenv_pack.h) is held word for word to its reference.  No GPU needed."""
import copy
import os

import numpy as np
import pytest
import torch

import gradient_check as gc
import host_program
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sigmarl_amd", "csrc")
F32 = np.float32

DIMS = [35, 256, 256, 4]  # K padded (35 -> 40), a square layer, an output layer padded 4 -> 8
ROWS = 838                # len = 256: three full ranges and a short one of 70 rows, whose last row tile has 6 rows


def make_net(dims, seed):
    torch.manual_seed(seed)
    layers = []
    for l in range(len(dims) - 1):
        layers += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.Tanh()] if l + 2 < len(dims) else [])
    return torch.nn.Sequential(*layers)


def forward_twin(mlp, x):
    """(y, acts) in float32: what the saving forward writes, up to the summation order."""
    lin = gc.linears(mlp)
    a, acts = x, []
    for i, m in enumerate(lin):
        z = (a @ m.weight.detach().numpy().T + m.bias.detach().numpy()).astype(F32)
        if i + 1 < len(lin):
            a = np.tanh(z).astype(F32)
            acts.append(a)
    return z, np.stack(acts)


def backward_twin(weights, x, acts, dout, defect=None):
    """sigmaenv_grad.inc in numpy float32.  g_{l-1}: one chain over f = 0, 1, .. per element (product rounded, then added), times fl(1 - a^2) rounded once, rounded
    product.  dW: per range of ``partition`` one chain over the rows, partials added in range order.  db: even-row and odd-row chains per range.  ``defect``: one of
    the planted faults of DEFECTS."""
    n, rows = len(weights), x.shape[0]
    a = [x.astype(F32)] + [acts[l] for l in range(n - 1)]
    g = [None] * n
    g[n - 1] = dout.astype(F32).reshape(rows, -1)
    for l in range(n - 1, 0, -1):
        Wl = weights[l].T if (defect == "untransposed" and weights[l].shape[0] == weights[l].shape[1]) else weights[l]
        live = np.flatnonzero((g[l] != 0).any(1))  # (a row whose g is zero throughout adds zeros to +0: its chains are not run)
        part = np.zeros((live.size, weights[l].shape[1]), F32)
        for f in range(weights[l].shape[0]):
            part = part + g[l][live, f:f + 1] * Wl[f:f + 1, :]
        acc = np.zeros((rows, weights[l].shape[1]), F32)
        acc[live] = part
        if defect == "pad_column" and l == n - 1:  # a padded feature column of the contraction (4 -> 8) carrying a value: one more, spurious, term
            rng = np.random.default_rng(5)
            acc = acc + (np.abs(g[l]).max(1, keepdims=True) * F32(2e-3)) * rng.standard_normal((1, acc.shape[1])).astype(F32) * np.abs(Wl).max()
        v = (1.0 - a[l].astype(np.float64) ** 2).astype(F32)  # fma(-a, a, 1): one rounding
        g[l - 1] = acc if (defect == "no_dtanh" and l == 1) else acc * v
        if defect == "drop_tile":
            g[l - 1][rows // 64 * 64:] = 0
    length, nr = gc.partition(rows)
    if defect == "range_floor":  # the range length held at its floor under the cap of 64 ranges: the rows from 64 * 256 on are in no range
        length, nr = gc.MIN_RANGE, min(gc.MAX_RANGES, -(-rows // gc.MIN_RANGE))
    in_w = np.arange(nr * length) < rows  # the rows a range adds (its slots past the last row add +0: exact)
    if defect == "r_end_short" and length > gc.MIN_RANGE:  # the end of every range one row short once the length is above the floor
        in_w[np.minimum(np.arange(1, nr + 1) * length, rows) - 1] = False
    in_b = in_w.copy()
    if defect == "db_one_tile":
        in_b[64:] = False

    def ranged(t, on):  # [nr, length, width]: the rows by range, zeros where a range adds nothing
        p = np.zeros((nr * length, t.shape[1]), F32)
        n = min(rows, nr * length)
        p[:n] = t[:n]
        p[~on] = 0
        return p.reshape(nr, length, t.shape[1])

    dW, db = [], []
    for l in range(n):
        gl = g[l].copy()
        if defect == "drop_tile":
            gl[rows // 64 * 64:] = 0
        gb = gl.copy()  # (row63 is a fault of the dW chain alone)
        if defect == "row63":
            gl[100] = 0  # one row of the second tile is never added
        gw_r, gb_r, a_r = ranged(gl, in_w), ranged(gb, in_b), ranged(a[l], in_w)
        pw, even, odd = np.zeros((nr, gl.shape[1], a[l].shape[1]), F32), np.zeros((nr, gl.shape[1]), F32), np.zeros((nr, gl.shape[1]), F32)
        on = np.flatnonzero((gw_r != 0).any((1, 2)) | (gb_r != 0).any((1, 2)))  # (a range whose g is zero throughout adds zeros to +0: its partial sums are +0)
        gw_o, gb_o, a_o, pw_o, even_o, odd_o = gw_r[on], gb_r[on], a_r[on], pw[on], even[on], odd[on]
        for i in range(length if on.size else 0):  # every range's chain over its rows in order, the ranges side by side
            pw_o = pw_o + gw_o[:, i, :, None] * a_o[:, i, None, :]
            if i % 2 == 0:
                even_o = even_o + gb_o[:, i]
            else:
                odd_o = odd_o + gb_o[:, i]
        pw[on], even[on], odd[on] = pw_o, even_o, odd_o
        pw, pb = list(pw), list(even + odd)
        if defect == "missing_partial" and l == 1:
            del pw[2]
        sw, sb = np.zeros((gl.shape[1], a[l].shape[1]), F32) if not pw else pw[0], np.zeros(gl.shape[1], F32) if not pb else pb[0]
        for t in pw[1:]:
            sw = sw + t
        for t in pb[1:]:
            sb = sb + t
        dW.append(sw)
        db.append(sb)
    return dW, db, g[:-1]


DEFECTS = ["drop_tile", "row63", "no_dtanh", "untransposed", "db_one_tile", "pad_column", "missing_partial"]
# faults of the row partition that need more than 64 * 256 rows to show: planted at the thresholds below, not at ROWS
PARTITION_DEFECTS = ["range_floor", "r_end_short"]


@pytest.fixture(scope="module")
def case():
    mlp = make_net(DIMS, 3)
    rng = np.random.default_rng(7)
    x = ((rng.random((ROWS, DIMS[0])) * 2 - 1) * 1.5).astype(F32)
    x[7] = 0.0
    y, acts = forward_twin(mlp, x)
    dout = (rng.standard_normal((ROWS, DIMS[-1])) / ROWS).astype(F32)  # the scale of a mean loss
    dout[11] = 0.0
    refs = gc.references(mlp, x, dout)
    return mlp, gc.weights_of(mlp), x, acts, dout, refs


def both_layers(case, defect):
    mlp, weights, x, acts, dout, refs = case
    dW, db, g = backward_twin(weights, x, acts, dout, defect)
    l1 = gc.measure_backward(weights, x, acts, dout, dW, db, g)
    l2 = gc.measure_end_to_end([t for q in zip(dW, db) for t in q], *refs)
    return l1, l2


def test_the_partition_is_the_stated_function_of_rows():
    assert gc.partition(0) == (256, 0) and gc.partition(1) == (256, 1) and gc.partition(256) == (256, 1) and gc.partition(257) == (256, 2)
    assert gc.partition(ROWS) == (256, 4) and ROWS - 3 * 256 == 70
    assert gc.partition(64 * 256) == (256, 64) and gc.partition(64 * 256 + 1) == (320, 52)
    assert gc.partition(32 * 4096 * 16) == (32768, 64)
    for rows in (1, 63, 64, 65, 130, 200, 838, 16385, 2 ** 21, 2 ** 31 - 1):
        length, n = gc.partition(rows)
        assert length % 64 == 0 and length >= 256 and 1 <= n <= 64 and (n - 1) * length < rows <= n * length
    src = open(os.path.join(CSRC, "sigmaenv_grad.inc")).read()
    assert "#define GRAD_MIN_RANGE 256" in src and "#define GRAD_MAX_RANGES 64" in src


def test_the_float32_twin_passes_both_layers(case):
    mlp, weights, x, acts, dout, refs = case
    gc.check_acts(acts, mlp, x, what="twin")
    l1, l2 = both_layers(case, None)
    print(l1["ratios"], l2["ratios"])
    assert l1["ok"], l1["ratios"]
    assert l2["ok"], l2["ratios"]
    # the float64 restatement of the formulas is what torch's autograd computes (on the float64 module's own activations)
    m64 = copy.deepcopy(mlp).double()
    h, acts64 = torch.from_numpy(x).double(), []
    with torch.no_grad():
        for q in gc.linears(m64)[:-1]:
            h = torch.tanh(q(h))
            acts64.append(h.numpy())
    b = gc.backward64([q.weight.detach().numpy() for q in gc.linears(m64)], x, acts64, dout)
    for l in range(len(weights)):
        for got, ref, scale in ((b["dW"][l], refs[0][2 * l], refs[2][2 * l]), (b["db"][l], refs[0][2 * l + 1], refs[2][2 * l + 1])):
            assert np.abs(got - ref).max() <= 1e-12 * scale


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_fail(case, defect):
    l1, l2 = both_layers(case, defect)
    print(defect, l1["ratios"], l2["ratios"])
    assert not l1["ok"], f"{defect} passes the backward-given-the-activations bound: {l1['ratios']}"


# ---- the row counts at which the partition changes (tests/test_gpu_mlp32_grad.py runs the device there) ------------------------------------------------------
THRESHOLDS = gc.THRESHOLDS
NARROW = [35, 64, 64, 4]  # the twin's network at these sizes: 64 wide, not 256 -- the partition and every chain over the rows are functions of the row count alone
# every row count the suite ran a backward on before (host and device): one range length, at most 4 ranges
EARLIER_ROWS = (0, 1, 5, 13, 52, 63, 64, 65, 70, 130, 200, 260, 838)
_big = {}


def big(rows):
    """(mlp, weights, x, acts, dout, refs) of the narrow network on ``rows`` rows, made once"""
    if rows not in _big:
        mlp = make_net(NARROW, 4)
        rng = np.random.default_rng(rows)
        x = ((rng.random((rows, NARROW[0])) * 2 - 1) * 1.5).astype(F32)
        x[7] = 0.0
        y, acts = forward_twin(mlp, x)
        dout = (rng.standard_normal((rows, NARROW[-1])) / rows).astype(F32)
        dout[11] = 0.0
        _big[rows] = (mlp, gc.weights_of(mlp), x, acts, dout, gc.references(mlp, x, dout))
    return _big[rows]


def probe(rows, r, defect=None):
    """The one-row probe of row ``r`` on the twin: the checks of tests/test_gpu_mlp32_grad.py's hold_one_row_probes; returns the small products per layer"""
    mlp, weights, x, acts, _, _ = big(rows)
    dout = np.zeros((rows, NARROW[-1]), F32)
    rng = np.random.default_rng(r)
    dout[r] = rng.uniform(0.5, 1.5, NARROW[-1]) * rng.choice([-1.0, 1.0], NARROW[-1])
    dW, db, g = backward_twin(weights, x, acts, dout, defect)
    assert all(np.count_nonzero(t) == np.count_nonzero(t[r]) > 0 for t in g)
    g_rows, a_rows = [t[r] for t in g] + [dout[r]], [x[r]] + [t[r] for t in acts]
    return [gc.check_one_row(rows, g_rows[l], a_rows[l], dW[l], db[l], what=f"twin rows={rows} probe {r} layer {l}") for l in range(len(weights))]


def dyadic(rows, defect=None):
    """(db of the output layer, the float64 sum of dout) for a dout of multiples of 2^-10 below 1 in magnitude: every partial sum in any order is exact"""
    mlp, weights, x, acts, _, _ = big(rows)
    dout = (np.random.default_rng(rows).integers(-1023, 1024, (rows, NARROW[-1])) / 1024.0).astype(F32)
    assert np.abs(dout.astype(np.float64)).sum(0).max() < 2.0 ** 14
    return backward_twin(weights, x, acts, dout, defect)[1][-1].astype(np.float64), dout.astype(np.float64).sum(0)


def test_the_thresholds_are_where_the_partition_changes():
    for rows, (length, n, last) in THRESHOLDS.items():
        assert gc.partition(rows) == (length, n) and rows - (n - 1) * length == last
        assert len(set(gc.probe_rows(rows))) == 8 and all(0 <= r < rows for r in gc.probe_rows(rows))
    assert all(gc.partition(r) == (256, -(-r // 256)) and -(-r // 256) <= 4 for r in EARLIER_ROWS)


@pytest.mark.parametrize("rows", list(THRESHOLDS))
def test_the_float32_twin_passes_every_check_at_the_thresholds(rows):
    mlp, weights, x, acts, dout, refs = big(rows)
    gc.check_acts(acts, mlp, x, what=f"twin rows={rows}")
    l1, l2 = both_layers(big(rows), None)
    print(rows, l1["ratios"], l2["ratios"])
    assert l1["ok"] and l2["ok"], (l1["ratios"], l2["ratios"])
    small = np.sum([probe(rows, r) for r in gc.probe_rows(rows)], 0)
    print(rows, "products below 2^-120 per layer:", list(small))
    assert small[-1] == 0
    got, want = dyadic(rows)
    assert np.array_equal(got, want)


def fails(f, *args):
    try:
        f(*args)
    except AssertionError:
        return True
    return False


def test_partition_defects_pass_the_earlier_sizes_and_fail_at_the_thresholds(case):
    """range_floor is the gap the thresholds close: below 64 * 256 + 1 rows it IS the partition, so at every size the suite had it gives the sound twin's bits; one row
    further it drops rows, which the last row's probe, the dyadic sum and (from 20480 rows) the bound see.  r_end_short needs a range above the floor length."""
    mlp, weights, x, acts, dout, refs = case
    assert ROWS == max(EARLIER_ROWS)
    for defect in PARTITION_DEFECTS:
        for a, b in zip(backward_twin(weights, x, acts, dout, defect), backward_twin(weights, x, acts, dout)):
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
        assert all(m["ok"] for m in both_layers(case, defect))
    caught = {}
    for defect in PARTITION_DEFECTS:
        for rows, (length, n, last) in THRESHOLDS.items():
            l1 = both_layers(big(rows), defect)[0]
            got, want = dyadic(rows, defect)
            caught[defect, rows] = dict(bound=not l1["ok"], probes=[r for r in gc.probe_rows(rows) if fails(probe, rows, r, defect)], dyadic=not np.array_equal(got, want))
            print(defect, rows, caught[defect, rows], {k: round(v, 3) for k, v in l1["ratios"].items() if k.startswith("d")})
    nothing = dict(bound=False, probes=[], dyadic=False)
    assert caught["range_floor", 16384] == nothing and caught["r_end_short", 16384] == nothing  # (64 ranges of the floor length: neither fault changes anything)
    assert caught["range_floor", 16385]["probes"] == [16384] and caught["range_floor", 16385]["dyadic"]   # the one row past 64 * 256
    assert caught["range_floor", 20480]["bound"] and caught["range_floor", 20481]["bound"] and caught["range_floor", 20481]["probes"] == [r for r in gc.probe_rows(20481) if r >= 16384]
    for rows in (16385, 20480, 20481):
        length, n = gc.partition(rows)
        assert caught["r_end_short", rows]["probes"] == [r for r in gc.probe_rows(rows) if (r + 1) % length == 0 or r == rows - 1] and caught["r_end_short", rows]["dyadic"]


def test_zero_rows_and_zero_dout_rows():
    mlp = make_net([7, 256, 1], 2)
    w = gc.weights_of(mlp)
    b = gc.backward64(w, np.zeros((0, 7), F32), np.zeros((1, 0, 256), F32), np.zeros((0, 1), F32))
    assert all((t == 0).all() for t in b["dW"] + b["db"] + b["bound_dW"] + b["bound_db"])
    assert gc.worst_ratio(np.zeros((256, 7)), b["dW"][0], b["bound_dW"][0]) == 0.0
    assert gc.worst_ratio(np.full((256, 7), 1e-30), b["dW"][0], b["bound_dW"][0]) == float("inf")
    rng = np.random.default_rng(1)
    x = rng.standard_normal((5, 7)).astype(F32)
    _, acts = forward_twin(mlp, x)
    dout = rng.standard_normal((5, 1)).astype(F32)
    dout[2] = 0
    b = gc.backward64(w, x, acts, dout)
    assert (b["g"][0][2] == 0).all() and (b["bound_g"][0][2] == 0).all()


def test_grad_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ("mlp32_forward_save", "mlp32_backward_workspace", "mlp32_backward"):
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY
        assert f"int sigmaenv_{name}(" in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "sigmaenv_grad.inc" in [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()  # sigmaenv_build_id() covers the kernels
    assert '#include "sigmaenv_grad.inc"' in open(os.path.join(CSRC, "sigmaenv.hip")).read()


PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define SIGMA_HD static inline
#include "sigmaenv_pack.h"
#include "weight_pack_reference.h"

static long bad = 0;
static void same(const char* what, int F, int K, const std::vector<float>& a, const std::vector<float>& b) {
  if (a.size() != b.size()) { printf("SIZE %s F=%d K=%d: %zu against %zu\n", what, F, K, a.size(), b.size()); ++bad; return; }
  for (size_t i = 0; i < a.size(); ++i)
    if (std::memcmp(&a[i], &b[i], 4) != 0 && ++bad <= 20) printf("MISMATCH %s F=%d K=%d slot %zu\n", what, F, K, i);
}
int main() {
  const int Fs[] = {256, 32, 9, 8, 7, 4, 2, 1}, Ks[] = {256, 35, 32, 7};
  long slots = 0;
  uint32_t x = 12345u;
  for (int F : Fs)
    for (int K : Ks) {
      std::vector<float> w((size_t)F * K), wT((size_t)F * K);
      for (auto& v : w) { x = x * 1664525u + 1013904223u; v = (float)(x >> 8) / 8388608.0f - 1.0f; }
      w[0] = -0.0f; w[w.size() - 1] = 1e-40f; w[w.size() / 2] = NAN;
      for (int f = 0; f < F; ++f) for (int k = 0; k < K; ++k) wT[(size_t)k * F + f] = w[(size_t)f * K + k];
      /* 1: the reference scatter by (f, k), written from the layout */
      const std::vector<float> a = ref::exact_t_pack_ref(w.data(), F, K);
      /* 2: the product's per-slot function, as sigmaenv_mlp32_create and the device pack kernel call it, one destination slot at a time */
      std::vector<float> b((size_t)load_exact_t_slots(F, K), 7.0f);
      for (int d = 0; d < (int)b.size(); ++d) pack_mlp32_t_slot(w.data(), b.data(), F, K, d);
      /* every weight lands in exactly one slot */
      std::vector<int> seen((size_t)F * K, 0);
      for (int d = 0; d < (int)b.size(); ++d) { const int s = load_exact_t_src(F, K, d); if (s >= (int)seen.size()) { ++bad; continue; } if (s >= 0) ++seen[s]; }
      for (int c : seen) if (c != 1) { if (++bad <= 20) printf("COVER F=%d K=%d: a weight packed %d times\n", F, K, c); }
      /* 3: the forward's exact form (held to the reference by tests/test_weight_load_host.py) of the transposed matrix [K][F] */
      std::vector<float> c((size_t)load_exact_slots(K, F));
      for (int d = 0; d < (int)c.size(); ++d) { const int s = load_exact_src(K, F, d); c[d] = s >= 0 ? wT[s] : 0.0f; }
      same("reference-vs-product", F, K, a, b);
      same("transposed-vs-exact-of-transpose", F, K, b, c);
      slots += (long)a.size();
    }
  printf("%ld slots compared: %ld mismatches\n", slots, bad);
  return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(host_program.compiler() is None, reason="no host C++ compiler")
def test_transposed_form_packers_agree_word_for_word(tmp_path):
    """F in {256, 32, 9, 8, 7, 4, 2, 1} x K in {256, 35, 32, 7}: the per-slot function of sigmaenv_pack.h that sigmaenv_mlp32_create loops over on the host and the
    device pack kernel on the device, the reference scatter by (f, k) of tests/weight_pack_reference.h, and the forward's exact form of the transposed matrix give the
    same words in every slot, padding (zeros) included; every weight lands in exactly one slot.  -0, a subnormal and a NaN are planted (words are compared)."""
    out = host_program.build_and_run(tmp_path, "t_check", PROGRAM)
    assert ": 0 mismatches" in out
