"""The input gradient's yardstick (tests/input_grad_check.py) on the host: a numpy float32 twin of the DX instantiation of the delta kernel -- one chain over
f = 0, 1, .., 255 per element, every product rounded separately, the padded columns zero -- passes layer 1 at every shape tests/test_gpu_input_grad.py runs on the
device and layer 2 where the references are cheap; the planted defects fail layer 1; the bound's carried term E_0 is needed (a case whose g_0 comes out of a
cancelling sum misses the bound without it); the transposed packed form at layer-0 shapes is held slot by slot to its reference; the entry points are declared and
bound.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import gradient_check as gc
import host_program
import input_grad_check as igc
import test_gpu_mlp32_grad as base
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sigmarl_amd", "csrc")
F32 = np.float32

EDGES = [[K, 256, 1] for K in (1, 31, 32, 33)]  # the column-tile edges
ODD, ACTOR, CRITIC, WIDE, WIDEST = [35, 256, 256, 32], [32, 256, 256, 256, 4], [512, 256, 256, 256, 1], [600, 256, 256, 256, 1], [4096, 256, 1]
ROWS = [0, 1, 63, 64, 65, 130]
CASES = [(d, r) for d in EDGES + [ODD, ACTOR, CRITIC, WIDE] for r in ROWS] + [(WIDEST, 65)]
DEFECTS = ["short_chain", "g1_for_g0", "untransposed", "tile0_column", "drop_last_row"]


def forward_twin(mlp, x):
    """acts [n - 1, rows, 256] in float32: what the saving forward writes, up to the summation order."""
    a, acts = x, []
    for m in gc.linears(mlp)[:-1]:
        a = np.tanh((a @ m.weight.detach().numpy().T + m.bias.detach().numpy()).astype(F32)).astype(F32)
        acts.append(a)
    return np.stack(acts)


def chain(g, w, depth=None):
    """[rows, K]: per element one chain over f = 0, 1, .. (``depth`` terms) from zero, the product rounded, then the sum."""
    part = np.zeros((g.shape[0], w.shape[1]), F32)
    for f in range(w.shape[0] if depth is None else depth):
        part = part + g[:, f:f + 1] * w[f:f + 1, :]
    return part


def dx_twin(weights, acts, dout, defect=None):
    n, rows = len(weights), dout.shape[0]
    g = dout.astype(F32).reshape(rows, weights[-1].shape[0])
    for l in range(n - 1, 0, -1):
        acc = chain(g, weights[l])
        v = (1.0 - acts[l - 1].astype(np.float64) ** 2).astype(F32)  # fma(-a, a, 1): one rounding
        g = acc if (defect == "g1_for_g0" and l == 1) else acc * v
    w0 = weights[0]
    K = w0.shape[1]
    wp = np.zeros((256, (K + 31) // 32 * 32), F32)  # K padded to the column tile: zeros
    wp[:, :K] = w0
    if defect == "untransposed":
        s = min(K, 256)
        wp[:s, :s] = w0[:s, :s].T
    dx = chain(g, wp, 255 if defect == "short_chain" else 256)
    assert (dx[:, K:] == 0).all()
    dx = dx[:, :K].copy()
    if defect == "tile0_column":
        dx[:, 32] = dx[:, 0]
    if defect == "drop_last_row":
        dx[rows - 1] = 0
    return dx


_cases = {}


def case(dims, rows):
    key = (tuple(dims), rows)
    if key not in _cases:
        mlp = base.make_net(dims, 1 + len(dims) + dims[0])
        x, dout = base.inputs(rows, dims)
        _cases[key] = (mlp, gc.weights_of(mlp), x, forward_twin(mlp, x), dout)
    return _cases[key]


@pytest.mark.parametrize("dims,rows", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_the_float32_twin_passes_layer_1_at_every_shape(dims, rows):
    mlp, weights, x, acts, dout = case(dims, rows)
    dx = dx_twin(weights, acts, dout)
    assert dx.shape == (rows, dims[0])
    r = igc.check_dx(weights, x, acts, dout, dx, what=f"twin {dims} rows={rows}")
    if rows > 12:  # (inputs: dout[11] = 0 -- no term at all, held with ==)
        assert (dx[11] == 0).all() and (igc.dx64(weights, x, acts, dout)[1][11] == 0).all()
    print(dims, rows, r["ratio"])


@pytest.mark.parametrize("dims", [[33, 256, 1], ODD, ACTOR], ids=lambda v: "x".join(map(str, v)))
def test_the_float32_twin_passes_layer_2(dims):
    mlp, weights, x, acts, dout = case(dims, 65)
    r = igc.measure_end_to_end(dx_twin(weights, acts, dout), *igc.references(mlp, x, dout))
    print(dims, r["ratio"])
    assert r["ok"], r
    # the float64 restatement is what torch's autograd computes
    m64 = [torch.from_numpy(x).double()]
    with torch.no_grad():
        for q in gc.linears(mlp)[:-1]:
            m64.append(torch.tanh(torch.nn.functional.linear(m64[-1], q.weight.double(), q.bias.double())))
    ref, _ = igc.dx64([w.astype(np.float64) for w in weights], x, [t.numpy() for t in m64[1:]], dout)
    r64, _, scale = igc.references(mlp, x, dout)
    assert np.abs(ref - r64).max() <= 1e-12 * scale


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_fail(defect):
    mlp, weights, x, acts, dout = case(ODD, 65)  # 35 columns: a second column tile; 65 rows: a second row tile of one row
    assert igc.measure_dx(weights, x, acts, dout, dx_twin(weights, acts, dout))["ok"]
    r = igc.measure_dx(weights, x, acts, dout, dx_twin(weights, acts, dout, defect))
    print(defect, r)
    assert not r["ok"], f"{defect} passes the layer-1 bound: {r}"


def test_the_carried_bound_is_needed():
    """E_0 not carried: the bound is then 257 roundings of S = |g_0| @ |W_0| alone.  Where g_0 comes out of a sum that cancels -- three outputs whose rows of W_1
    nearly cancel under this dout -- its absolute error is that of the sum's terms, far above ulp32 of g_0 itself, and it is that error times |W_0| that dX carries:
    the sound twin misses the bound without E_0 and meets the full one.  The first input row is scaled so that it has near-saturated units (|a| > 0.999), whose
    g_0 is small but no less exact: the need comes from the cancellation, in saturated and unsaturated units alike."""
    dims, rows = [33, 256, 3], 65
    mlp = base.make_net(dims, 9)
    rng = np.random.default_rng(4)
    d = np.array([0.7310586, -1.2345679, 0.4567891], F32)
    with torch.no_grad():
        w1 = gc.linears(mlp)[1].weight
        w = w1.numpy().astype(np.float64)
        w[2] = -(d[0] * w[0] + d[1] * w[1]) / np.float64(d[2]) * (1.0 + 1e-5 * rng.standard_normal(256))
        w1.copy_(torch.from_numpy(w.astype(F32)))
    x = base.inputs(rows, dims)[0]
    x[0] *= 40.0
    acts = forward_twin(mlp, x)
    assert (np.abs(acts[0][0]) > 0.999).any() and (np.abs(acts[0][0]) < 0.9).any()
    dout = np.tile(d, (rows, 1)).astype(F32)
    weights = gc.weights_of(mlp)
    dx = dx_twin(weights, acts, dout)
    assert igc.measure_dx(weights, x, acts, dout, dx)["ok"]
    b = gc.backward64(weights, x, acts, dout)
    s = np.abs(b["g"][0]) @ np.abs(weights[0].astype(np.float64))
    no_carry = gc.worst_ratio(dx, b["g"][0] @ weights[0].astype(np.float64), gc.C1 * igc.COUNT * (gc.ulp32(s) + gc.TINY))
    print("error / bound without E_0:", no_carry)
    assert no_carry > 1.0


def test_input_grad_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ("mlp32_create_input_grad", "mlp32_input_grad_workspace", "mlp32_input_grad", "mlp32_backward_dx"):
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY
        assert f"int sigmaenv_{name}(" in header
    src = open(os.path.join(CSRC, "sigmaenv_grad.inc")).read()
    assert "template <bool DX>" in src and "__launch_bounds__(256, 2) sigmaenv_mlp32_delta_kernel" in src


PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define SIGMA_HD static inline
#include "sigmaenv_pack.h"
#include "weight_pack_reference.h"

int main() {
  const int F = MLP32_H, Ks[] = {1, 31, 32, 33, 600};
  long slots = 0, bad = 0;
  uint32_t x = 2463534242u;
  for (int K : Ks) {
    std::vector<float> w((size_t)F * K);
    for (auto& v : w) { x = x * 1664525u + 1013904223u; v = (float)(x >> 8) / 8388608.0f - 1.0f; }
    w[0] = -0.0f; w[w.size() - 1] = 1e-40f;
    const std::vector<float> a = ref::exact_t_pack_ref(w.data(), F, K);
    const int Kp = (K + 31) / 32 * 32;
    if ((int)a.size() != load_exact_t_slots(F, K) || (int)a.size() != Kp * F) { printf("SIZE K=%d\n", K); ++bad; continue; }
    std::vector<float> b(a.size(), 7.0f);
    for (int d = 0; d < (int)b.size(); ++d) pack_mlp32_t_slot(w.data(), b.data(), F, K, d);
    for (size_t i = 0; i < a.size(); ++i)
      if (std::memcmp(&a[i], &b[i], 4) != 0 && ++bad <= 20) printf("MISMATCH K=%d slot %zu\n", K, i);
    /* the layout the DX contraction reads: tile kt = k / 32 at float4 kt * 32 * 64, k block fq, lane (mm, hh), component u: W_0[8 fq + 2 u + hh][32 kt + mm] */
    for (int k = 0; k < Kp; ++k)
      for (int f = 0; f < F; ++f) {
        const float got = b[((((size_t)(k >> 5) * 32 + (f >> 3)) * 2 + (f & 1)) * 32 + (k & 31)) * 4 + ((f & 7) >> 1)], want = k < K ? w[(size_t)f * K + k] : 0.0f;
        if (std::memcmp(&got, &want, 4) != 0 && ++bad <= 20) printf("LAYOUT K=%d f=%d k=%d\n", K, f, k);
      }
    slots += (long)a.size();
  }
  printf("%ld slots compared: %ld mismatches\n", slots, bad);
  return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(host_program.compiler() is None, reason="no host C++ compiler")
def test_layer_0_transposed_form_is_the_reference_packers_slot_by_slot(tmp_path):
    """pack_mlp32_t_slot at F = 256, K in {1, 31, 32, 33, 600} -- layer 0's shapes, K padded to the 32-wide column tile -- against the frozen transposed packer of
    tests/weight_pack_reference.h, every slot, padding (zeros) included; -0 and a subnormal are planted (words are compared)."""
    out = host_program.build_and_run(tmp_path, "t0_check", PROGRAM)
    assert ": 0 mismatches" in out
