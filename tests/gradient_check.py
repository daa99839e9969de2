"""The yardstick of the fp32 network's backward pass (sigmaenv_mlp32_forward_save / sigmaenv_mlp32_backward, sigmarl_amd/csrc/sigmaenv_grad.inc): a plain helper
module like network_check.py, imported by the tests (tests/test_gradient_check.py runs it on a numpy float32 twin on the host, tests/test_gpu_mlp32_grad.py on the
device's tensors).  Two layers, so that what can be derived is derived.

Notation: layers l = 0 .. n - 1, z_l = W_l a_l + b_l, a_{l+1} = tanh(z_l) for l < n - 1, a_0 the input rows; acts[l] = a_{l+1}; g_{n-1} = dout and
    g_{l-1} = (g_l W_l) (.) (1 - a_l^2),     dW_l = g_l^T a_l,     db_l = sum_rows g_l.

LAYER 1 -- the backward GIVEN the activations (``backward64`` / ``check_backward``).  The three formulas in float64 on the device's own saved ``acts``, its fp32
weights, inputs and ``dout``, all widened exactly.  Against that the only errors are the roundings of products and sums, so the bound of every element is a COUNT of
roundings times ulp32 of that element's sum of |terms| S (float64), plus what the error of the g above it carries in.  One rounding to nearest of a value v costs at
most u |v|, u = 2^-24, and u S <= ulp32(S) (S < 2^(e+1) gives 2^-24 S < 2^(e-23) = ulp32(S)); every partial sum of a chain is at most S in magnitude.  C1 = 1.01
covers the second-order terms (asserted: count * u < 0.005), and each count also multiplies 2^-149 for results below the normal range.

  g_{l-1}[r, k]   terms t_f = g_l[r, f] W_l[f, k] (1 - a^2), f < F_l (the padded features are exact zeros and adding +0 is exact).  The kernel runs ONE chain of fused
      multiply-adds over f = 0, 1, .. from 0 (v_mfma_f32_32x32x2_f32), multiplies by fl(1 - a^2) formed with one rounding (fma(-a, a, 1): relative error u, also where
      |a| -> 1) and rounds the product.  Count: 1 per product (a chain that rounds its products separately, like the host twin, stays inside; an fma spends none) + the
      depth of the chain F_l + the factor 1 + the last product 1:     F_l + 3.
  dW_l[f, k]     terms g_l[r, f] a_l[r, k] over the rows.  The rows are cut into ranges (``partition``: len = max(256, ceil(rows / 64) rounded up to a multiple of 64));
      per range one chain over its rows in order, then the partial sums are added in range order.  Count: 1 per product + the longest chain min(len, rows) + the
      n_ranges - 1 additions:     min(len, rows) + n_ranges.
  db_l[f]        terms g_l[r, f], no product.  Per range one chain of additions over its even rows and one over its odd rows, added (+1), then the ranges in order:
      ceil(min(len, rows) / 2) + 1 + n_ranges - 1.
  carried in     the device's g_l is g_l* + e_l, |e_l| <= E_l (E_{n-1} = 0: dout is given).  Everything below is linear in g_l:
      E_{l-1} = C1 count ulp32(S) + (E_l |W_l|) (.) (1 - a^2);    dW_l gets + E_l^T |a_l|;    db_l gets + sum_rows E_l.
  An element whose bound is zero (rows = 0, all-zero columns) is compared with ==.

LAYER 2 -- the saved activations and the gradients end to end.  ``check_acts``: every saved layer is held to the float64 module truncated after that layer with
``network_check.check`` at the project's A = 4, B = 3 (the forward's outputs pass through these layers under that criterion already).  ``check_end_to_end``: the full
gradients (``y.backward(dout)``) against float64 torch autograd on the CPU, in the same form: the fp32 CPU autograd's own error against float64 is the yardstick,

    max|got - ref64| <= A max|t32 - ref64| + B ulp32(S),      mean likewise,

S the tensor's largest sum of |terms| (float64).  E2E_A = 4 and E2E_B = 3, the project's values.  If a kernel that passes layer 1 exceeds ratio 1 here the cause is
the device tanh (<= ~4 ulp, mlp32_tanh, against torch's 1 ulp) amplified through 1 - a^2 where |a| -> 1; A for this check alone is then the smallest power of two at or
above twice the worst measured ratio x 4, with the measured ratios quoted here.  Measured on the MI355X (GRADIENT_CHECK_REPORT=path writes the worst ratio per tensor
and every case; the run is kept as profiles/gradient_check_ratios.json), worst ratio per tensor over the networks of tests/test_gpu_mlp32_grad.py:

    rows            cases   dW0    db0    dW1    db1    dW2    db2    dW3    db3
    1 .. 838          42    0.421  0.403  0.393  0.273  0.366  0.510  0.360  0.101
    16384 .. 20481     8    0.069  0.034  0.074  0.035  0.062  0.039  0.049  0.015

No ratio exceeds 1: A stays 4.  (The large row counts sit lower because the fp32 autograd's own error, the yardstick, grows with the length of its sums while the
device's ranged chains stay short; the largest ratios are single rows.)

ONE-ROW PROBES (``check_one_row``, ``probe_rows``).  At the row counts where the partition changes a lost or doubled row moves an element by about S / rows, no more
than a few times the layer-1 bound (count ~ 372 at 16385 rows).  So there the partition is also held exactly: with dout zero in every row but one, every chain is
zeros plus one term, and dW / db must be that term.
"""
from __future__ import annotations

import atexit
import copy
import json
import os

import numpy as np
import torch

import network_check

U = 2.0 ** -24
C1 = 1.01
TINY = 2.0 ** -149
E2E_A, E2E_B = 4.0, 3.0

MIN_RANGE, MAX_RANGES = 256, 64

# rows -> (range length, ranges, rows of the last range): the four row counts at which the partition changes -- the cap of 64 ranges reached with the floor length,
# the first length above the floor (a short tail), the cap reached above the floor, the next length
THRESHOLDS = {16384: (256, 64, 256), 16385: (320, 52, 65), 20480: (320, 64, 320), 20481: (384, 54, 129)}

RECORDS: list[dict] = []  # every check_end_to_end of the process (GRADIENT_CHECK_REPORT=path: the worst ratios per tensor, written as JSON at exit)


def partition(rows: int):
    """(len, n_ranges) of the dW kernel's row partition (sigmaenv_grad.inc, grad::range_len): a function of ``rows`` alone."""
    per = (-(-rows // MAX_RANGES) + 63) // 64 * 64
    length = max(per, MIN_RANGE)
    return length, (-(-rows // length) if rows > 0 else 0)


def counts(rows: int, F: int):
    """The rounding counts of the module docstring for a layer with ``F`` outputs: (g of the layer below, dW, db)."""
    length, n = partition(rows)
    chain = min(length, rows)
    return F + 3, chain + n, -(-chain // 2) + n


def ulp32(v: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def linears(mlp: torch.nn.Module):
    return [m for m in mlp.modules() if isinstance(m, torch.nn.Linear)]


def weights_of(mlp: torch.nn.Module):
    return [m.weight.detach().cpu().numpy().astype(np.float32) for m in linears(mlp)]


def backward64(weights, x, acts, dout):
    """The three formulas in float64 and every element's bound.  ``weights``: the fp32 ``[F, K]`` matrices; ``x [rows, K_0]``, ``acts [n - 1, rows, 256]``,
    ``dout [rows, F_last]`` fp32.  Returns ``dict(g, dW, db, bound_g, bound_dW, bound_db)``: lists over the layers (g[n - 1] = dout, its bound zero)."""
    n = len(weights)
    W = [np.asarray(w, np.float64) for w in weights]
    a = [np.asarray(x, np.float64)] + [np.asarray(acts[l], np.float64) for l in range(n - 1)]
    rows = a[0].shape[0]
    g, E = [None] * n, [None] * n
    g[n - 1] = np.asarray(dout, np.float64).reshape(rows, W[n - 1].shape[0])
    E[n - 1] = np.zeros_like(g[n - 1])
    dW, db, bW, bb = [None] * n, [None] * n, [None] * n, [None] * n
    for l in range(n - 1, -1, -1):
        cg, cw, cb = counts(rows, W[l].shape[0])
        assert max(cg, cw, cb) * U < 0.005, "C1 does not cover the second-order terms of a chain this long"
        dW[l] = g[l].T @ a[l]
        bW[l] = C1 * cw * (ulp32(np.abs(g[l]).T @ np.abs(a[l])) + TINY) + E[l].T @ np.abs(a[l])
        db[l] = g[l].sum(0)
        bb[l] = C1 * cb * (ulp32(np.abs(g[l]).sum(0)) + TINY) + E[l].sum(0)
        if rows == 0:
            bW[l], bb[l] = np.zeros_like(dW[l]), np.zeros_like(db[l])
        if l > 0:
            v = 1.0 - a[l] * a[l]
            g[l - 1] = (g[l] @ W[l]) * v
            E[l - 1] = C1 * cg * (ulp32((np.abs(g[l]) @ np.abs(W[l])) * v) + TINY) + (E[l] @ np.abs(W[l])) * v
            zero = (np.abs(g[l]) @ np.abs(W[l])) * v == 0  # no term at all (a zero row of dout): exact
            E[l - 1][zero] = 0.0
    return dict(g=g, dW=dW, db=db, bound_g=E, bound_dW=bW, bound_db=bb)


def worst_ratio(got, ref, bound) -> float:
    """max error / bound; inf where the bound is zero and the value differs (or is not finite)."""
    got, ref, bound = np.asarray(got, np.float64).reshape(ref.shape), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def measure_backward(weights, x, acts, dout, grad_w, grad_b, g=None) -> dict:
    """Layer 1 on precomputed tensors: ``ok`` and the worst error / bound of every tensor (``g``: the device's g_l, l < n - 1, optional)."""
    ref = backward64(weights, x, acts, dout)
    ratios = {}
    for l in range(len(weights)):
        ratios[f"dW{l}"] = worst_ratio(grad_w[l], ref["dW"][l], ref["bound_dW"][l])
        ratios[f"db{l}"] = worst_ratio(grad_b[l], ref["db"][l], ref["bound_db"][l])
        if g is not None and l < len(weights) - 1:
            ratios[f"g{l}"] = worst_ratio(g[l], ref["g"][l], ref["bound_g"][l])
    return dict(ok=all(r <= 1.0 for r in ratios.values()), ratios=ratios)


def check_backward(weights, x, acts, dout, grad_w, grad_b, g=None, what: str = "") -> dict:
    r = measure_backward(weights, x, acts, dout, grad_w, grad_b, g)
    assert r["ok"], f"{what}: backward given the activations: error / bound {r['ratios']}"
    return r


SMALL = 2.0 ** -120  # a product below this may lie under the fp32 normal range once the matrix instruction has formed it: held to the bound, not to ==


def check_one_row(rows: int, g_row, a_row, grad_w, grad_b, what: str = "") -> int:
    """One layer of a backward whose g is zero in every row but one (``g_row [F]``, ``a_row [K]``: that row of the device's g_l and a_l, ``rows`` the row count of
    the call): every chain is zeros plus one term, so ``db[f] == g_row[f]`` and ``dW[f, k] == fl32(g_row[f] a_row[k])`` -- the product of two fp32 values is exact in
    float64 and is rounded once -- as values (+0 and -0 alike; a NaN equals nothing).  A row that is lost leaves zeros, one that is added twice -- in a range or in
    two -- doubles the element.  A non-zero product below SMALL in magnitude is held to the layer-1 bound of its one-term sum instead; their number is returned."""
    g64, a64 = np.asarray(g_row, np.float64).reshape(-1), np.asarray(a_row, np.float64).reshape(-1)
    dW, db = np.asarray(grad_w, np.float32).reshape(g64.size, a64.size), np.asarray(grad_b, np.float32).reshape(g64.size)
    want = g64[:, None] * a64[None, :]
    small = (want != 0) & (np.abs(want) < SMALL)
    bad = ~small & ~(dW == want.astype(np.float32))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements of dW are not the one product, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{dW[bad][0]!r} against {want.astype(np.float32)[bad][0]!r}"
    bound = C1 * counts(rows, g64.size)[1] * (ulp32(want) + TINY)
    assert (np.abs(dW.astype(np.float64) - want)[small] <= bound[small]).all(), f"{what}: a product below 2^-120 misses the layer-1 bound"
    bad = ~(db == g64.astype(np.float32))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements of db are not the row's g, first at {int(np.argwhere(bad)[0][0])}"
    return int(small.sum())


def probe_rows(rows: int):
    """The rows of the one-row probes: the first and the last row, and the rows on either side of the first, a middle and the last boundary between two ranges"""
    length, n = partition(rows)
    return [0, rows - 1] + [k * length - j for k in sorted({1, n // 2, n - 1}) for j in (1, 0)]


def truncated(mlp: torch.nn.Module, l: int) -> torch.nn.Sequential:
    """The module up to and including the Tanh after Linear ``l``."""
    lin = linears(mlp)
    mods = []
    for m in lin[: l + 1]:
        mods += [copy.deepcopy(m), torch.nn.Tanh()]
    return torch.nn.Sequential(*mods)


def check_acts(acts, mlp: torch.nn.Module, x, what: str = "") -> list:
    """Layer 2, first half: every saved layer against the float64 truncated module (network_check.check, A = 4, B = 3)."""
    return [network_check.check(np.asarray(acts[l]), truncated(mlp, l), x, what=f"{what} acts[{l}]") for l in range(len(linears(mlp)) - 1)]


def references(mlp: torch.nn.Module, x, dout):
    """(ref64, t32, scales): the gradients of ``y.backward(dout)`` by torch autograd on the CPU in float64 and in float32 (lists [dW_0, db_0, dW_1, ..]) and every
    tensor's largest sum of |terms| from the float64 pass."""
    x, dout = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(dout, np.float32)
    out = []
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(mlp).cpu().to(dt)
        for p in m.parameters():
            p.grad = None
        y = m(torch.from_numpy(x).to(dt))
        y.backward(torch.from_numpy(dout).to(dt).reshape(y.shape))
        out.append([t.grad.numpy().astype(np.float64) for q in linears(m) for t in (q.weight, q.bias)])
    m64 = copy.deepcopy(mlp).cpu().double()
    lin = linears(m64)
    with torch.no_grad():
        a = [torch.from_numpy(x).double()]
        for q in lin[:-1]:
            a.append(torch.tanh(q(a[-1])))
    b = backward64([q.weight.detach().numpy() for q in lin], a[0].numpy(), [t.numpy() for t in a[1:]], dout)
    scales = []
    for l in range(len(lin)):
        ga, al = np.abs(b["g"][l]), np.abs(a[l].numpy())
        scales += [float((ga.T @ al).max()) if x.shape[0] else 0.0, float(ga.sum(0).max()) if x.shape[0] else 0.0]
    return out[0], out[1], scales


def measure_end_to_end(grads, ref64, t32, scales, a: float = E2E_A, b: float = E2E_B) -> dict:
    names = [f"{k}{l}" for l in range(len(ref64) // 2) for k in ("dW", "db")]
    res = {nm: network_check.measure(np.asarray(got), r, t, s, a, b) for nm, got, r, t, s in zip(names, grads, ref64, t32, scales)}
    return dict(ok=all(r["ok"] for r in res.values()), ratios={nm: max(r["ratio_max"], r["ratio_mean"]) for nm, r in res.items()}, detail=res)


def check_end_to_end(grads, mlp: torch.nn.Module, x, dout, what: str = "", a: float = E2E_A, b: float = E2E_B, refs=None) -> dict:
    """Layer 2, second half: ``grads`` = [dW_0, db_0, dW_1, ..] against float64 autograd, the fp32 autograd's own error as the yardstick."""
    r = measure_end_to_end(grads, *(refs if refs is not None else references(mlp, x, dout)), a, b)
    RECORDS.append(dict(what=what, ratios=r["ratios"]))
    assert r["ok"], f"{what}: gradients end to end (A = {a}, B = {b}): error / bound {r['ratios']}"
    return r


def _write_report():  # pragma: no cover
    path = os.environ.get("GRADIENT_CHECK_REPORT")
    if path and RECORDS:
        worst = {}
        for rec in RECORDS:
            for nm, v in rec["ratios"].items():
                if v > worst.get(nm, (-1.0, ""))[0]:
                    worst[nm] = (v, rec["what"])
        with open(path, "w") as f:
            json.dump(dict(A=E2E_A, B=E2E_B, cases=len(RECORDS), worst_ratio_per_tensor={k: dict(ratio=v[0], case=v[1]) for k, v in sorted(worst.items())},
                           records=RECORDS), f, indent=1)
            f.write("\n")


atexit.register(_write_report)
