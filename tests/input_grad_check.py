"""The yardstick of the gradient with respect to the input rows (sigmaenv_mlp32_input_grad / sigmaenv_mlp32_backward_dx, the DX instantiation of the delta kernel in
sigmarl_amd/csrc/sigmaenv_grad.inc): a plain helper module on top of gradient_check.py, imported by the tests (tests/test_input_grad_check.py runs it on a numpy
float32 twin on the host, tests/test_gpu_input_grad.py on the device's tensors).  Two layers, as there.

Notation of gradient_check.py: g_0 [rows, 256] is the delta of the first layer, W_0 [256, K] the first Linear's weight, dX[r, k] = sum_f g_0[r, f] W_0[f, k].

LAYER 1 -- dX GIVEN the activations (``dx64`` / ``check_dx``).  ``gradient_check.backward64`` gives g_0 in float64 on the device's own saved ``acts`` and the bound E_0
its error carries (the device's g_0 is g_0* + e, |e| <= E_0).  The kernel runs ONE chain of fused multiply-adds over f = 0, 1, .., 255 from zero and nothing else: no
factor, no last product.  Count, by the counting rule of gradient_check.py: 1 per product (a chain that rounds its products separately, like the host twin, stays
inside) + the depth of the chain 256 = 257.  With S = |g_0| @ |W_0| (float64):

    |dX - g_0 @ W_0|  <=  C1 257 (ulp32(S) + TINY)  +  E_0 @ |W_0|.

An element with no non-zero term (S == 0: a zero row of dout, the rows of a one-row probe that are not the probe's) is compared with ==.  Nothing here is measured.

LAYER 2 -- end to end (``references`` / ``check_end_to_end``).  ``x.grad`` of ``y.backward(dout)`` against float64 torch autograd on the CPU; the fp32 CPU autograd's own
error against float64 is the yardstick, at the project's A = 4, B = 3:

    max|got - ref64| <= A max|t32 - ref64| + B ulp32(S),      mean likewise,

S the largest sum of |terms| of the tensor (float64).  INPUT_GRAD_CHECK_REPORT=path writes the worst ratio of every case as JSON at exit.  Measured on the MI355X
over the cases of tests/test_gpu_input_grad.py (the run is kept as profiles/input_grad_ratios.json):

    network (rows 1 .. 130)     worst ratio        network                        worst ratio
    1 x 256 x 1                 0.093              32 x 256^3 x 4, split handle   0.252
    31 x 256 x 1                0.250              32 x 256^3 x 4, exact handle   0.202
    32 x 256 x 1                0.331              512 x 256^3 x 1                0.265
    33 x 256 x 1                0.249              600 x 256^3 x 1                0.251
    35 x 256 x 256 x 32         0.226              4096 x 256 x 1 (65 rows)       0.277
    observation_saliency's dx, 96 rows of a rollout record, output columns 0 / 1:  0.256 / 0.257

48 cases; no ratio exceeds 1 (the worst is 0.331): A stays 4.  Layer 1's worst error / bound over the same cases is 0.015.

If a kernel that passes layer 1 exceeds ratio 1 here, the rule of gradient_check.py applies: A for this check alone is the smallest power of two at or above twice the
worst measured ratio x 4, with the measured ratios quoted here.
"""
from __future__ import annotations

import atexit
import copy
import json
import os

import numpy as np
import torch

import gradient_check as gc
import network_check

CHAIN = 256
COUNT = CHAIN + 1  # one rounding per product + the depth of the chain
E2E_A, E2E_B = gc.E2E_A, gc.E2E_B

RECORDS: list[dict] = []


def dx64(weights, x, acts, dout):
    """``(dx, bound)`` in float64: g_0 @ W_0 from ``gradient_check.backward64`` on the given activations, and every element's bound (zero where no term is non-zero)."""
    assert COUNT * gc.U < 0.005
    b = gc.backward64(weights, x, acts, dout)
    g0, e0, w0 = b["g"][0], b["bound_g"][0], np.asarray(weights[0], np.float64)
    assert g0.shape[1] == CHAIN == w0.shape[0]
    s = np.abs(g0) @ np.abs(w0)
    bound = gc.C1 * COUNT * (gc.ulp32(s) + gc.TINY) + e0 @ np.abs(w0)
    bound[s == 0] = 0.0
    return g0 @ w0, bound


def measure_dx(weights, x, acts, dout, dx) -> dict:
    ref, bound = dx64(weights, x, acts, dout)
    ratio = gc.worst_ratio(dx, ref, bound)
    return dict(ok=ratio <= 1.0, ratio=ratio)


def check_dx(weights, x, acts, dout, dx, what: str = "") -> dict:
    r = measure_dx(weights, x, acts, dout, dx)
    assert r["ok"], f"{what}: dx given the activations: error / bound {r['ratio']}"
    return r


def references(mlp: torch.nn.Module, x, dout):
    """(ref64, t32, scale): ``x.grad`` of ``y.backward(dout)`` by torch autograd on the CPU in float64 and in float32, and the largest sum of |terms| of an element."""
    x, dout = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(dout, np.float32)
    out = []
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(mlp).cpu().to(dt)
        xt = torch.from_numpy(x).to(dt).requires_grad_()
        y = m(xt)
        y.backward(torch.from_numpy(dout).to(dt).reshape(y.shape))
        out.append(xt.grad.numpy().astype(np.float64))
    m64 = copy.deepcopy(mlp).cpu().double()
    lin = gc.linears(m64)
    with torch.no_grad():
        a = [torch.from_numpy(x).double()]
        for q in lin[:-1]:
            a.append(torch.tanh(q(a[-1])))
    w = [q.weight.detach().numpy() for q in lin]
    b = gc.backward64(w, a[0].numpy(), [t.numpy() for t in a[1:]], dout)
    s = np.abs(b["g"][0]) @ np.abs(w[0])
    return out[0], out[1], float(s.max()) if s.size else 0.0


def measure_end_to_end(dx, ref64, t32, scale, a: float = E2E_A, b: float = E2E_B) -> dict:
    if ref64.size == 0:
        return dict(ok=np.asarray(dx).size == 0, ratio=0.0)
    r = network_check.measure(np.asarray(dx), ref64, t32, scale, a, b)
    return dict(ok=r["ok"], ratio=max(r["ratio_max"], r["ratio_mean"]), detail=r)


def check_end_to_end(dx, mlp: torch.nn.Module, x, dout, what: str = "", a: float = E2E_A, b: float = E2E_B, refs=None) -> dict:
    r = measure_end_to_end(dx, *(refs if refs is not None else references(mlp, x, dout)), a, b)
    RECORDS.append(dict(what=what, ratio=r["ratio"]))
    assert r["ok"], f"{what}: dx end to end (A = {a}, B = {b}): error / bound {r['ratio']}"
    return r


def _write_report():  # pragma: no cover
    path = os.environ.get("INPUT_GRAD_CHECK_REPORT")
    if path and RECORDS:
        worst = max(RECORDS, key=lambda rec: rec["ratio"])
        with open(path, "w") as f:
            json.dump(dict(A=E2E_A, B=E2E_B, cases=len(RECORDS), worst_ratio=worst["ratio"], worst_case=worst["what"], records=RECORDS), f, indent=1)
            f.write("\n")


atexit.register(_write_report)
