"""The precision yardstick of the on-device networks (sigmaenv_mlp32_* in both modes, sigmaenv_actor): a plain helper module, imported by the tests.

fp32 kernels (``check``): the reference is the same ``torch.nn`` module in fp64 on the CPU, applied to the fp32 inputs widened to fp64.  What the reference
computes in its own precision -- the module in fp32 on the CPU -- has an error against fp64 too; that error is the yardstick.  A kernel passes when

    max|got - ref64|  <= A * max|t32 - ref64|  + B * ulp32(S)
    mean|got - ref64| <= A * mean|t32 - ref64| + B * ulp32(S)

with S the largest |b| + sum_k |w_k h_k| of the output layer (h: its inputs, fp64): the magnitude at which that layer's fp32 dot products round.  An output can be
far smaller than its terms, and on a case of a few outputs the fp32 forward's own error can be near zero by chance: the B term keeps such a case from
failing an fp32 forward in another summation order.  So a kernel passes when its error is of the class of such a forward (tests/test_network_check.py
shows that, and which defects the criterion catches).

bf16 kernel (``emulated_bf16``): a restatement of what it computes -- bf16 inputs, weights and hidden activations, fp32 accumulation -- in numpy; the tests
hold the kernel to it with their own tolerances (the matrix cores' summation order differs); tests/bf16_actor_check.py holds it bit for bit where that order cannot matter."""
from __future__ import annotations

import atexit
import copy
import json
import os

import numpy as np
import torch

A = 4.0  # times the fp32 forward's own error against fp64
B = 3.0  # ulps of S, the output layer's largest |b| + sum |w h|

# every check() of the process, for the report of worst ratios (NETWORK_CHECK_REPORT=path: written as JSON lines at exit)
RECORDS: list[dict] = []


def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def references(mlp: torch.nn.Module, x: np.ndarray):
    """(ref64, t32, scale): the module in fp64 and in fp32 on the CPU on the fp32 inputs ``x [rows, in_dim]``; ``scale`` = the largest |b| + sum |w h| of the
    output layer in fp64 (h: its inputs), the magnitude at which an fp32 dot product of that layer rounds."""
    x = np.ascontiguousarray(x, np.float32)
    m64 = copy.deepcopy(mlp).cpu().double()
    m32 = copy.deepcopy(mlp).cpu().float()
    last = [m for m in m64.modules() if isinstance(m, torch.nn.Linear)][-1]
    seen = {}

    def keep_input(mod, inp, out):
        seen["h"] = inp[0]

    hook = last.register_forward_hook(keep_input)
    with torch.no_grad():
        ref64 = m64(torch.from_numpy(x).double()).numpy()
        t32 = m32(torch.from_numpy(x)).numpy().astype(np.float64)
        scale = float((seen["h"].abs() @ last.weight.abs().T + last.bias.abs()).max()) if x.shape[0] else 0.0
    hook.remove()
    return ref64, t32, scale


def measure(got: np.ndarray, ref64: np.ndarray, t32: np.ndarray, scale: float, a: float = A, b: float = B) -> dict:
    """The criterion on precomputed references; ``ok`` and the two ratios error / bound (<= 1 passes)."""
    got = np.asarray(got, np.float64).reshape(ref64.shape)
    err, e32 = np.abs(got - ref64), np.abs(t32 - ref64)
    u = ulp32(scale)
    bmax, bmean = a * e32.max() + b * u, a * e32.mean() + b * u
    ratio = lambda e, bound: float(e / bound) if bound > 0 else (0.0 if e == 0 else float("inf"))  # noqa: E731
    r = dict(err_max=float(err.max()), err_mean=float(err.mean()), t32_max=float(e32.max()), t32_mean=float(e32.mean()), ulp=u,
             ratio_max=ratio(err.max(), bmax), ratio_mean=ratio(err.mean(), bmean))
    r["ok"] = bool(np.isfinite(got).all() and r["ratio_max"] <= 1.0 and r["ratio_mean"] <= 1.0)
    return r


def check(got, mlp: torch.nn.Module, x, what: str = "", a: float = A, b: float = B) -> dict:
    """Asserts the criterion for the kernel's outputs ``got [rows, out_dim]`` of ``mlp`` on ``x [rows, in_dim]`` (numpy or torch, any device)."""
    if isinstance(got, torch.Tensor):
        got = got.detach().cpu().numpy()
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    r = measure(got, *references(mlp, x), a, b)
    r["what"] = what
    RECORDS.append(r)
    assert r["ok"], f"{what}: max err {r['err_max']:.3e} (fp32 forward: {r['t32_max']:.3e}), mean err {r['err_mean']:.3e} (fp32 forward: {r['t32_mean']:.3e}), " \
                    f"ulp {r['ulp']:.2e}: ratios {r['ratio_max']:.2f} / {r['ratio_mean']:.2f} of the bound (A = {a}, B = {b})"
    return r


def _write_report():  # pragma: no cover
    path = os.environ.get("NETWORK_CHECK_REPORT")
    if path and RECORDS:
        with open(path, "a") as f:
            for r in RECORDS:
                f.write(json.dumps(r) + "\n")


atexit.register(_write_report)


# ---- the bf16 inference kernel ----------------------------------------------------------------------------------------------------
def bf16(a):
    """round-to-nearest-even fp32 -> bf16 -> fp32 (numpy)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def emulated_bf16(mlp, obs):
    """What the kernel computes: bf16 inputs / weights / hidden activations, fp32 accumulation (the summation order inside the matrix
    cores differs, hence the tolerance)."""
    lin = [m for m in mlp.modules() if isinstance(m, torch.nn.Linear)]
    x = bf16(obs)
    for k, m in enumerate(lin):
        w, b = bf16(m.weight.detach().numpy()), m.bias.detach().numpy().astype(np.float32)
        x = (x.astype(np.float64) @ w.T.astype(np.float64) + b).astype(np.float32)
        if k < 3:
            x = bf16(np.tanh(x))
    return x
