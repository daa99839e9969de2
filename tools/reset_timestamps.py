#!/usr/bin/env python
"""Diagnostic: per-phase shader-clock cycles of the device-side resets (needs SIGMAENV_TIMESTAMPS=2 and the profile build).

Default: the stand-alone auto-reset kernel's active workgroups after 20 x (step; auto_reset).
FUSED=1: the step kernel's fused resets (phase R, auto_reset_tile's wavefront form; one tile per workgroup) -- T=1 (default): 20 single-step launches, every
reset a complete one; T=k: ONE launch of k steps on a fresh batch, where the last reset of most tiles is a mid-launch one (`fin == false`).  A row holds the stamps of the tile's LAST reset: start (1), candidates in registers (7), accept loop done (8),
rows placed (9), end of the sampler + placement (2), and for a complete reset the pair distances / env tail (5) and the observation (6).  A library without the
stamps 7..9 (an older profile build) reports the sampler + placement total only."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SIGMAENV_TIMESTAMPS"] = "2"
os.environ.setdefault("SIGMAENV_LIB", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigmarl_amd", "csrc", "libsigmaenv_prof.so"))  # profile build (make -C sigmarl_amd/csrc prof)
import numpy as np, torch
from sigmarl_amd.env import SigmaEnv
from sigmarl_amd.params import Parameters
B, N = int(os.environ.get("B", 4096)), int(os.environ.get("N", 16))
FUSED, T = int(os.environ.get("FUSED", 0)), int(os.environ.get("T", 1))
env = SigmaEnv(Parameters(n_agents=N, scenario_type=os.environ.get("SCENARIO", "cpm_entire"), is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=B, device="cuda:0")
env.reset_random(seed=1)
acts = torch.rand((B, N, 2), device="cuda") * torch.tensor([1.0, 0.5], device="cuda") - torch.tensor([0.0, 0.25], device="cuda")
pf, pc = env.map.list_first[0], env.map.list_count[0]
if FUSED and T > 1:
    env.step_autoreset_n(acts.unsqueeze(0).expand(T, B, N, 2).contiguous(), None, seed=1, counter0=0, path_first=pf, path_count=pc)
elif FUSED:
    for t in range(20):
        env.step_autoreset(acts, seed=1, counter=t, path_first=pf, path_count=pc)
else:
    for t in range(20):
        env.step(acts); env.auto_reset(seed=1)
env.sync()
f = env.lib.cdll.sigmaenv_debug_timestamps
f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
ts = np.zeros((B, 16), np.uint64)
n = f(env.h, ts.ctypes.data_as(C.c_void_p), B)
ts = ts[:n].astype(np.int64)


def line(nm, d):
    print(f"{nm:34s} mean {d.mean():9.0f}  p10 {np.percentile(d, 10):9.0f}  p50 {np.percentile(d, 50):9.0f}  p90 {np.percentile(d, 90):9.0f}")


def core(a):
    """The sampler + placement of the rows `a`, split at the stamps 7 .. 9 where the library has them."""
    line("sampler + placement (1 -> 2)", a[:, 2] - a[:, 1])
    if (a[:, 7] > 0).all() and (a[:, 8] > 0).all() and (a[:, 9] > 0).all():
        for a0, a1, nm in ((1, 7, "  candidates in registers"), (7, 8, "  accept loop"), (8, 9, "  rows placed"), (9, 2, "  fence + barrier")):
            line(nm, a[:, a1] - a[:, a0])


if FUSED:
    act = (ts[:, 1] > 0) & (ts[:, 2] > 0)
    print(f"fused resets of the step kernel, N={N} B={B} T={T}: tiles {n}, with a reset {int(act.sum())}")
    a = ts[act]
    core(a)
    if T == 1:  # (T > 1: the stamps 5 / 6 of most rows are older than the row's last reset, which was a mid-launch one)
        line("pair distances + env tail (2 -> 5)", a[:, 5] - a[:, 2])
        line("observation (5 -> 6)", a[:, 6] - a[:, 5])
    sys.exit(0)
act = ts[:, 6] > 0
print("workgroups", n, "active", int(act.sum()))
t0 = ts[:, 0].min()
print("start spread (all wgs)", ts[:, 0].max() - t0, " last end", ts[act, 6].max() - t0)
a = ts[act]
for a0, a1, nm in ((0, 1, "flags + state load"), (1, 2, "sampler + placement"), (2, 5, "pair distances + env tail"), (5, 6, "observation")):
    d = a[:, a1] - a[:, a0]
    print(f"{nm:28s} mean {d.mean():9.0f}  p10 {np.percentile(d, 10):9.0f}  p90 {np.percentile(d, 90):9.0f}")
core(a)
print("active wg total mean", (a[:, 6] - a[:, 0]).mean())
