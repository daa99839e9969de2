#!/usr/bin/env python
"""Diagnostic: per-phase shader-clock cycles of the wave-per-tile step kernel.  Needs the profile build
(make -C sigmarl_amd/csrc prof; SIGMAENV_LIB is set here) -- the product library carries no stamps."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SIGMAENV_TIMESTAMPS"] = "1"
os.environ.setdefault("SIGMAENV_LIB", os.path.join(ROOT, "sigmarl_amd", "csrc", "libsigmaenv_prof.so"))
import numpy as np, torch
from sigmarl_amd.env import SigmaEnv
from sigmarl_amd.params import Parameters
B, N = int(os.environ.get("B", 4096)), int(os.environ.get("N", 16))
scen = os.environ.get("SCENARIO", "cpm_entire")
import json
extra = json.loads(os.environ.get("PARAMS", "{}"))  # e.g. PARAMS='{"is_ego_view": false}': the non-default observation rows
env = SigmaEnv(Parameters(**dict(dict(n_agents=N, scenario_type=scen, is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), **extra)), n_envs=B, device="cuda:0")
env.reset_random(seed=1)
acts = torch.rand((B, N, 2), device="cuda") * torch.tensor([1.0, 0.5], device="cuda") - torch.tensor([0.0, 0.25], device="cuda")
pf, pc = env.map.list_first[0], env.map.list_count[0]
f = env.lib.cdll.sigmaenv_debug_timestamps
f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
def stamp_rows():
    env.sync()
    rows = np.zeros((B, 16), np.uint64)
    return rows[:f(env.h, rows.ctypes.data_as(C.c_void_p), B)]
# T=1 (default): 20 launches of one step, the accumulated words read back after every launch (per tile-step figures); T=k: one launch of k steps after the same
# 20 single ones -- the stamps are then those of its last step, the accumulated words those of all its steps
T = int(os.environ.get("T", 1))
edge_steps = []  # per launch: (list entries, overflowed tile-steps) of every tile
item_steps = []  # per single-step launch: the work-list items of every tile (one value per tile-step)
prev = stamp_rows()[:, 8:10] >> np.uint64(32)
prev_items = stamp_rows()[:, 8] & np.uint64(0xFFFFFFFF)
for t in range(20):
    env.step_autoreset(acts, seed=1, counter=t, path_first=pf, path_count=pc)
    if T == 1:
        rows_t = stamp_rows()
        cur = rows_t[:, 8:10] >> np.uint64(32)
        edge_steps.append((cur - prev).astype(np.int64))
        prev = cur
        cur_items = rows_t[:, 8] & np.uint64(0xFFFFFFFF)
        item_steps.append((cur_items - prev_items).astype(np.int64))
        prev_items = cur_items
n_steps = 20
if T > 1:
    prev = stamp_rows()[:, 8:10] >> np.uint64(32)
    env.step_autoreset_n(acts.unsqueeze(0).expand(T, B, N, 2).contiguous(), None, seed=1, counter0=20, path_first=pf, path_count=pc)
    edge_steps.append(((stamp_rows()[:, 8:10] >> np.uint64(32)) - prev).astype(np.int64))
    n_steps += T
ts = stamp_rows()
n = len(ts)
sub = ts[:n, [1, 10, 11, 2]].astype(np.int64)  # scan: start, end of S1 (candidate masks), end of S2 (work-list rounds), end (S3)
stats = (ts[:n, 8:10] & np.uint64(0xFFFFFFFF)).astype(np.int64)  # (the upper halves: phase E's list statistics, read above)
lvl = (ts[:n, 12:16] & np.uint64(0xFFFFFFFF)).astype(np.int64)
passes = (ts[:n, 12:14] >> np.uint64(32)).astype(np.int64)  # (the upper halves of words 12 / 13: phase E's tile-steps with a second pass / with an entry taken from the map; all launches)
ts = ts[:n, :8].astype(np.int64)
ts = ts[ts[:, 0] > 0]
d = np.diff(ts, axis=1)
names = ["A dynamics", "S scan", "E edges", "B1 pairs", "C reward", "D obs+slab", "R resets"]
print("tiles", len(ts), "(shader-clock cycles per tile and phase; the clocks of different XCDs are not comparable, only differences within a tile)")
for k, nm in enumerate(names):
    print(f"{nm:12s} mean {d[:, k].mean():9.0f}  p10 {np.percentile(d[:, k], 10):9.0f}  p90 {np.percentile(d[:, k], 90):9.0f}")
print("tile total mean", (ts[:, 7] - ts[:, 0]).mean())
if stats[:, 1].sum():  # accumulated over the launches above
    per = stats[:, 0] / np.maximum(stats[:, 1], 1)
    print("scan work list: items per tile-step mean %.1f p10 %.0f p50 %.0f p90 %.0f max %.0f; rounds per step %.2f" % (per.mean(), np.percentile(per, 10), np.percentile(per, 50), np.percentile(per, 90), per.max(), stats[:, 1].sum() / (float(n_steps) * len(stats))))
if item_steps:  # T = 1: the distribution over tile-steps (above: over the tiles' means), and the S2 passes of 64 lanes it takes (the third one starts at 129 items)
    it = np.concatenate(item_steps)
    print("scan work list per tile-step: items mean %.1f p10 %.0f p50 %.0f p90 %.0f max %.0f; tile-steps with more than 128 items %d of %d (%.2f %%), with more than 64 %d (%.2f %%)" % (
        it.mean(), np.percentile(it, 10), np.percentile(it, 50), np.percentile(it, 90), it.max(), (it > 128).sum(), len(it), 100.0 * (it > 128).mean(), (it > 64).sum(), 100.0 * (it > 64).mean()))
if edge_steps and sum(int(e[:, 0].sum()) for e in edge_steps):
    ent = np.concatenate([e[:, 0] for e in edge_steps]) / float(T)  # T = 1: one value per tile-step; T > 1: per tile, the mean over the launch's steps
    print("edge list (%s): entries per tile-step mean %.1f p50 %.0f p99 %.0f max %.0f; overflowed tile-steps %d of %d" % (
        "per tile-step" if T == 1 else "per tile, mean of the %d-step launch" % T, ent.mean(), np.percentile(ent, 50), np.percentile(ent, 99), ent.max(),
        sum(int(e[:, 1].sum()) for e in edge_steps), len(ent) * T))
    print("edge passes (all %d steps): tile-steps with a second pass of 64 lanes %d of %d (%.3f %%), with an entry beyond the coordinate capacity (segment from the map) %d of %d (%.3f %%)" % (
        n_steps, passes[:, 0].sum(), n_steps * n, 100.0 * passes[:, 0].sum() / (n_steps * n), passes[:, 1].sum(), n_steps * n, 100.0 * passes[:, 1].sum() / (n_steps * n)))

sub = sub[(sub[:, 0] > 0) & (sub[:, 1] > 0)]
if len(sub):
    print("scan split: S1 candidate masks %.0f, S2 work-list rounds %.0f, S3 results %.0f" % ((sub[:, 1] - sub[:, 0]).mean(), (sub[:, 2] - sub[:, 1]).mean(), (sub[:, 3] - sub[:, 2]).mean()))
if lvl.sum():
    steps = np.maximum(stats[:, 1], 1)
    print("scan neighbour levels: tasks beyond the near level per tile-step %.2f, tile-steps with such a task %.3f, tasks at the tight level per tile-step %.1f" % ((lvl[:, 0] / steps).mean(), (lvl[:, 1] / steps).mean(), (lvl[:, 2] / steps).mean()))
    print("  of those: the first agent's (stale corner queries) %.2f per tile-step" % ((lvl[:, 3] / steps).mean()))
