#!/usr/bin/env python
"""What a snapshot of an env handle costs (``SigmaEnv.snapshot`` / ``restore``: sigmaenv_state_save / _restore, ONE launch each) at 16 agents x 4096 envs and
4 agents x 32768 envs on the CPM map:
  save            every segment packed into the blob
  restore         the whole blob back
  restore_third   the masked form, every third env selected
  copy_chain      the alternative the kernel replaces for the unmasked case: the bytes of the 21 ``sigmaenv_get`` buffers moved by one device-to-device copy each
                  (``Tensor.copy_`` between contiguous tensors of one dtype: a hipMemcpyAsync per buffer; the few bytes per env ``sigmaenv_get`` does not reach --
                  reset_mask, reset_full -- are left out, in the chain's favour)
  step            one fused step with its resets (``step_autoreset``), for scale
Device time from events on the env's stream: after WARMUP untimed calls of every route, SAMPLES samples per route, the routes alternating; one sample = the event time
around BATCH back-to-back calls / BATCH; the median, the minimum and the maximum over the samples are reported, and the bytes moved over the median as GB/s (read +
write: twice the blob).  A report; no test asserts a time.  Writes the table to the file named on the command line (default profiles/snapshot_timing.txt) and
prints it."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd.env import SigmaEnv, _buf_layout  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

WARMUP, SAMPLES, BATCH = int(os.environ.get("WARMUP", 5)), int(os.environ.get("SAMPLES", 21)), int(os.environ.get("BATCH", 20))
SHAPES = [(16, 4096), (4, 32768)]


def measure(N, B):
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                              max_steps=128), n_envs=B, device="cuda:0")
    env.reset_random(seed=3)
    g = torch.Generator(device="cuda").manual_seed(6)
    act = torch.stack([torch.rand(B, N, generator=g, device="cuda"), torch.rand(B, N, generator=g, device="cuda") - 0.5], -1).contiguous()
    for t in range(4):
        env.step_autoreset(act, seed=5, counter=t)
    snap = env.snapshot()
    third = torch.zeros(B, dtype=torch.uint8, device="cuda")
    third[0::3] = 1
    views = [env.buffer(w).reshape(-1) for w in _buf_layout(env.B, env.N, env.K, env.D)]
    copies = [torch.empty_like(v) for v in views]
    chain_bytes = sum(v.numel() * v.element_size() for v in views)
    counter = [100]

    def chain():
        for dst, src in zip(copies, views):
            dst.copy_(src)

    def step():
        counter[0] += 1
        env.step_autoreset(act, seed=5, counter=counter[0])

    routes = {"save": lambda: env.snapshot(out=snap), "restore": lambda: env.restore(snap), "restore_third": lambda: env.restore(snap, envs=third),
              "copy_chain": chain, "step": step}
    ms = {k: [] for k in routes}
    with torch.cuda.stream(env.stream):
        for fn in routes.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        for _ in range(SAMPLES):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(env.stream)
                for _ in range(BATCH):
                    fn()
                e1.record(env.stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / BATCH)
    total = int(snap.header["total_bytes"])
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        moved = {"save": 2 * total, "restore": 2 * total, "restore_third": 2 * total * int(third.sum()) // B, "copy_chain": 2 * chain_bytes}.get(k)
        rows.append((k, med * 1e3, min(v) * 1e3, max(v) * 1e3, f"{moved / med / 1e6:8.1f}" if moved else "       -"))
    env.close()
    return total, chain_bytes, len(views), rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "snapshot_timing.txt")
    lines = [f"tools/snapshot_timing.py on {torch.cuda.get_device_name(0)}: device time per call from events on the env's stream, microseconds;",
             f"{WARMUP} warm-up calls, {SAMPLES} samples of {BATCH} back-to-back calls per route, routes alternating; GB/s = bytes read + written over the median", ""]
    for N, B in SHAPES:
        total, chain_bytes, n_views, rows = measure(N, B)
        lines.append(f"{N} agents x {B} envs: blob {total} bytes ({total / B:.0f} per env); copy chain {chain_bytes} bytes in {n_views} copies")
        lines.append(f"  {'route':<14} {'median us':>10} {'min us':>10} {'max us':>10} {'GB/s':>8}")
        for k, med, lo, hi, rate in rows:
            lines.append(f"  {k:<14} {med:10.2f} {lo:10.2f} {hi:10.2f} {rate}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
