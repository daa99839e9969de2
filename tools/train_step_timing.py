#!/usr/bin/env python
"""What differentiating the device networks costs (Mlp32.apply: sigmaenv_mlp32_forward_save + sigmaenv_mlp32_backward), at the collect shape -- N agents x B envs,
T steps (default 16 x 4096, 32: 2.1 M actor rows, 131 072 critic rows) --, against torch autograd of the same torch.nn modules on the same device in fp32:
  actor        y = net(rows); y.backward(dout) over the root-observation record (dense [T B N, D]): Actor.apply against the torch module
  critic       the same for the critic over the root-observation record ([T B, N D])
  critic_slab  the critic over the observation part of the record rows [T, B, W] (W odd): Critic.apply reads them in place, torch needs slice + .contiguous() first
Both routes produce the parameters' .grad from the same dout; forward and backward together, allocations included (acts, workspace / autograd's saved tensors).
HIP events around each call, after CONDITION_MS (default 200) of the same work so that the device is at its sustained clocks; REPS (default 3)
repetitions with the two routes alternating inside one process.  A report, not a pass criterion.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sigmarl_amd.actor import Actor, Critic, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

B, N, T, REPS = int(os.environ.get("B", 4096)), int(os.environ.get("N", 16)), int(os.environ.get("T", 32)), int(os.environ.get("REPS", 3))
CONDITION_MS = float(os.environ.get("CONDITION_MS", 200))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def condition(fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < CONDITION_MS:
        fn()
        torch.cuda.synchronize()


def compare(routes: dict) -> dict:
    """ms of every route, REPS times, the routes alternating; conditioned on the first."""
    for fn in routes.values():  # (first calls: allocations, kernel loads)
        fn()
    torch.cuda.synchronize()
    condition(next(iter(routes.values())))
    out = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            out[k].append(timed(fn))
    return out


torch.manual_seed(0)
env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False, is_obs_noise=False,
                          max_steps=128), n_envs=B, device="cuda:0")
env.reset_random(seed=1)
D, W = env.D, N * (env.D + 1) + 1
amod, cmod = make_mlp(D).cuda(), make_mlp(N * D, n_out=1).cuda()
actor, critic = Actor(amod, low=[-1.0, -0.6], high=[1.0, 0.6]), Critic(cmod)
kw = dict(dtype=torch.float32, device="cuda")
slab, rec = torch.empty((T, B, W), **kw), torch.empty((T, B, N, D), **kw)
actor.rollout(env, T, slab=slab, obs_rec=rec, seed=1, counter0=0)  # real records
env.sync()
da, dc = torch.randn((T * B * N, 4), **kw) / (T * B * N), torch.randn((T, B), **kw) / (T * B)
res = {"n_agents": N, "n_envs": B, "steps": T, "actor_rows": T * B * N, "critic_rows": T * B, "reps": REPS, "condition_ms": CONDITION_MS, "ms": {}}


def zero():
    for p in list(amod.parameters()) + list(cmod.parameters()):
        p.grad = None


def actor_device():
    zero()
    actor.apply(env, rows=(rec, 0, T * B * N, D, 1, 0)).view(T * B * N, 4).backward(da)


def actor_torch():
    zero()
    amod(rec.view(T * B * N, D)).backward(da)


def critic_device(record):
    zero()
    critic.apply(env, record, T=T).backward(dc)


def critic_torch(x):
    zero()
    cmod(x.reshape(T * B, N * D)).view(T, B).backward(dc)


res["ms"]["actor"] = compare({"device_apply": actor_device, "torch_autograd": actor_torch})
res["ms"]["critic"] = compare({"device_apply": lambda: critic_device(rec), "torch_autograd": lambda: critic_torch(rec)})
res["ms"]["critic_slab"] = compare({"device_apply_in_place": lambda: critic_device(slab), "slice_contiguous_torch_autograd": lambda: critic_torch(slab[:, :, : N * D].contiguous())})
res["best_ms"] = {k: {r: min(v) for r, v in d.items()} for k, d in res["ms"].items()}
flop = lambda rows, dims: 6.0 * rows * sum(a * b for a, b in zip(dims[:-1], dims[1:]))  # noqa: E731  (forward + two backward products per weight; the input gradient's share of layer 0 is not computed)
res["tflops_device"] = {"actor": flop(T * B * N, [D, 256, 256, 256, 4]) / (res["best_ms"]["actor"]["device_apply"] * 1e-3) / 1e12,
                        "critic": flop(T * B, [N * D, 256, 256, 256, 1]) / (res["best_ms"]["critic"]["device_apply"] * 1e-3) / 1e12}
actor.close()
critic.close()
env.close()
print(json.dumps(res))
