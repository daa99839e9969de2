#!/usr/bin/env python
"""What putting a learner's updated parameters back into the device networks costs, one MI355X: the actor 32 -> 256^3 -> 4 (fp32 forms; with BF16=1 also the bf16
handle) and the critic 512 -> 256^3 -> 1, by two routes from the same CUDA parameters
  load      Actor.load / Critic.load: one pack launch per layer on the env's stream, in place, the 4-byte range word read back (sigmaenv_load.inc)
  recreate  the only route before it: parameters .cpu(), the scalar host packers in a new Actor / Critic (about 16 hipMalloc + hipMemcpy), close() of the old one
Wall clock around a stream synchronisation on both sides (the recreate route is host work: events would not see it), the routes alternating, REPS (default 3)
repetitions after one untimed call of each.  A report, not a pass criterion.  Prints one JSON line and writes it to profiles/weight_refresh_timing.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd.actor import Actor, Critic, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

REPS = int(os.environ.get("REPS", 3))
PRECISION = "bf16" if os.environ.get("BF16") == "1" else "fp32"
LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]

torch.manual_seed(0)
env = SigmaEnv(Parameters(n_agents=16, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=64, device="cuda:0")
env.reset_random(seed=1)
assert env.D == 32
mods = {"actor": make_mlp(32).cuda(), "critic": make_mlp(16 * 32, n_out=1).cuda()}
make = {"actor": lambda m: Actor(m, LOW, HIGH, precision=PRECISION), "critic": lambda m: Critic(m)}
nets = {k: make[k](m) for k, m in mods.items()}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def load(k):
    nets[k].load(env, mods[k])


def recreate(k):
    old = nets[k]
    nets[k] = make[k](mods[k])
    old.close()


res = {"reps": REPS, "actor_precision": PRECISION, "weights": {k: sum(p.numel() for p in m.parameters()) for k, m in mods.items()}, "ms": {}}
for k in mods:
    load(k)
    recreate(k)
    out = {"load": [], "recreate": []}
    for _ in range(REPS):
        with torch.no_grad():  # (new numbers every time, as after an optimiser step)
            for p in mods[k].parameters():
                p.mul_(0.999)
        out["load"].append(wall_ms(lambda: load(k)))
        out["recreate"].append(wall_ms(lambda: recreate(k)))
    res["ms"][k] = out
res["ms_min_total"] = {r: sum(min(res["ms"][k][r]) for k in mods) for r in ("load", "recreate")}
for n in nets.values():
    n.close()
env.close()
line = json.dumps(res)
print(line)
out_dir = os.environ.get("OUT_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "weight_refresh_timing.json"), "w") as f:
    f.write(line + "\n")
