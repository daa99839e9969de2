#!/usr/bin/env python
"""What the tail of one minibatch update costs -- from the parameters' .grad to networks that hold the updated weights -- for the reference-shaped actor
(32 -> 256^3 -> 4) and critic (512 -> 256^3 -> 1), 404 229 parameters in 16 tensors, with gradients present:
  device   learn.Adam.step(max_grad_norm): sigmaenv_optim_step -- the clip over both networks in one norm, Adam, the repack of every weight form; three launches, no
           host wait (one Adam.resolve() at the end of a run of updates, as learn.update calls it)
  parent   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step + zero_grad + actor.load + critic.load: the foreach kernels, two snapshot copies, one pack launch
           per layer and form, and per network a host wait for the range word
Two figures per route.  ``event_ms``: HIP events around one call.  ``wall_ms_per_update``: the host's wall clock over a run of UPDATES (default 16) consecutive
updates without a synchronisation in between, divided by their number -- the host waits the device route removes show only here.  (Either route is handed the same
fixed gradient tensors before every call; that assignment is inside the wall-clock run of both.)  One untimed call of each route, then REPS (default 5) repetitions
with the two routes alternating inside one process.  A report, not a bound.  Writes the JSON to the path given (default profiles/optim_step_timing.json) and prints it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd import learn  # noqa: E402
from sigmarl_amd.actor import Actor, Critic, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

REPS, UPDATES = int(os.environ.get("REPS", 5)), int(os.environ.get("UPDATES", 16))
N, D, LOW, HIGH, MAX_NORM, LR = 16, 32, [-1.0, -0.6], [1.0, 0.6], 1.0, 3e-4


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "optim_step_timing.json")
    torch.manual_seed(0)
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", dt=0.05, is_use_mtv_distance=False, rew_method="distance", is_apply_mask=False,
                              is_obs_noise=False, max_steps=128), n_envs=8, device="cuda:0")
    assert env.D == D
    routes = {}
    for name in ("device", "parent"):
        amod, cmod = make_mlp(D).cuda(), make_mlp(N * D, n_out=1).cuda()
        actor, critic = Actor(amod, LOW, HIGH), Critic(cmod)
        pars = list(amod.parameters()) + list(cmod.parameters())
        grads = [torch.randn_like(p) * 1e-2 for p in pars]
        if name == "device":
            opt = learn.Adam(env, [(actor, amod), (critic, cmod)], lr=LR)

            def update(opt=opt):
                opt.step(MAX_NORM)

            finish = opt.resolve
        else:
            opt = torch.optim.Adam(pars, lr=LR)

            def update(opt=opt, pars=pars, actor=actor, critic=critic, amod=amod, cmod=cmod):
                torch.nn.utils.clip_grad_norm_(pars, MAX_NORM)
                opt.step()
                opt.zero_grad()
                actor.load(env, amod)
                critic.load(env, cmod)

            def finish():
                return None

        def give(pars=pars, grads=grads):
            for p, g in zip(pars, grads):
                p.grad = g.clone()

        routes[name] = (give, update, finish, (actor, critic))

    def event_ms(name):
        give, update, finish, _ = routes[name]
        give()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        update()
        e.record()
        torch.cuda.synchronize()
        finish()
        return s.elapsed_time(e)

    def wall_ms(name):
        give, update, finish, _ = routes[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(UPDATES):
            give()
            update()
        finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / UPDATES

    for name in routes:  # untimed: allocations, code loading
        event_ms(name)
        wall_ms(name)
    ev, wl = {n: [] for n in routes}, {n: [] for n in routes}
    for _ in range(REPS):
        for name in routes:
            ev[name].append(event_ms(name))
        for name in routes:
            wl[name].append(wall_ms(name))
    n_par = sum(p.numel() for p in list(routes["device"][3][0]._mlp32._params) + list(routes["device"][3][1]._params))
    out = {"actor": [D, 256, 256, 256, 4], "critic": [N * D, 256, 256, 256, 1], "parameters": n_par, "reps": REPS, "updates_per_wall_run": UPDATES,
           "event_ms": ev, "wall_ms_per_update": wl,
           "best": {"event_ms": {n: min(v) for n, v in ev.items()}, "wall_ms_per_update": {n: min(v) for n, v in wl.items()}},
           "spread": {"event_ms": {n: max(v) - min(v) for n, v in ev.items()}, "wall_ms_per_update": {n: max(v) - min(v) for n, v in wl.items()}}}
    text = json.dumps(out, indent=1)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)
    for _, _, _, nets in routes.values():
        for n in nets:
            n.close()
    env.close()


if __name__ == "__main__":
    main()
