#!/usr/bin/env python
"""What the gradient with respect to the input costs, at the minibatch shapes of the workload (the reference's minibatch_size of 512 frames, 16 agents): the actor
32 -> 256^3 -> 4 on 8192 rows and the critic 512 -> 256^3 -> 1 on 512 rows.  Per network, the backward pass alone (the saving forward has run; dout is given):
  input_grad    sigmaenv_mlp32_input_grad: the DX delta launch alone -> dx
  backward      sigmaenv_mlp32_backward: delta launch, dW and sum kernels -> the parameters' gradients                     (what training runs today)
  backward_dx   sigmaenv_mlp32_backward_dx: the DX delta launch, the same dW and sum kernels -> both
  torch_*       torch autograd of the same fp32 module on the GPU, backward alone on a retained graph (torch.autograd.grad): x alone, the parameters alone, both
Each figure is HIP events around CALLS (default 50) consecutive calls on preallocated buffers, divided by their number; one untimed round first, then REPS (default
5) rounds with the routes alternating inside one process; best and spread are reported.  A report, not a bound: no target is set for dx.  Writes the text to the
path given (default profiles/input_grad_timing.txt) and prints it."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sigmarl_amd.actor import Mlp32, make_mlp  # noqa: E402
from sigmarl_amd.env import SigmaEnv  # noqa: E402
from sigmarl_amd.params import Parameters  # noqa: E402

REPS, CALLS = int(os.environ.get("REPS", 5)), int(os.environ.get("CALLS", 50))
N, D, FRAMES = 16, 32, int(os.environ.get("MINIBATCH", Parameters().minibatch_size))


def routes_of(env, name, dims, rows):
    torch.manual_seed(len(name))
    mod = make_mlp(dims[0], n_out=dims[-1]).cuda()
    net = Mlp32(mod, mode="exact", input_grad=True)
    lib, h, L = env.lib, net.handle(env.lib, env), len(dims) - 1
    x = (torch.rand((rows, dims[0]), device="cuda") * 2 - 1) * 1.5
    dout = torch.randn((rows, dims[-1]), device="cuda") / rows
    y, acts = net._forward_save(env, (x, 0, rows, dims[0], 1, 0, None))
    nf = C.c_uint64()
    assert lib.mlp32_backward_workspace(h, rows, C.byref(nf)) == 0
    ws, dx = torch.empty(int(nf.value), device="cuda"), torch.empty((rows, dims[0]), device="cuda")
    gw, gb = [torch.empty((dims[l + 1], dims[l]), device="cuda") for l in range(L)], [torch.empty(dims[l + 1], device="cuda") for l in range(L)]
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    PA = C.c_void_p * L
    W, B = PA(*[t.data_ptr() for t in gw]), PA(*[t.data_ptr() for t in gb])
    keep = (mod, net, x, dout, y, acts, ws, dx, gw, gb, W, B)

    def chk(rc):
        assert rc == 0, lib.last_error(env.h)

    xr = x.clone().requires_grad_()
    yt = mod(xr)
    params = list(mod.parameters())
    return {
        "input_grad": (env.stream, lambda: chk(lib.mlp32_input_grad(env.h, h, p(acts), p(dout), rows, p(ws), p(dx)))),
        "backward": (env.stream, lambda: chk(lib.mlp32_backward(env.h, h, p(x), rows, dims[0], 1, 0, p(acts), p(dout), p(ws), W, B))),
        "backward_dx": (env.stream, lambda: chk(lib.mlp32_backward_dx(env.h, h, p(x), rows, dims[0], 1, 0, None, 0, 0, 0, p(acts), p(dout), p(ws), W, B, p(dx)))),
        "torch_x": (None, lambda: torch.autograd.grad(yt, [xr], dout, retain_graph=True)),
        "torch_params": (None, lambda: torch.autograd.grad(yt, params, dout, retain_graph=True)),
        "torch_x_and_params": (None, lambda: torch.autograd.grad(yt, [xr] + params, dout, retain_graph=True)),
    }, keep


def ms_per_call(stream, call):
    stream = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(CALLS):
        call()
    e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) / CALLS


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "input_grad_timing.txt")
    env = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=8, device="cuda:0")
    lines = [f"backward pass alone, ms per call: HIP events around {CALLS} consecutive calls, best of {REPS} rounds (spread = worst - best), routes alternating; "
             f"{torch.cuda.get_device_name(0)}"]
    kept = []
    for name, dims, rows in (("actor", [D, 256, 256, 256, 4], FRAMES * N), ("critic", [N * D, 256, 256, 256, 1], FRAMES)):
        routes, keep = routes_of(env, name, dims, rows)
        kept.append(keep)
        for stream, call in routes.values():  # untimed: allocations, code loading
            ms_per_call(stream, call)
        t = {r: [] for r in routes}
        for _ in range(REPS):
            for r, (stream, call) in routes.items():
                t[r].append(ms_per_call(stream, call))
        lines.append(f"{name} {'x'.join(map(str, dims))}, {rows} rows")
        for r, v in t.items():
            lines.append(f"  {r:20s} {min(v):9.4f}   spread {max(v) - min(v):8.4f}")
        lines.append(f"  dx on top of today's backward (backward_dx - backward): {min(t['backward_dx']) - min(t['backward']):.4f} ms")
    text = "\n".join(lines)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)
    for keep in kept:
        keep[1].close()
    env.close()


if __name__ == "__main__":
    main()
