"""The gradient with respect to the input rows on the device (sigmaenv_mlp32_input_grad / sigmaenv_mlp32_backward_dx, Mlp32(input_grad=True).apply,
Mlp32.input_grad, saliency.observation_saliency): every case is held to both layers of tests/input_grad_check.py -- dx given the device's own saved activations
within a derived count of roundings, and end to end against float64 autograd with the fp32 autograd's own error as the yardstick; dense rows, the same rows inside a
record, through an index and padded give the same bits, as do two runs, the two C entry points and ``loss.backward()``; sigmaenv_mlp32_backward_dx's parameter
gradients are those of the existing entry points bit for bit; layer 0's transposed form follows ``load`` and ``learn.Adam.step``.  Networks and inputs are built as
tests/test_gpu_mlp32_grad.py builds them; every workspace is exactly the floats asked for, followed by guard words."""
import copy
import ctypes as C

import numpy as np
import pytest

import gradient_check as gc
import input_grad_check as igc
import test_gpu_mlp32_grad as base
from test_gpu_mlp32_grad import GUARD, GUARD_WORD, same

pytestmark = pytest.mark.gpu

ACTOR, CRITIC, ODD, WIDE, WIDEST = base.ACTOR, base.CRITIC, base.ODD, base.WIDE, [4096, 256, 1]
EDGES = [[K, 256, 1] for K in (1, 31, 32, 33)]  # the column-tile edges
ROWS = [0, 1, 63, 64, 65, 130]                  # the row-tile edges
NETS = [(d, "split") for d in EDGES + [ODD]] + [(ACTOR, "split"), (ACTOR, "exact"), (CRITIC, "split"), (WIDE, "split")]
CASES = [(d, m, r) for d, m in NETS for r in ROWS] + [(WIDEST, "split", 65)]
IDS = dict(ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, list) else str(v))


@pytest.fixture(scope="module")
def env():
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    e = SigmaEnv(Parameters(n_agents=4, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=8, device="cuda:0")
    e.reset_random(seed=3)
    yield e
    e.close()


_nets = {}


def network(dims, mode, input_grad=True):
    """(torch module on the CPU, its copy on the device, Mlp32 made from the copy) per (dims, mode, input_grad), made once."""
    from sigmarl_amd.actor import Mlp32

    key = (tuple(dims), mode, input_grad)
    if key not in _nets:
        mlp = base.make_net(dims, 1 + len(_nets))
        dev = copy.deepcopy(mlp).cuda()
        _nets[key] = (mlp, dev, Mlp32(dev, mode=mode, input_grad=input_grad))
    return _nets[key]


def nan(*shape):
    import torch

    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def guarded(n_floats):
    """A NaN workspace of exactly ``n_floats`` followed by GUARD words of a fixed pattern"""
    import torch

    ws = nan(int(n_floats) + GUARD)
    ws[int(n_floats):].view(torch.int32).fill_(GUARD_WORD)
    return ws


def unchanged(ws, n_floats):
    import torch

    return bool((ws[int(n_floats):].view(torch.int32) == GUARD_WORD).all())


p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731


def forward_save(env, net, rec, spec, index=None, pad=None):
    """(y, acts) of the rows ``spec`` of ``rec`` (``index``: blocks of the record; ``pad``: padded rows), both starting as NaN"""
    offset, rpb, rs, nb, bs = spec
    n, L, lib, h = rpb * (nb if index is None else index.numel()), len(net._keep[1]), env.lib, net.handle(env.lib, env)
    y, acts = nan(n, net.out_dim), nan(L - 1, n, 256)
    src = C.c_void_p(rec.data_ptr() + 4 * offset)
    if index is None:
        rc = lib.mlp32_forward_save(env.h, h, src, rpb, rs, nb, bs, p(y), p(acts))
    elif pad is None:
        rc = lib.mlp32_forward_save_indexed(env.h, h, src, rpb, rs, nb, bs, p(index), index.numel(), p(y), p(acts))
    else:
        rc = lib.mlp32_forward_save_indexed_pad(env.h, h, src, rpb, rs, nb, bs, p(index), index.numel(), pad[0], pad[1], p(y), p(acts))
    assert rc == 0, lib.last_error(env.h)
    return y, acts


def c_input_grad(env, net, acts, dout):
    """sigmaenv_mlp32_input_grad: (dx, g); dx and the guarded workspace start as NaN"""
    import torch

    n, L, lib, h = acts.shape[1], len(net._keep[1]), env.lib, net.handle(env.lib, env)
    nf = C.c_uint64(77)
    assert lib.mlp32_input_grad_workspace(h, n, C.byref(nf)) == 0 and nf.value == (L - 1) * n * 256
    ws, dx, d = guarded(nf.value), nan(n, net.in_dim + 1), torch.from_numpy(np.ascontiguousarray(dout, np.float32)).cuda()
    torch.cuda.synchronize()
    rc = lib.mlp32_input_grad(env.h, h, p(acts), p(d), n, p(ws), p(dx))  # (dx: in_dim + 1 columns of NaN, of which the first n * in_dim floats are the dense dx)
    assert rc == 0, lib.last_error(env.h)
    env.sync()
    assert unchanged(ws, nf.value), "input_grad wrote past the workspace it asks for"
    flat = dx.view(-1)
    assert torch.isnan(flat[n * net.in_dim:]).all(), "input_grad wrote past dx"
    return flat[: n * net.in_dim].view(n, net.in_dim).clone(), ws[: (L - 1) * n * 256].view(L - 1, n, 256)


def c_backward_dx(env, net, rec, spec, acts, dout, index=None, pad=None):
    """sigmaenv_mlp32_backward_dx: (grad_w, grad_b, g, dx); every output and the guarded workspace start as NaN"""
    import torch

    offset, rpb, rs, nb, bs = spec
    n, L, lib, h = acts.shape[1], len(net._keep[1]), env.lib, net.handle(env.lib, env)
    dims = [int(d) for d in net._keep[0]]
    nf = C.c_uint64()
    assert lib.mlp32_backward_workspace(h, n, C.byref(nf)) == 0
    ws, dx, d = guarded(nf.value), nan(n, net.in_dim), torch.from_numpy(np.ascontiguousarray(dout, np.float32)).cuda()
    gw, gb = [nan(dims[l + 1], dims[l]) for l in range(L)], [nan(dims[l + 1]) for l in range(L)]
    PA = C.c_void_p * L
    torch.cuda.synchronize()
    rc = lib.mlp32_backward_dx(env.h, h, C.c_void_p(rec.data_ptr() + 4 * offset), rpb, rs, nb, bs, p(index), 0 if index is None else index.numel(),
                               *(pad or (0, 0)), p(acts), p(d), p(ws), PA(*[t.data_ptr() for t in gw]), PA(*[t.data_ptr() for t in gb]), p(dx))
    assert rc == 0, lib.last_error(env.h)
    env.sync()
    assert unchanged(ws, nf.value), "backward_dx wrote past the workspace it asks for"
    return gw, gb, ws[: (L - 1) * n * 256].view(L - 1, n, 256), dx


@pytest.mark.parametrize("dims,mode,rows", CASES, **IDS)
def test_dx_holds_both_layers_and_does_not_depend_on_the_row_layout(env, dims, mode, rows):
    import torch

    mlp, dev, net = network(dims, mode)
    x, dout = base.inputs(rows, dims)
    xd = torch.from_numpy(x).cuda()
    dense = (0, rows, dims[0], 1, 0)
    y, acts = forward_save(env, net, xd, dense)
    dx, g = c_input_grad(env, net, acts, dout)
    gw, gb, g2, dx2 = c_backward_dx(env, net, xd, dense, acts, dout)
    # the existing entry point on the same arguments: its grad_w / grad_b, its g, its y and acts
    y0, acts0, gw0, gb0, g0 = base.c_grad(env, net, xd, dense, dout)
    assert same(y, y0) and same(acts, acts0) and same(g, g0) and same(g2, g0) and same(dx, dx2)
    assert all(same(a, b) for a, b in zip(gw + gb, gw0 + gb0))
    # a second run; the same rows inside a NaN-surrounded record with an odd stride and a 4-byte-aligned base
    assert same(c_input_grad(env, net, acts, dout)[0], dx)
    rec, spec = base.in_record(x)
    y3, acts3 = forward_save(env, net, rec, spec)
    gw3, gb3, g3, dx3 = c_backward_dx(env, net, rec, spec, acts3, dout)
    assert same(acts3, acts) and same(dx3, dx) and all(same(a, b) for a, b in zip(gw3 + gb3, gw0 + gb0))
    if rows == 0:
        return
    assert not torch.isnan(dx).any()
    # loss.backward(): x.grad, and the parameters' gradients next to it
    xr = xd.clone().requires_grad_()
    out = net.apply(env, xr)
    assert out.grad_fn is not None and tuple(out.shape) == (rows, dims[-1])
    out.backward(torch.from_numpy(dout).cuda())
    torch.cuda.synchronize()
    assert same(out.detach(), y) and same(xr.grad, dx)
    params = [t for m in gc.linears(dev) for t in (m.weight, m.bias)]
    assert all(same(t.grad, ref) for t, ref in zip(params, [t for q in zip(gw0, gb0) for t in q]))
    dev.zero_grad()
    # dx alone: the parameters are not asked for, and are not given a gradient
    for t in params:
        t.requires_grad_(False)
    try:
        xr2 = xd.clone().requires_grad_()
        net.apply(env, xr2).backward(torch.from_numpy(dout).cuda())
        torch.cuda.synchronize()
        assert same(xr2.grad, dx) and all(t.grad is None for t in params)
    finally:
        for t in params:
            t.requires_grad_(True)
    what = f"{'x'.join(map(str, dims))} {mode} rows={rows}"
    r1 = igc.check_dx(gc.weights_of(mlp), x, acts.cpu().numpy(), dout, dx.cpu().numpy(), what=what)
    r2 = igc.check_end_to_end(dx.cpu().numpy(), mlp, x, dout, what=what)
    print(what, "layer 1", round(r1["ratio"], 5), "end to end", round(r2["ratio"], 4))


@pytest.mark.parametrize("dims,mode,pad", [(ACTOR, "exact", (5, 8)), (CRITIC, "split", (100, 128))], **IDS)
def test_dx_through_an_index_and_on_padded_rows_equals_the_dense_gather(env, dims, mode, pad):
    """130 rows = 10 index entries (a duplicate, not sorted) x 13 rows per block out of a record of 6 blocks"""
    import torch

    mlp, dev, net = network(dims, mode)
    rows, rpb, m, K = 130, 13, 10, dims[0]
    dout = base.inputs(rows, dims)[1]
    rng = np.random.default_rng(5)
    xf = ((rng.random((6, rpb, K)) * 2 - 1) * 1.5).astype(np.float32)
    rec, spec, index, x = base.frames_record((xf, m), 17)
    y, acts = forward_save(env, net, rec, spec, index)
    gw, gb, g, dx = c_backward_dx(env, net, rec, spec, acts, dout, index)
    xd = torch.from_numpy(x).cuda()
    yd, actsd = forward_save(env, net, xd, (0, rows, K, 1, 0))
    y0, acts0, gw0, gb0, g0 = base.c_grad(env, net, rec, spec, dout, index)
    assert same(acts, actsd) and same(acts, acts0) and same(dx, c_input_grad(env, net, actsd, dout)[0])
    assert all(same(a, b) for a, b in zip(gw + gb, gw0 + gb0))
    igc.check_dx(gc.weights_of(mlp), x, acts.cpu().numpy(), dout, dx.cpu().numpy(), what=f"{dims} indexed")
    # Mlp32.input_grad on the rows where they lie
    yi, dxi = net.input_grad(env, rows=(rec, *spec), index=index, dout=torch.from_numpy(dout).cuda())
    torch.cuda.synchronize()
    assert tuple(yi.shape) == (m, rpb, dims[-1]) and same(yi.reshape(rows, -1), y) and same(dxi, dx)
    # padded rows: the record holds in_dim / dst segments of src floats
    src, dst = pad
    segs = K // dst
    xm = ((rng.random((6, rpb, segs * src)) * 2 - 1) * 1.5).astype(np.float32)
    recp, specp, indexp, gathered = base.frames_record((xm, m), 18)
    xp = np.zeros((rows, K), np.float32)
    for a in range(segs):
        xp[:, a * dst:a * dst + src] = gathered[:, a * src:(a + 1) * src]
    yp, actsp = forward_save(env, net, recp, specp, indexp, pad)
    gwp, gbp, gp, dxp = c_backward_dx(env, net, recp, specp, actsp, dout, indexp, pad)
    ydp, actsdp = forward_save(env, net, torch.from_numpy(xp).cuda(), (0, rows, K, 1, 0))
    assert same(actsp, actsdp) and tuple(dxp.shape) == (rows, K) and same(dxp, c_input_grad(env, net, actsdp, dout)[0])
    gwd, gbd = base.c_grad(env, net, torch.from_numpy(xp).cuda(), (0, rows, K, 1, 0), dout)[2:4]
    assert all(same(a, b) for a, b in zip(gwp + gbp, gwd + gbd))
    igc.check_dx(gc.weights_of(mlp), xp, actsp.cpu().numpy(), dout, dxp.cpu().numpy(), what=f"{dims} padded")
    yq, dxq = net.input_grad(env, rows=(recp, *specp), index=indexp, pad=pad, dout=torch.from_numpy(dout).cuda())
    torch.cuda.synchronize()
    assert same(dxq, dxp)


@pytest.mark.parametrize("dims,mode", [(ODD, "split"), (CRITIC, "split")], **IDS)
def test_one_row_of_dout_gives_one_row_of_dx(env, dims, mode):
    import torch

    mlp, dev, net = network(dims, mode)
    rows = 130
    x = base.inputs(rows, dims)[0]
    xd = torch.from_numpy(x).cuda()
    y, acts = forward_save(env, net, xd, (0, rows, dims[0], 1, 0))
    rng = np.random.default_rng(rows)
    for r in (0, 63, 64, 129):
        dout = np.zeros((rows, dims[-1]), np.float32)
        dout[r] = rng.uniform(0.5, 1.5, dims[-1]) * rng.choice([-1.0, 1.0], dims[-1])
        dx, g = c_input_grad(env, net, acts, dout)
        inside = int(torch.count_nonzero(dx[r]))
        assert 0 < inside == int(torch.count_nonzero(dx)), f"probe {r}: dx is not zero outside the row"  # (a NaN left in dx counts as non-zero)
        igc.check_dx(gc.weights_of(mlp), x, acts.cpu().numpy(), dout, dx.cpu().numpy(), what=f"{dims} probe {r}")


@pytest.mark.parametrize("dims", [ACTOR, WIDE, [33, 256, 1]], ids=lambda v: "x".join(map(str, v)))
def test_layer_0s_transposed_form_follows_load_and_the_optimiser_step(env, dims):
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Mlp32

    w0, w1 = base.make_net(dims, 21).cuda(), base.make_net(dims, 22).cuda()
    a = Mlp32(w0, input_grad=True)
    x, dout = base.inputs(130, dims)
    xd, spec = torch.from_numpy(x).cuda(), (0, 130, dims[0], 1, 0)

    def dx_of(net):
        y, acts = forward_save(env, net, xd, spec)
        return c_input_grad(env, net, acts, dout)[0]

    before = dx_of(a)
    a.load(env, w1)
    b = Mlp32(w1, input_grad=True)
    after = dx_of(a)
    assert same(after, dx_of(b)) and not same(after, before)
    b.close()
    # one optimiser step on the device: the repack launch rewrites layer 0's transposed form from the updated parameters
    opt = learn.Adam(env, [(a, w1)], lr=1e-2)
    out = a.apply(env, xd)
    out.backward(torch.from_numpy(dout).cuda())
    opt.step(0.5)
    torch.cuda.synchronize()
    stepped = dx_of(a)
    fresh = Mlp32(copy.deepcopy(w1), input_grad=True)
    assert same(stepped, dx_of(fresh)) and not same(stepped, after)
    fresh.close()
    a.close()


def test_a_network_without_the_flag_refuses(env):
    import torch

    mlp, dev, net = network(ACTOR, "split", input_grad=False)
    x, dout = base.inputs(64, ACTOR)
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(NotImplementedError):
        net.apply(env, xd.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="input_grad=True"):
        net.input_grad(env, xd, dout=torch.from_numpy(dout).cuda())
    y, acts = forward_save(env, net, xd, (0, 64, 32, 1, 0))
    lib, h = env.lib, net.handle(env.lib, env)
    ws, dx, d = torch.zeros(3 * 64 * 256 + (1 << 16), device="cuda"), torch.zeros((64, 32), device="cuda"), torch.from_numpy(dout).cuda()
    EINVAL = lib.mlp32_input_grad(env.h, None, p(acts), p(d), 64, p(ws), p(dx))
    assert EINVAL != 0 and b"null network" in lib.last_error(env.h)
    assert lib.mlp32_input_grad(env.h, h, p(acts), p(d), 64, p(ws), p(dx)) == EINVAL and b"create_input_grad" in lib.last_error(env.h)
    gw, gb = [torch.zeros((o, i), device="cuda") for i, o in zip(ACTOR[:-1], ACTOR[1:])], [torch.zeros(o, device="cuda") for o in ACTOR[1:]]
    PA = C.c_void_p * 4
    args = (env.h, h, p(xd), 64, 32, 1, 0, None, 0, 0, 0, p(acts), p(d), p(ws), PA(*[t.data_ptr() for t in gw]), PA(*[t.data_ptr() for t in gb]), p(dx))
    assert lib.mlp32_backward_dx(*args) == EINVAL and b"create_input_grad" in lib.last_error(env.h)
    # a handle with the form: null and misaligned pointers, before any launch
    mlp2, dev2, net2 = network(ACTOR, "split")
    h2 = net2.handle(env.lib, env)
    assert lib.mlp32_input_grad(env.h, h2, p(acts), p(d), 64, p(ws), None) == EINVAL
    assert lib.mlp32_input_grad(env.h, h2, p(acts), p(d), 64, C.c_void_p(ws.data_ptr() + 4), p(dx)) == EINVAL
    assert lib.mlp32_input_grad(env.h, h2, p(acts), p(d), 64, p(ws), C.c_void_p(dx.data_ptr() + 2)) == EINVAL
    assert lib.mlp32_input_grad(env.h, h2, p(acts), p(d), -1, p(ws), p(dx)) == EINVAL
    assert lib.mlp32_input_grad(env.h, h2, None, None, 0, None, None) == 0  # no rows: nothing is launched
    nf = C.c_uint64(5)
    assert lib.mlp32_input_grad_workspace(h2, -1, C.byref(nf)) == EINVAL and lib.mlp32_input_grad_workspace(h2, 0, C.byref(nf)) == 0 and nf.value == 0
    env.sync()
    assert all((t == 0).all() for t in gw + gb + [dx])  # nothing ran
    # rows = (base, ...) with base.requires_grad stays refused with the flag too
    with pytest.raises(NotImplementedError):
        net2.apply(env, rows=(xd.clone().requires_grad_(), 0, 64, 32, 1, 0))


def test_observation_saliency_reads_the_record_in_place(env):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.saliency import observation_saliency

    torch.manual_seed(7)
    mlp = make_mlp(env.D)
    actor = Actor(copy.deepcopy(mlp).cuda(), low=base.LOW, high=base.HIGH, input_grad=True)
    T = 3
    obs_rec = torch.zeros((T, env.B, env.N, env.D), dtype=torch.float32, device="cuda")
    actor.rollout(env, T, obs_rec=obs_rec, seed=5)
    env.sync()
    assert obs_rec.abs().sum() > 0
    mean_abs, max_abs = observation_saliency(env, actor, obs_rec, outputs=(0, 1))
    torch.cuda.synchronize()
    assert tuple(mean_abs.shape) == tuple(max_abs.shape) == (2, env.D)
    dense = obs_rec.reshape(-1, env.D).clone()
    x = dense.cpu().numpy()
    for i, c in enumerate((0, 1)):
        dout = torch.zeros((len(x), 4), device="cuda")
        dout[:, c] = 1.0
        y, dx = actor._mlp32.input_grad(env, dense, dout=dout)
        torch.cuda.synchronize()
        assert same(mean_abs[i], dx.abs().mean(0)) and same(max_abs[i], dx.abs().amax(0))
        ref64, t32, scale = igc.references(mlp, x, dout.cpu().numpy())
        igc.check_end_to_end(dx.cpu().numpy(), mlp, x, dout.cpu().numpy(), what=f"saliency output {c}", refs=(ref64, t32, scale))
        bar = igc.E2E_A * np.abs(t32 - ref64).max() + igc.E2E_B * gc.ulp32(np.float64(scale))
        # the reductions: | max|got| - max|ref| | and | mean|got| - mean|ref| | are at most max|got - ref|, layer 2's bar; torch's fp32 mean over n rows adds at
        # most n roundings of partial sums no larger than the sum and one of the division: (n + 1) ulp32 of the mean
        assert np.abs(max_abs[i].cpu().numpy() - np.abs(ref64).max(0)).max() <= bar
        mean64 = np.abs(ref64).mean(0)
        assert (np.abs(mean_abs[i].cpu().numpy().astype(np.float64) - mean64) <= bar + (len(x) + 1) * gc.ulp32(mean64)).all()
    actor.close()
