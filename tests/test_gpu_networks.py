"""The network kernels against fp64 (tests/network_check.py) at the shapes the C-ABI accepts: sigmaenv_mlp32_* in both arithmetic modes over depth 2-4, input
widths 1-4096 (every staging path of layer 0, the K = 256 path, chunked inputs beyond 256), 1-32 outputs and ragged row counts; the split form's range edges;
output bounds; repeatability with models of different LDS needs interleaved on one handle, through every forward entry point; the MAPPO critic on wide observations; the bf16 actor at every
width it takes.  Every case has a fixed seed."""
import numpy as np
import pytest

import network_check as nc

pytestmark = pytest.mark.gpu

IN_DIMS = [1, 7, 8, 9, 16, 17, 33, 35, 255, 256, 257, 512, 592, 593, 608, 609, 1024, 1728, 4096]
DEPTHS = [2, 3, 4]
OUT_DIMS = [1, 2, 3, 4, 5, 31, 32]
ROWS = [1, 31, 63, 64, 65, 4097]
SPLIT_MAX_IN = 592  # the split form's widest input (sigmaenv_mlp32_create: its input tile in LDS); wider networks run exact


def sweep_cases():
    """(case id, depth, in_dim, out_dim, rows, weight scale, seed): every input width once, the other axes cycled so that each of their values occurs"""
    return [(i, DEPTHS[i % 3], d, OUT_DIMS[i % 7], ROWS[i % 6], 1.7 if i % 2 else 1.0, 1000 + i) for i, d in enumerate(IN_DIMS)]


def fuzz_cases(seed=0, n=12):
    """A fixed-seed run of tools/fuzz_mlp32.py's draws"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        depth = int(rng.integers(2, 5))
        in_dim = int(rng.choice([1, 3, 10, 16, 17, 31, 32, 33, 43, 64, 100, 255, 256, 257, 512, 600]))
        out_dim = int(rng.integers(1, 33))
        rows = int(rng.choice([1, 5, 31, 32, 33, 64, 1000, 4097]))
        out.append((100 + k, depth, in_dim, out_dim, rows, float(rng.choice([1.0, 1.7])), 2000 + k))
    return out


def make_net(depth, in_dim, out_dim, scale, seed):
    import torch
    torch.manual_seed(seed)
    dims = [in_dim] + [256] * (depth - 1) + [out_dim]
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers += [torch.nn.Linear(a, b), torch.nn.Tanh()]
    mlp = torch.nn.Sequential(*layers[:-1])
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(scale)
                m.bias.uniform_(-0.3, 0.3)
    return mlp


def make_input(rows, in_dim, seed, amp=1.5):
    g = np.random.default_rng(seed)
    return ((g.random((rows, in_dim), dtype=np.float32) * 2 - 1) * amp).astype(np.float32)


@pytest.fixture(scope="module")
def env():
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters
    e = SigmaEnv(Parameters(n_agents=2, scenario_type="cpm_entire", is_apply_mask=False, is_obs_noise=False), n_envs=2, device="cuda:0")
    yield e
    e.close()


PAD = 1024  # NaN sentinels behind every output


def run(env, net, x):
    """net.forward into an output buffer followed by PAD NaN sentinels; returns the outputs (numpy) after asserting the sentinels are untouched"""
    import torch
    xd = torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x
    rows = xd.shape[0]
    buf = torch.full((rows * net.out_dim + PAD,), float("nan"), device="cuda")
    out = buf[:rows * net.out_dim].view(rows, net.out_dim)
    net.forward(env, xd, out=out)
    env.sync()
    tail = buf[rows * net.out_dim:]
    assert torch.isnan(tail).all(), f"the kernel wrote {int((~torch.isnan(tail)).sum())} values beyond rows x out_dim"
    return out.cpu().numpy()


def expected_mode(mode, in_dim):
    return "split" if mode == "split" and in_dim <= SPLIT_MAX_IN else "exact"


@pytest.mark.parametrize("mode", ["split", "exact"])
@pytest.mark.parametrize("case", sweep_cases() + fuzz_cases(), ids=lambda c: f"c{c[0]}-d{c[1]}-in{c[2]}-out{c[3]}-r{c[4]}")
def test_mlp32_against_fp64(env, case, mode):
    from sigmarl_amd.actor import Mlp32
    _, depth, in_dim, out_dim, rows, scale, seed = case
    mlp = make_net(depth, in_dim, out_dim, scale, seed)
    x = make_input(rows, in_dim, seed)
    net = Mlp32(mlp, mode=mode)
    assert net.set_mode(mode) == expected_mode(mode, in_dim)
    try:
        nc.check(run(env, net, x), mlp, x, f"{mode} {case}")
    finally:
        net.close()


def test_split_mode_range_edges(env):
    """Weights at +-254.9 stay split and pass; one weight at 255 falls back to exact (and passes); inputs at +-4093 and near 1e-4 (fp16 lo parts subnormal) pass."""
    import torch
    from sigmarl_amd.actor import Mlp32
    mlp = make_net(4, 40, 4, 1.0, 31)
    with torch.no_grad():
        lin = [m for m in mlp if isinstance(m, torch.nn.Linear)]
        lin[0].weight[0, 0], lin[0].weight[1, 3] = 254.9, -254.9
        lin[1].weight[5, 7] = 254.9
        lin[3].weight[2, 9] = -254.9
    x = make_input(200, 40, 32)
    net = Mlp32(mlp)
    assert net.set_mode("split") == "split"
    nc.check(run(env, net, x), mlp, x, "split, weights at +-254.9")
    big = x.copy()
    big[::3, 0], big[1::3, 5], big[2::7, 39] = 4093.0, -4093.0, 4093.0
    nc.check(run(env, net, big), mlp, big, "split, inputs at +-4093")
    tiny = make_input(200, 40, 33, amp=1e-4)
    nc.check(run(env, net, tiny), mlp, tiny, "split, inputs near 1e-4")
    net.close()
    with torch.no_grad():
        lin[1].weight[5, 7] = 255.0
    net = Mlp32(mlp)
    assert net.set_mode("split") == "exact"
    nc.check(run(env, net, x), mlp, x, "split requested, a weight at 255: exact")
    net.close()


@pytest.mark.parametrize("mode", ["split", "exact"])
def test_zero_rows_write_nothing(env, mode):
    import ctypes as C

    import torch
    from sigmarl_amd.actor import Mlp32
    net = Mlp32(make_net(4, 32, 4, 1.0, 41), mode=mode)
    x = torch.from_numpy(make_input(64, 32, 41)).cuda()
    buf = torch.full((256,), float("nan"), device="cuda")
    assert env.lib.mlp32_forward(env.h, net.handle(env.lib), C.c_void_p(x.data_ptr()), 0, C.c_void_p(buf.data_ptr())) == 0
    assert tuple(net.forward(env, x[:0]).shape) == (0, 4)
    env.sync()
    assert torch.isnan(buf).all()
    net.close()


@pytest.mark.parametrize("mode", ["split", "exact"])
@pytest.mark.parametrize("in_dim", [32, 36, 512])
def test_input_view_at_a_storage_offset(env, in_dim, mode):
    """A view whose data pointer is not 16-byte aligned is copied by Mlp32.forward (the kernels read rows with 16-byte loads): same bits as the aligned input."""
    import torch
    from sigmarl_amd.actor import Mlp32
    net = Mlp32(make_net(3, in_dim, 4, 1.0, 51), mode=mode)
    x = make_input(130, in_dim, 52)
    flat = torch.zeros(130 * in_dim + 1, device="cuda")
    flat[1:] = torch.from_numpy(x).reshape(-1).cuda()
    view = flat[1:].view(130, in_dim)
    assert view.data_ptr() % 16 != 0
    got = run(env, net, view)
    assert np.array_equal(got, run(env, net, x))
    assert torch.equal(view, torch.from_numpy(x).cuda())  # (the caller's tensor is left as it was)
    net.close()


def test_repeatable_and_lds_settings_per_model(env):
    """The same input twice on one handle gives the same bits; models of different LDS needs -- a wide exact one, a narrow split one, a split one at 512
    inputs (the split kernel's dynamic-LDS attribute above 64 KB) -- interleaved on one env handle give the bits each gives alone."""
    from sigmarl_amd.actor import Mlp32
    specs = [("wide exact", 4, 1024, 1, "exact"), ("narrow", 4, 35, 4, "split"), ("split 512", 4, 512, 1, "split"), ("narrow exact", 2, 9, 3, "exact")]
    nets, xs, alone = [], [], []
    for k, (name, depth, in_dim, out_dim, mode) in enumerate(specs):
        mlp = make_net(depth, in_dim, out_dim, 1.0, 60 + k)
        nets.append(Mlp32(mlp, mode=mode))
        assert nets[-1].set_mode(mode) == mode
        xs.append(make_input(333, in_dim, 70 + k))
        a = run(env, nets[-1], xs[-1])
        assert np.array_equal(a, run(env, nets[-1], xs[-1])), f"{name}: two runs differ"
        nc.check(a, mlp, xs[-1], name)
        alone.append(a)
    for k in [0, 1, 2, 0, 2, 1, 3, 0, 3, 2]:
        assert np.array_equal(run(env, nets[k], xs[k]), alone[k]), f"{specs[k][0]} interleaved differs from alone"
    for n in nets:
        n.close()


LDS_WIDTHS = [8, SPLIT_MAX_IN, 8]  # a narrow network, the widest the split kernel's LDS takes, the narrow one again
LDS_CASES = [(entry, mode) for entry in ("forward", "forward_rows", "forward_rows_pad") for mode in ("split", "exact")] + [
    (entry, "exact") for entry in ("forward_save", "forward_save_indexed", "forward_save_indexed_pad")]  # (the saving forward is the exact chain in either mode)
_lds_nets = {}


def lds_net(in_dim, mode):
    """(torch module, Mlp32) per (input width, mode), made once"""
    from sigmarl_amd.actor import Mlp32
    if (in_dim, mode) not in _lds_nets:
        mlp = make_net(3, in_dim, 3, 1.0, 80 + in_dim)
        _lds_nets[(in_dim, mode)] = (mlp, Mlp32(mlp, mode=mode))
    return _lds_nets[(in_dim, mode)]


@pytest.mark.parametrize("entry,mode", LDS_CASES, ids=lambda v: v)
def test_every_forward_entry_point_gets_the_lds_its_network_needs(env, entry, mode):
    """Each forward entry point, on one env handle, with networks of 8, 592 and 8 inputs in turn: the dynamic-LDS limit is kept per kernel instantiation and raised
    when a network needs more than an earlier one left set -- a limit looked up under another kernel's key makes the wide launch fail with an error code.  65 rows
    as 5 blocks of 13 (two tiles, the second ragged) at a row stride one float above the row's width and a base 3 floats into the tensor (4-byte aligned rows), NaN
    around them; padded: segments of 3 floats read as 4 columns; indexed: 5 of a record's 7 blocks, one twice.  Every call succeeds and gives the bits of
    sigmaenv_mlp32_forward on the dense (padded) copy of the rows in the same arithmetic; sigmaenv_mlp32_forward itself is held to fp64.  (The limit is also kept per
    device: one GPU cannot show that.)"""
    import torch
    SRC, DST, RPB, NB, FRAMES, OFF = 3, 4, 13, 5, 7, 3
    padded, indexed = entry.endswith("_pad"), "indexed" in entry
    pick = np.array([6, 0, 3, 3, 1])
    index = torch.from_numpy(pick.astype(np.int32)).cuda()
    for in_dim in LDS_WIDTHS:
        mlp, net = lds_net(in_dim, mode)
        assert net.set_mode(mode) == mode
        width, nrec = in_dim // DST * SRC if padded else in_dim, FRAMES if indexed else NB  # the row in memory; the record's blocks
        rs = width + 1
        x = make_input(nrec * RPB, width, 7 * in_dim)
        rec = np.full(OFF + nrec * RPB * rs, np.nan, np.float32)
        rec[OFF:].reshape(nrec * RPB, rs)[:, :width] = x
        dense = x.reshape(nrec, RPB, width)[pick] if indexed else x
        dense = dense.reshape(NB * RPB, width)
        if padded:
            dense = np.concatenate([dense.reshape(NB * RPB, -1, SRC), np.zeros((NB * RPB, in_dim // DST, DST - SRC), np.float32)], axis=2)
        dense = np.ascontiguousarray(dense.reshape(NB * RPB, in_dim))
        spec = (torch.from_numpy(rec).cuda(), OFF, RPB, rs, nrec, RPB * rs)
        want = net.forward(env, torch.from_numpy(dense).cuda())
        if entry == "forward":
            env.sync()
            nc.check(want.cpu().numpy(), mlp, dense, f"{entry} {mode} in={in_dim}")
            continue
        if entry.startswith("forward_rows"):
            got = net.forward_rows(env, *spec, pad=(SRC, DST) if padded else None)
        else:
            got = net._forward_save(env, spec + (index if indexed else None,) + (((SRC, DST),) if padded else ()))[0]
        env.sync()
        assert torch.equal(got.reshape(want.shape).view(torch.int32), want.view(torch.int32)), f"{entry} {mode} in={in_dim}"


@pytest.mark.parametrize("mode", ["split", "exact"])
@pytest.mark.parametrize("n_agents,n_observed", [(32, 2), (16, 4)])
def test_wide_critic_on_env_observations(n_agents, n_observed, mode):
    """The MAPPO critic at 32 agents x D = 32 (BASELINE config 4: 1024 inputs) and 16 agents x D = 54 (n_nearing_agents_observed = 4: 864 inputs), on real
    observations -- sigmaenv_mlp32_create refused both before layer 0's inputs were staged in chunks."""
    import torch
    from sigmarl_amd.actor import Critic
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters
    e = SigmaEnv(Parameters(n_agents=n_agents, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False,
                            n_nearing_agents_observed=n_observed), n_envs=70, device="cuda:0")
    e.reset_random(seed=8)
    assert e.N * e.D == {32: 1024, 16: 864}[n_agents]
    net = make_net(4, e.N * e.D, 1, 1.0, 90 + n_agents)
    critic = Critic(net, mode=mode)
    assert critic.set_mode(mode) == "exact"  # (wider than the split form takes)
    v = critic.values(e)
    e.sync()
    assert tuple(v.shape) == (e.B, e.N, 1) and torch.equal(v[:, 0], v[:, -1])
    obs = e.obs.reshape(e.B, e.N * e.D).cpu().numpy()
    nc.check(v[:, 0].cpu().numpy(), net, obs, f"critic {n_agents} x {e.D} {mode}")
    e.close()
    critic.close()


def test_inputs_wider_than_4096_are_refused_at_construction():
    from sigmarl_amd.actor import Critic, Mlp32
    for cls in (Mlp32, Critic):
        with pytest.raises(ValueError, match="4096"):
            cls(make_net(2, 4097, 1, 1.0, 0))


# rows of the bf16 actor: (n_envs, n_agents) with B N = 1, 255, 256, 257
BF16_ROWS = [(1, 1), (51, 5), (16, 16), (257, 1)]


@pytest.mark.parametrize("obs_dim", [8, 16, 24, 32])
def test_bf16_actor_against_its_restatement(obs_dim):
    """sigmaenv_actor (bf16 weights / activations, fp32 accumulation) at every width it takes, on explicit observations, against the bf16 restatement with
    the tolerances of tests/test_gpu_actor.py"""
    import torch
    from sigmarl_amd.actor import Actor, make_mlp
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters
    torch.manual_seed(obs_dim)
    mlp = make_mlp(obs_dim)
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    bias = np.log(np.expm1(0.99))
    sp = lambda v: np.maximum(np.log1p(np.exp(v + bias)) + 0.01, 1e-4)  # noqa: E731
    for B, N in BF16_ROWS:
        e = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=B, device="cuda:0")
        actor = Actor(mlp, low=[-1.0, -0.6], high=[1.0, 0.6], precision="bf16")
        R = B * N
        obs = torch.from_numpy(make_input(R, obs_dim, 300 + R)).cuda()
        act = torch.zeros((B, N, 2), device="cuda")
        ls = torch.full((B, N, 4), float("nan"), device="cuda")
        actor.forward(e, act, None, ls, obs=obs, deterministic=True)
        e.sync()
        got = ls.reshape(R, 4).cpu().numpy()
        want = nc.emulated_bf16(mlp, obs.cpu().numpy())
        assert np.isfinite(got).all()
        assert np.abs(got[:, :2] - want[:, :2]).max() <= 2e-2, (obs_dim, R)
        assert np.abs(got[:, 2:] - sp(want[:, 2:])).max() <= 2e-2, (obs_dim, R)
        assert np.abs(got[:, :2] - want[:, :2]).mean() <= 2e-3, (obs_dim, R)
        e.close()
        actor.close()
