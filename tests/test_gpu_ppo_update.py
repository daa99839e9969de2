"""Minibatch PPO on the device: frames by index in the differentiated network (sigmaenv_mlp32_forward_save_indexed / sigmaenv_mlp32_backward_indexed,
``apply(index=)``), the fused clip-PPO head (sigmaenv_ppo_head, ``learn.ppo_head``) and the update loop (``learn.update``).  The indexed kernels are held bit for bit
to the non-indexed ones on the same rows gathered dense -- the partition and every order depend on the row count alone --, the head to tests/ppo_head_check.py's
criterion against float64, the whole chain to float64 torch autograd with tests/gradient_check.py's end-to-end criterion.

Shapes: a record of F = 37 frames of N = 5 agents; the actor D -> 256^3 -> 4 with D in {32, 35} (16-byte and 4-byte rows), the critic N D -> 256^3 -> 1;
M in {1, 13, 52} frames = 5 / 65 / 260 actor rows (inside a 64-row tile, one row past it, two dW ranges) and 1 / 13 / 52 critic rows, plus 70 critic rows with
repetition (past a tile).  The head alone also at M in {1024, 1025, 2049} frames of an env of 16 agents: 64 / 65 / 129 workgroups, where a lane of the final sum adds
one, two, three workgroups (ppo_head_check.BIG_M)."""
import copy
import ctypes as C

import numpy as np
import pytest

import gradient_check as gc
import ppo_head_check as pc

pytestmark = pytest.mark.gpu

F, N = 37, 5
LOW, HIGH = list(pc.LOW), list(pc.HIGH)


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make_net(dims, seed):
    import torch

    torch.manual_seed(seed)
    layers = []
    for l in range(len(dims) - 1):
        layers += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.Tanh()] if l + 2 < len(dims) else [])
    net = torch.nn.Sequential(*layers)
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.5)
                m.bias.uniform_(-0.3, 0.3)
    return net


@pytest.fixture(scope="module")
def env():
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    e = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=6), n_envs=16,
                 device="cuda:0")
    e.reset_random(seed=3)
    yield e
    e.close()


_nets = {}


def network(which, D):
    """(torch module on the CPU, Mlp32, the rows of the [F, N, D] record as this network reads them) per (actor | critic, D), made once"""
    from sigmarl_amd.actor import Mlp32

    key = (which, D)
    if key not in _nets:
        dims = [D, 256, 256, 256, 4] if which == "actor" else [N * D, 256, 256, 256, 1]
        mlp = make_net(dims, 50 + len(_nets))
        _nets[key] = (mlp, Mlp32(mlp), (0, N, D, F, N * D) if which == "actor" else (0, 1, N * D, F, N * D))
    return _nets[key]


_records = {}


def record(D):
    """The observation record [F, N, D] (CPU float32 array and CUDA tensor), made once per D"""
    import torch

    if D not in _records:
        x = ((np.random.default_rng(7 + D).random((F, N, D)) * 2 - 1) * 1.5).astype(np.float32)
        _records[D] = (x, torch.from_numpy(x).cuda())
    return _records[D]


def patterns(M, seed=0):
    """the index patterns of a minibatch of M frames: the identity and a reversed permutation (M <= F), a random sample with duplicates"""
    g = np.random.default_rng(100 * M + seed)
    dup = g.integers(0, F, M).astype(np.int32)
    if M > 1:
        dup[-1] = dup[0]
    p = {"duplicates": dup}
    if M <= F:
        p["identity"] = np.arange(M, dtype=np.int32)
        p["reversed"] = g.permutation(F).astype(np.int32)[::-1][:M].copy()
    return p


def run(env, net, base, rows, index, dout):
    """(y, acts, grad_w, grad_b) of the saving forward and the backward on ``rows`` of ``base`` (``index``: a CUDA int32 tensor or None)"""
    spec = (base, *rows, index)
    y, acts = net._forward_save(env, spec)
    gw, gb = net._backward(env, spec, acts, dout)
    env.sync()
    return y, acts, gw, gb


# (70 frames with repetition: the critic's tile crossing -- the actor crosses a tile at 13 frames)
INDEXED_CASES = [(w, D, M) for w in ("actor", "critic") for D in (32, 35) for M in (1, 13, 52)] + [("critic", 32, 70), ("critic", 35, 70)]


@pytest.mark.parametrize("which,D,M", INDEXED_CASES)
def test_indexed_forward_and_backward_equal_the_dense_gather(env, which, D, M):
    import torch

    mlp, net, rows = network(which, D)
    x, xd = record(D)
    rpb, width = rows[1], rows[2]
    flat = xd.reshape(F, N * D)  # a frame per line
    for name, idx in patterns(M).items():
        index = torch.from_numpy(idx).cuda()
        n = M * rpb
        dout = torch.from_numpy((np.random.default_rng(M).standard_normal((n, net.out_dim)) / n).astype(np.float32)).cuda()
        y, acts, gw, gb = run(env, net, xd, rows, index, dout)
        assert tuple(y.shape) == (n, net.out_dim) and tuple(acts.shape) == (3, n, 256)
        # the same rows gathered dense, through the non-indexed entry points
        dense = flat.index_select(0, index.long()).reshape(n, width).contiguous()
        yd, actsd, gwd, gbd = run(env, net, dense, (0, n, width, 1, 0), None, dout)
        assert same(y, yd) and same(acts, actsd), (which, D, M, name)
        assert all(same(a, b) for a, b in zip(gw + gb, gwd + gbd)), (which, D, M, name)
        # a second run: the same bits
        y2, acts2, gw2, gb2 = run(env, net, xd, rows, index, dout)
        assert same(y, y2) and same(acts, acts2) and all(same(a, b) for a, b in zip(gw + gb, gw2 + gb2))
        if name == "identity":  # the existing strided call on the record's first M blocks
            ys, actss, gws, gbs = run(env, net, xd, (rows[0], rows[1], rows[2], M, rows[4]), None, dout)
            assert same(y, ys) and same(acts, actss) and all(same(a, b) for a, b in zip(gw + gb, gws + gbs))
        assert all(torch.isfinite(t).all() for t in gw + gb)


def c_head(env, case):
    """sigmaenv_ppo_head on ``case`` (tests/ppo_head_check.py): (dout_actor, dout_critic, result[8]) as numpy arrays; every output starts as NaN"""
    import torch
    from sigmarl_amd import capi

    M, N = case["out"].shape[:2]
    assert env.N == N
    dev = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    t = dict(index=dev(case["index"], np.int32), out=dev(case["out"]), value=dev(case["value"]), action=dev(case["action"]), sample_log_prob=dev(case["sample_log_prob"]),
             advantage=dev(case["advantage"]), value_target=dev(case["value_target"]), dout_actor=nan(M, N, 4), dout_critic=nan(M), result=nan(8),
             workspace=nan(capi.PPO_SUMS * ((M * N + 255) // 256)))
    a = capi.PpoHeadArgs()
    a.n_index, a.n_frames = M, case["action"].shape[0]
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    for d in range(2):
        a.low[d], a.high[d] = float(case["low"][d]), float(case["high"][d])
    a.clip_epsilon, a.entropy_coeff, a.critic_coeff = float(case["clip_epsilon"]), float(case["entropy_coeff"]), float(case["critic_coeff"])
    a.seed, a.counter = int(case["seed"]), int(case["counter"])
    torch.cuda.synchronize()
    rc = env.lib.ppo_head(env.h, C.byref(a))
    assert rc == 0, env.lib.last_error(env.h)
    env.sync()
    return t["dout_actor"].cpu().numpy(), t["dout_critic"].cpu().numpy(), t["result"].cpu().numpy()


@pytest.mark.parametrize("M", [1, 13, 52])
def test_head_holds_the_criterion_against_float64_and_repeats_its_bits(env, M):
    assert env.N == N
    for name, idx in patterns(M).items():
        case = pc.synthetic_case(N=N, F=F, seed=20 + M, index=idx, floor_rows=2)
        da, dc, res = c_head(env, case)
        r, ref = pc.check(da, dc, res, case, what=f"head M={M} {name}")
        assert res[6] == 0 and res[7] == 0
        da2, dc2, res2 = c_head(env, case)
        assert np.array_equal(da.view(np.int32), da2.view(np.int32)) and np.array_equal(dc.view(np.int32), dc2.view(np.int32))
        assert np.array_equal(res.view(np.int32), res2.view(np.int32))
    if M == 52:  # every branch is populated where it can be (260 rows)
        p = pc.populations(ref)
        assert all(p[k] > 0 for k in ("inside_pos", "inside_neg", "above_pos", "above_neg", "below_pos", "below_neg", "e_small", "e_large", "sigma_floor")), p


@pytest.fixture(scope="module")
def env16():
    """16 agents (the head's rows per frame are the env's agents): 1024 frames are 64 workgroups of 256 rows"""
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    e = SigmaEnv(Parameters(n_agents=pc.BIG_N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=6), n_envs=8,
                 device="cuda:0")
    e.reset_random(seed=3)
    yield e
    e.close()


@pytest.mark.parametrize("M", list(pc.BIG_M))
def test_head_past_64_workgroups_holds_the_criterion_and_counts_the_clipped_rows_exactly(env16, M):
    """M x 16 rows in 64 / 65 / 129 workgroups: in sigmaenv_ppo_sum_kernel every lane adds one workgroup, lane 0 two, lane 0 three (a ragged last pass).  The
    criterion against float64 as it stands, the same bits from a second launch, and clip_fraction bit for bit: the flags are 0 or 1, so their sum is exact in any
    order, and no row of the case lies in the branch band (asserted; tests/test_ppo_head_check.py holds the twin to the same)."""
    rows, groups, chain = pc.BIG_M[M]
    assert M * pc.BIG_N == rows and -(-rows // 256) == groups and -(-groups // 64) == chain
    for pattern in pc.BIG_PATTERNS:
        case, ref, c, moved = pc.big_case(M, pattern)
        assert not pc.in_the_band(ref, c).any() and pc.head(case, np.float32)["clipped"] == ref["clipped"]
        da, dc, res = c_head(env16, case)
        r, _ = pc.check(da, dc, res, case, what=f"head M={M} N={pc.BIG_N} {pattern}")
        assert r["ambiguous_rows"] == 0 and res[6] == 0 and res[7] == 0
        print(f"head M={M} {pattern}: clip_fraction {res[4]!r}, {ref['clipped']} of {rows} rows clipped in float64")
        assert res[4].tobytes() == pc.exact_clip_fraction(ref).tobytes()
        da2, dc2, res2 = c_head(env16, case)
        assert np.array_equal(da.view(np.int32), da2.view(np.int32)) and np.array_equal(dc.view(np.int32), dc2.view(np.int32))
        assert np.array_equal(res.view(np.int32), res2.view(np.int32))


def test_head_entropy_draws_are_those_the_host_generator_predicts(env):
    """entropy_coeff = 1 and zero advantages: dout_actor is the entropy sample's gradient alone, 2 tanh(loc + sigma z) / (M N) in its loc half -- a function of the
    draw of every row.  It and the entropy pass the criterion with the draws of the key (seed, counter, frame, agent, 7300 / 7301), and miss it with another counter."""
    case = pc.synthetic_case(N=N, F=F, seed=31, index=patterns(52)["duplicates"], entropy_coeff=1.0, counter=11, floor_rows=2)
    case["advantage"] = np.zeros_like(case["advantage"])
    da, dc, res = c_head(env, case)
    pc.check(da, dc, res, case, what="entropy draws")
    other = dict(case, counter=12)
    r, _ = pc.compare(da, dc, res, other)
    assert not r["ok"] and r["dloc"] > 1e3


def whole_chain_case(D, M, seed):
    """Networks, record, index and records for the end-to-end test; the records populate the branches for the float64 networks' outputs"""
    import torch

    amlp, anet, arows = network("actor", D)
    cmlp, cnet, crows = network("critic", D)
    x, xd = record(D)
    idx = patterns(M, seed)["duplicates"]
    with torch.no_grad():
        xs = torch.from_numpy(x[idx]).double()
        out64 = copy.deepcopy(amlp).double()(xs.reshape(M * N, D)).reshape(M, N, 4).numpy()
        v64 = copy.deepcopy(cmlp).double()(xs.reshape(M, N * D)).reshape(M).numpy()
    rec = pc.records_for(out64, v64, idx, F, N, seed)
    case = dict(out=out64.astype(np.float32), value=v64.astype(np.float32), index=idx, low=np.asarray(LOW, np.float32), high=np.asarray(HIGH, np.float32),
                clip_epsilon=0.2, entropy_coeff=0.01, critic_coeff=1.0, seed=77, counter=5, **rec)
    return amlp, cmlp, x, xd, idx, case


def chain_reference(amlp, cmlp, x, idx, case, dtype):
    """The parameter gradients of both networks, [dW_0, db_0, ..] each, by torch autograd of the whole chain (gather, networks, head) on the CPU in ``dtype``"""
    import torch

    M = len(idx)
    D = x.shape[-1]
    a, c = copy.deepcopy(amlp).to(dtype), copy.deepcopy(cmlp).to(dtype)
    xs = torch.from_numpy(x[idx]).to(dtype)
    out, v = a(xs.reshape(M * N, D)).reshape(M, N, 4), c(xs.reshape(M, N * D)).reshape(M)
    z = torch.from_numpy(pc.draws(case, np.float64 if dtype == torch.float64 else np.float32)).to(dtype)
    lo, le, lc = pc.torch_head(out, v, torch.from_numpy(idx.astype(np.int64)), case, z, dtype)
    (lo + le + lc).backward()
    return [[t.grad.numpy().astype(np.float64) for q in gc.linears(m) for t in (q.weight, q.bias)] for m in (a, c)]


@pytest.mark.parametrize("D,M", [(35, 52), (32, 13)])
def test_whole_chain_gradients_against_float64_autograd(env, D, M):
    """apply(index=) -> learn.ppo_head -> backward: the parameter gradients of both networks against float64 torch autograd of the whole chain, with
    gradient_check's end-to-end criterion and constants (the fp32 CPU autograd's own error as the yardstick)."""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Actor, Critic, Mlp32

    amlp, cmlp, x, xd, idx, case = whole_chain_case(D, M, seed=3)
    am, cm = copy.deepcopy(amlp).cuda(), copy.deepcopy(cmlp).cuda()
    actor, critic = Actor(am, low=LOW, high=HIGH), Critic(cm)
    index = torch.from_numpy(idx).cuda()
    out = actor.apply(env, rows=(xd, 0, N, D, F, N * D), index=index)
    value = Mlp32.apply(critic, env, rows=(xd, 0, 1, N * D, F, N * D), index=index).view(-1)
    assert tuple(out.shape) == (M, N, 4) and tuple(value.shape) == (M,) and out.grad_fn is not None and value.grad_fn is not None
    out.retain_grad()
    value.retain_grad()
    # the records as a [T, B, ..] batch of one time slice of F envs
    batch = {k: torch.from_numpy(case[k]).cuda().unsqueeze(0) for k in ("action", "sample_log_prob", "advantage", "value_target")}
    loss, info = learn.ppo_head(env, out, value, batch, index, low=LOW, high=HIGH, clip_epsilon=0.2, entropy_coeff=0.01, critic_coeff=1.0, seed=77, counter=5)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and set(info) == set(pc.RESULT) and not any(v.requires_grad for v in info.values())
    assert float(loss.detach()) == pytest.approx(sum(float(info[k]) for k in ("loss_objective", "loss_entropy", "loss_critic")), rel=1e-6)
    # the head inside the chain holds its own criterion on the device's network outputs
    # (backward scales the stored dout tensors by the incoming gradient 1.0: out.grad and value.grad ARE the head's dout)
    hc = dict(case, out=out.detach().cpu().numpy(), value=value.detach().cpu().numpy())
    pc.check(out.grad.cpu().numpy(), value.grad.cpu().numpy(), np.array([float(info[k]) for k in pc.RESULT], np.float32), hc, what=f"head in the chain D={D} M={M}")
    ref64, t32 = chain_reference(amlp, cmlp, x, idx, case, torch.float64), chain_reference(amlp, cmlp, x, idx, case, torch.float32)
    ref_head = pc.head(case)
    xs = x[idx]
    for mlp, mod, rows_x, dout, r64, r32, nm in ((amlp, am, xs.reshape(M * N, D), ref_head["dout_actor"].reshape(M * N, 4), ref64[0], t32[0], "actor"),
                                                  (cmlp, cm, xs.reshape(M, N * D), ref_head["dout_critic"].reshape(M, 1), ref64[1], t32[1], "critic")):
        grads = [t.grad.cpu().numpy() for q in gc.linears(mod) for t in (q.weight, q.bias)]
        scales = gc.references(mlp, rows_x, dout.astype(np.float32))[2]  # every tensor's largest sum of |terms|, at the float64 head's dout
        r = gc.measure_end_to_end(grads, r64, r32, scales)
        print(f"whole chain D={D} M={M} {nm}", {k: round(v, 4) for k, v in r["ratios"].items()})
        assert r["ok"], f"{nm}: gradients of the whole chain (A = {gc.E2E_A}, B = {gc.E2E_B}): error / bound {r['ratios']}"
    actor.close()
    critic.close()


def test_index_out_of_range_raises_on_the_host_before_any_launch(env):
    import torch

    mlp, net, rows = network("actor", 32)
    x, xd = record(32)
    net_dev = copy.deepcopy(mlp).cuda()
    net.load(env, net_dev)
    for bad in ([0, F, 1], [3, -1], [2 ** 31 - 1]):
        with pytest.raises(ValueError, match="index"):
            net.apply(env, rows=(xd, *rows), index=torch.tensor(bad, dtype=torch.int32, device="cuda"))
    # the Critic's frames and the Actor's pass the same check
    from sigmarl_amd.actor import Critic
    cm = make_net([env.N * env.D, 256, 256, 256, 1], 90).cuda()
    critic = Critic(cm)
    obs = torch.zeros((4, env.B, env.N, env.D), device="cuda")
    with pytest.raises(ValueError, match="index"):
        critic.apply(env, obs, index=torch.tensor([4 * env.B], dtype=torch.int32, device="cuda"))
    ok = critic.apply(env, obs, index=torch.tensor([4 * env.B - 1, 0], dtype=torch.int32, device="cuda"))
    assert tuple(ok.shape) == (2,)
    critic.close()


def test_index_of_the_wrong_kind_raises_type_error(env):
    import torch

    mlp, net, rows = network("actor", 32)
    x, xd = record(32)
    net.load(env, copy.deepcopy(mlp).cuda())
    good = torch.arange(6, dtype=torch.int32, device="cuda")
    for bad in (good.long(), good.cpu(), torch.arange(12, dtype=torch.int32, device="cuda")[::2], good.reshape(2, 3), [0, 1]):
        with pytest.raises(TypeError, match="index"):
            net.apply(env, rows=(xd, *rows), index=bad)
    with pytest.raises(TypeError, match="index"):
        net.apply(env, xd.reshape(-1, 32), index=good)  # index picks blocks of rows=
    assert tuple(net.apply(env, rows=(xd, *rows), index=good).shape) == (6, N, 4)


def test_update_changes_every_parameter_and_equals_the_loop_written_out(env):
    """One learn.update of 2 epochs x 2 minibatches on a 16-env, 4-step batch: every parameter changes, apply works afterwards (load was called), and the result is
    bit for bit that of the same loop written with the public pieces."""
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Actor, Critic, make_mlp

    T, B, D = 4, env.B, env.D
    assert B == 16
    torch.manual_seed(1)
    amod, cmod = make_mlp(D).cuda(), make_mlp(N * D, n_out=1).cuda()
    amod2, cmod2 = copy.deepcopy(amod), copy.deepcopy(cmod)
    actor, critic = Actor(amod, low=LOW, high=HIGH), Critic(cmod)
    actor2, critic2 = Actor(amod2, low=LOW, high=HIGH), Critic(cmod2)
    env.reset_random(seed=3)
    batch = learn.collect(env, actor, critic, T, gamma=0.99, lmbda=0.9, seed=5, counter0=0)
    env.sync()
    before = [p.detach().clone() for p in list(amod.parameters()) + list(cmod.parameters())]
    kw = dict(num_epochs=2, minibatch_size=32, clip_epsilon=0.2, entropy_coeff=1e-2, max_grad_norm=1.0)
    opt = torch.optim.Adam(list(amod.parameters()) + list(cmod.parameters()), lr=3e-4)
    gen = torch.Generator(device="cuda").manual_seed(9)
    infos = learn.update(env, actor, critic, amod, cmod, opt, batch, seed=4, counter0=100, generator=gen, **kw)
    torch.cuda.synchronize()
    assert len(infos) == 4 and all(np.isfinite(float(i[k])) for i in infos for k in pc.RESULT)
    after = list(amod.parameters()) + list(cmod.parameters())
    assert all(not torch.equal(a, b) and torch.isfinite(b).all() for a, b in zip(before, after))
    obs = batch["observation"]
    index = torch.arange(3, dtype=torch.int32, device="cuda")
    assert torch.isfinite(actor.apply(env, rows=(obs, 0, N, D, T * B, N * D), index=index)).all()  # (no stale-weight refusal: load was called)
    assert torch.isfinite(critic.apply(env, obs, index=index)).all()
    # the loop written out
    opt2 = torch.optim.Adam(list(amod2.parameters()) + list(cmod2.parameters()), lr=3e-4)
    gen2 = torch.Generator(device="cuda").manual_seed(9)
    pars2, k = list(amod2.parameters()) + list(cmod2.parameters()), 0
    for _ in range(2):
        chunks = learn.minibatches(T * B, 32, gen2)
        assert len(chunks) == 2 and all(c.dtype == torch.int32 and c.numel() == 32 for c in chunks)
        assert sorted(torch.cat(chunks).tolist()) == list(range(T * B))
        for idx in chunks:
            out = actor2.apply(env, rows=(obs, 0, N, D, T * B, N * D), index=idx)
            value = critic2.apply(env, obs, index=idx)
            loss, info = learn.ppo_head(env, out, value, batch, idx, low=LOW, high=HIGH, clip_epsilon=0.2, entropy_coeff=1e-2, seed=4, counter=100 + k)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(pars2, 1.0)
            opt2.step()
            opt2.zero_grad()
            actor2.load(env, amod2)
            critic2.load(env, cmod2)
            assert same(info["loss_objective"], infos[k]["loss_objective"]) and same(info["entropy"], infos[k]["entropy"])
            k += 1
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(after, pars2))
    # the last short chunk is kept (SamplerWithoutReplacement's default)
    assert [c.numel() for c in learn.minibatches(70, 32, torch.Generator(device="cuda").manual_seed(1))] == [32, 32, 6]
    for n in (actor, critic, actor2, critic2):
        n.close()
