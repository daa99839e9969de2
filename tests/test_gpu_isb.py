"""The challenging initial-state buffer on the device (sigmaenv_isb_*, ``sigmarl_amd.initial_states``) held to the numpy twin tests/isb_check.py and to the oracle's
``reset`` / ``auto_reset``.

1. planted frames through ``record``, five steps, every bank row, ptr, count, every ring, held / head and pending compared with the twin as words: tiles 2 x 1,
   3 x 5, 4 x 4, 16 x 1; B = 1, 5, W, W + 1, 2 W + 1 with W the record workgroup's chunk (asserted); capacity and n_steps_stored 1 and 3; R = 0, 1, capacity,
   capacity + 1, 2 capacity + 1 recorders in one step with ptr wrapping across the steps; p_record 0, 1 and 0.5 with the draws recomputed on the host.
2. ``restart`` + ``auto_reset`` + ``settle`` against ``OracleEnv.reset(the twin's entries, full_env=1)`` + ``auto_reset`` at the bars of test_gpu_parity.py; an empty
   bank restarts nothing; p_use = 0 attached is the unattached fused rollout, bit for bit.
3. ``Actor.rollout`` of 24 steps with the bank attached equals the chain written out with the public per-step calls, bit for bit: plain, prioritized, with the CBF-QP
   chain, with an ``Evaluator`` attached as well; ``learn.train_iteration(initial_states=)`` equals its parts.
4. a run that really records: CPM, 4 agents x 64 envs, full speed straight ahead, p_use = 0.5, the seed picked on the CPU with the oracle
   (tests/test_isb_check.py::test_the_recording_run_on_the_oracle): at least 8 recordings, at least 2 restarts from the bank, every restarted env's rows are the entry's."""
import copy

import numpy as np
import pytest

import isb_check as ic

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)
TILES = [(2, 1), (3, 5), (4, 4), (16, 1)]  # agents x envs per tile
W = ic.CHUNK


def _env(N, B, G=0, **kw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    p = dict(KW, n_agents=N)
    p.update(kw)
    env = SigmaEnv(Parameters(**p), n_envs=B, device="cuda:0", envs_per_group=G)
    if G:
        assert env.launch_shape()["wave_G"] == G
    return env


def _bank_words(bank):
    from sigmarl_amd import capi

    bank.env.sync()
    names = dict(bank_state=capi.ISB_BANK_STATE, bank_path=capi.ISB_BANK_PATH, words=capi.ISB_WORDS, ring_state=capi.ISB_RING_STATE, ring_path=capi.ISB_RING_PATH,
                 held=capi.ISB_HELD, head=capi.ISB_HEAD, pending=capi.ISB_PENDING)
    return {k: bank.view(v).cpu().numpy() for k, v in names.items()}


def _same_as_twin(got, tw, tag):
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    assert got["words"].tolist() == [tw.ptr, tw.count], (tag, got["words"].tolist(), tw.ptr, tw.count)
    for k in ("bank_state", "bank_path", "ring_state", "ring_path", "held", "head", "pending"):
        assert np.array_equal(bits(got[k]), bits(getattr(tw, k))), (tag, k)


def _plant(env, rng, n_recorders):
    """A frame written through the env's views: random rows, ``n_recorders`` envs with one collision byte set somewhere, random requests, done flags, counters"""
    import torch
    from sigmarl_amd import capi

    B, N = env.B, env.N
    f = dict(state=rng.standard_normal((B, N, 8)).astype(np.float32), path=rng.integers(0, 1 << 20, (B, N, 4)).astype(np.int32),
             col_agents=np.zeros((B, N, N), np.uint8), col_flags=(rng.random((B, N, 4)) < 0.1).astype(np.uint8), done=(rng.random(B) < 0.4).astype(np.uint8),
             timer=rng.integers(0, 50, (B, 4)).astype(np.int32))
    who = rng.permutation(B)[: min(n_recorders, B)]
    flat = f["col_agents"].reshape(B, N * N)
    flat[who, rng.integers(0, N * N, len(who))] = rng.integers(1, 256, len(who)).astype(np.uint8)
    if len(who):
        flat[who[0], N * N - 1] = 1  # (the last byte of a block: the scan reaches the end)
    for k, which in (("state", capi.BUF_STATE), ("path", capi.BUF_PATH), ("col_agents", capi.BUF_COL_AGENTS), ("col_flags", capi.BUF_COL_FLAGS), ("done", capi.BUF_DONE),
                     ("timer", capi.BUF_TIMER)):
        env.buffer(which).copy_(torch.from_numpy(f[k]))
    return f


# ---- 1. planted frames -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, W, W + 1, 2 * W + 1])
@pytest.mark.parametrize("N,G", TILES)
def test_planted_frames_equal_the_twin_as_words(N, G, B):
    from sigmarl_amd import capi
    from sigmarl_amd.initial_states import InitialStateBank

    assert capi.ISB_CHUNK == W == 1024  # SIGMAENV_ISB_CHUNK: the record workgroup's chunk (tests/test_isb_check.py holds it to the headers)
    env = _env(N, B, G)
    rng = np.random.default_rng(1000 * N + B)
    seed = 0xABCDEF0123456789
    recorded = 0
    for cap, S, p_record in ((1, 1, 1.0), (3, 3, 1.0), (1, 3, 1.0), (3, 1, 1.0), (3, 3, 0.0), (3, 3, 0.5)):
        f = _plant(env, rng, 0)
        bank = InitialStateBank(env, capacity=cap, n_steps_stored=S, probability_record=p_record, probability_use_recording=0.0)
        tw = ic.Twin(B, N, cap, S, p_record, 0.0)
        tw.reset(f["state"], f["path"], f["timer"])
        _same_as_twin(_bank_words(bank), tw, (cap, S, p_record, "reset"))
        for t, R in enumerate((0, 1, cap, cap + 1, 2 * cap + 1) if p_record == 1.0 else (B, B, B, B, B)):
            f = _plant(env, rng, R)
            bank.record(seed, 7 + t)
            r = tw.record(f["state"], f["path"], f["col_agents"], f["col_flags"], f["done"], seed, 7 + t)
            if p_record == 1.0:
                assert r["R"] == min(R, B)
            recorded += r["R"]
            _same_as_twin(_bank_words(bank), tw, (cap, S, p_record, t))
        if p_record == 0.0:
            assert tw.count == 0
        bank.close()
    assert recorded > 0
    env.close()


# ---- 2. restart against the oracle ------------------------------------------------------------------------------------------------------------------
def _pair(N, B, G):
    import oracle_binding as ob
    from sigmarl_amd.env import NumpyAdapter, SigmaEnv
    from sigmarl_amd.maps import load_map
    from sigmarl_amd.params import Parameters, make_config

    p = Parameters(**dict(KW, n_agents=N))
    mp = load_map("cpm_entire")
    cfg = make_config(p, mp, B)
    cfg.envs_per_group = G
    dev = NumpyAdapter(SigmaEnv(cfg=cfg, map_table=mp, device="cuda:0"))
    assert dev.env.launch_shape()["wave_G"] == G
    return dev, ob.OracleEnv(cfg, mp), mp


@pytest.mark.parametrize("p_use", [1.0, 0.5])
@pytest.mark.parametrize("N,G", TILES)
def test_restart_auto_reset_settle_against_the_oracle(N, G, p_use):
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.initial_states import InitialStateBank
    from test_gpu_parity import _compare_all

    B, seed, counter = 9, 11, 77
    dev, ora, mp = _pair(N, B, G)
    first, count = mp.list_first[0], mp.list_count[0]
    dev.env.buffer(capi.BUF_DONE).fill_(1)
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    dev.auto_reset(1, 0, first, count)
    ora.auto_reset(1, 0, first, count)
    entries_state, entries_path = dev.get(capi.BUF_STATE)[:3].copy(), dev.get(capi.BUF_PATH)[:3].copy()  # three scenes the sampler placed
    entries_state[:, :, 3] = 0.25  # (a speed of their own: the whole state row is restored)
    rng = np.random.default_rng(N)
    for t in range(3):
        act = np.stack([rng.uniform(0, 1, (B, N)), rng.uniform(-0.25, 0.25, (B, N))], axis=-1).astype(np.float32)
        dev.step(act)
        ora.step(act)
    done = np.zeros(B, np.uint8)
    done[[0, 2, 3, 5, 8]] = 1  # a planted mix of finished and live envs
    dev.env.buffer(capi.BUF_DONE).copy_(torch.from_numpy(done))
    ora.get(capi.BUF_DONE, copy=False)[:] = done
    # an empty bank restarts nothing
    empty = InitialStateBank(dev.env, capacity=4, n_steps_stored=2, probability_record=0.0, probability_use_recording=1.0)
    before = {w: dev.get(w) for w in range(capi.BUF_CBF_NOMINAL + 1)}
    empty.restart(seed, counter)
    for w, a in before.items():
        assert np.array_equal(a.view(np.uint8), dev.get(w).view(np.uint8)), w
    empty.close()
    bank = InitialStateBank(dev.env, capacity=4, n_steps_stored=2, probability_record=0.0, probability_use_recording=p_use)
    bank.load(torch.from_numpy(entries_state).cuda(), torch.from_numpy(entries_path).cuda())
    assert bank.count == 3 and bank.ptr == 3
    tw = ic.Twin(B, N, 4, 2, 0.0, p_use)
    tw.reset(dev.get(capi.BUF_STATE), dev.get(capi.BUF_PATH), dev.get(capi.BUF_TIMER))
    tw.count, tw.ptr = 3, 3
    uses, j = tw.restart(done, seed, counter)
    assert uses.sum() >= 1 and (p_use < 1.0 or uses.sum() == done.sum()) and not uses[done == 0].any()
    bank.restart(seed, counter)
    dev.auto_reset(seed, counter, first, count)
    bank.settle()
    env_idx = np.repeat(np.nonzero(uses)[0], N).astype(np.int32)
    ora.reset(env_idx, np.tile(np.arange(N, dtype=np.int32), int(uses.sum())), entries_path[j[uses]].reshape(-1, 4), entries_state[j[uses]].reshape(-1, 8), True)
    ora.observe()
    ora.auto_reset(seed, counter, first, count)
    assert _compare_all(dev, ora, f"restart {N}x{G}") == 0  # integer buffers and masks bit for bit, zero differing non-observation fp32 words, observations 1e-5
    state = dev.get(capi.BUF_STATE)
    for b in np.nonzero(uses)[0]:
        assert np.array_equal(state[b].view(np.uint32), entries_state[j[b]].view(np.uint32))
    timer = dev.get(capi.BUF_TIMER)
    assert not dev.get(capi.BUF_DONE).any() and (timer[done == 1, 0] == 0).all() and (timer[done == 1, 3] == 2).all() and (timer[done == 0, 3] == 1).all()
    # settle: every env that was reset starts its history anew, the others keep theirs
    settled = tw.settle(state, dev.get(capi.BUF_PATH), timer)
    assert np.array_equal(settled, done == 1)
    got = _bank_words(bank)
    for k in ("ring_state", "ring_path", "held", "head", "pending"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(getattr(tw, k)).view(np.uint8)), k
    bank.close()
    dev.close()
    ora.close()


def _actor(env, in_extra=False, seed=1):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp

    torch.manual_seed(seed)
    mlp = make_mlp(env.D + (2 * env.K if in_extra else 0))
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    return Actor(mlp, low=LOW, high=HIGH)


def _records(T, B, N, D):
    import torch

    return dict(slab=torch.zeros(T, B, N * (D + 1) + 1, device="cuda"), log_prob=torch.zeros(T, B, N, device="cuda"), actions=torch.zeros(T, B, N, 2, device="cuda"),
                obs_rec=torch.zeros(T, B, N, D, device="cuda"))


def _bits(t):
    import torch

    return t.contiguous().reshape(-1).view(torch.uint8)


def _same_envs(a, b):
    import torch
    from sigmarl_amd.env import _buf_layout

    return [w for w in _buf_layout(a.B, a.N, a.K, a.D) if not torch.equal(_bits(a.buffer(w)), _bits(b.buffer(w)))]


def test_p_use_zero_attached_is_the_unattached_fused_rollout():
    import torch
    from sigmarl_amd.initial_states import InitialStateBank

    N, B, T = 16, 5, 12
    envs = [_env(N, B, max_steps=5) for _ in range(2)]
    for e in envs:
        e.reset_random(seed=3)
    actor = _actor(envs[0])
    rec = [_records(T, B, N, envs[0].D) for _ in range(2)]
    actor.rollout(envs[0], T, seed=5, counter0=40, **rec[0])
    bank = InitialStateBank(envs[1], capacity=3, n_steps_stored=3, probability_use_recording=0.0)
    with bank.attached():
        actor.rollout(envs[1], T, seed=5, counter0=40, **rec[1])
    envs[0].sync()
    envs[1].sync()
    for k in rec[0]:
        assert torch.equal(_bits(rec[0][k]), _bits(rec[1][k])), k
    assert _same_envs(envs[0], envs[1]) == []
    assert rec[0]["slab"][:, :, -1].sum().item() >= B  # envs finished: the resets ran
    for x in (bank, actor, *envs):
        x.close()


# ---- 3. the attached rollout equals the chain written out ----------------------------------------------------------------------------------------
CASES = {
    "plain": dict(N=16, B=5, pkw=dict(max_steps=5), roll=dict()),
    "prioritized": dict(N=16, B=5, pkw=dict(is_using_prioritized_marl=True, max_steps=5), roll=dict(wrapper="prioritized", priority="random"), in_extra=True),
    "cbf_qp": dict(N=4, B=6, pkw=dict(rew_method="cbf", is_solve_qp=True, is_using_cbf_training=True, is_apply_cbf_action=True, dt=0.05, max_steps=5), roll=dict(), cbf=True),
    "evaluator": dict(N=4, B=6, pkw=dict(max_steps=5), roll=dict(), evaluator=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_attached_rollout_equals_the_chain_written_out(case):
    import torch
    from sigmarl_amd.evaluate import Evaluator
    from sigmarl_amd.initial_states import InitialStateBank

    c = CASES[case]
    N, B, T, seed, counter0 = c["N"], c["B"], 24, 5, 40
    envs = [_env(N, B, **c["pkw"]) for _ in range(3)]  # unattached, attached, the chain by hand
    for e in envs:
        e.reset_random(seed=3)
        if c.get("cbf"):
            e.cbf_attach()
    actor = _actor(envs[0], c.get("in_extra", False))
    D = envs[0].D
    rec = [_records(T, B, N, D) for _ in range(2)]
    actor.rollout(envs[0], T, seed=seed, counter0=counter0, **rec[0], **c["roll"])
    banks = [InitialStateBank(e, capacity=3, n_steps_stored=3, probability_use_recording=0.5) for e in envs[1:]]
    for bk in banks:  # two scenes to restart from, from the first step on
        bk.load(bk.env.state[:2].clone(), bk.env.buffer(3)[:2].clone())  # (3: capi.BUF_PATH)
    evs = [Evaluator(e) for e in envs[1:]] if c.get("evaluator") else [None, None]
    with banks[0].attached():
        if evs[0] is not None:
            with evs[0].attached():
                actor.rollout(envs[1], T, seed=seed, counter0=counter0, **rec[1], **c["roll"])
        else:
            actor.rollout(envs[1], T, seed=seed, counter0=counter0, **rec[1], **c["roll"])
    slab = torch.zeros_like(rec[1]["slab"])
    for t in range(T):
        act = rec[1]["actions"][t].contiguous()
        envs[2].set_slab(slab[t])
        envs[2].step(envs[2].cbf_qp(act) if c.get("cbf") else act)
        if evs[1] is not None:
            evs[1].accumulate()
        banks[1].record(seed, counter0 + t)
        banks[1].restart(seed, counter0 + t)
        envs[2].auto_reset(seed=seed, counter=counter0 + t)
        banks[1].settle()
    envs[2].set_slab(None)
    got, want = _bank_words(banks[0]), _bank_words(banks[1])
    for k in got:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
    assert _same_envs(envs[1], envs[2]) == []
    assert torch.equal(_bits(rec[1]["slab"]), _bits(slab))
    assert _same_envs(envs[0], envs[1]) != [], "no restart changed the course of the rollout: the test shows nothing"
    if evs[0] is not None:
        a, h = evs[0].accumulators(), evs[1].accumulators()
        assert all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(h[k]).view(np.uint8)) for k in a) and evs[0].frames == T
    for x in (*[e for e in evs if e is not None], *banks, actor, *envs):
        x.close()


def test_train_iteration_with_a_bank_equals_its_parts():
    import torch
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Actor, Critic, make_mlp
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.initial_states import InitialStateBank
    from sigmarl_amd.params import Parameters

    def params():
        return Parameters(n_agents=4, num_vmas_envs=8, n_iters=4, num_epochs=2, minibatch_size=16, lr=3e-4, lr_min=1e-5, max_steps=4,
                          is_challenging_initial_state_buffer=True, **KW)

    p, p2 = params(), params()
    B, T, SEED, C0 = 8, p.frames_per_batch // 8, 4, 100
    env, env2 = SigmaEnv(p, n_envs=B, device="cuda:0"), SigmaEnv(p2, n_envs=B, device="cuda:0")
    env.reset_random(seed=3)
    env2.reset_random(seed=3)
    torch.manual_seed(1)
    amod, cmod = make_mlp(env.D).cuda(), make_mlp(env.N * env.D, n_out=1).cuda()
    amod2, cmod2 = copy.deepcopy(amod), copy.deepcopy(cmod)
    actor, critic, actor2, critic2 = Actor(amod, low=LOW, high=HIGH), Critic(cmod), Actor(amod2, low=LOW, high=HIGH), Critic(cmod2)
    opt, opt2 = learn.Adam(env, [(actor, amod), (critic, cmod)], lr=p.lr), learn.Adam(env2, [(actor2, amod2), (critic2, cmod2)], lr=p.lr)
    bank, bank2 = InitialStateBank(env, capacity=3, probability_use_recording=0.5), InitialStateBank(env2, capacity=3, probability_use_recording=0.5)
    assert bank.n_steps_stored == p.n_steps_stored == 10
    for bk in (bank, bank2):
        bk.load(bk.env.state[:2].clone(), bk.env.buffer(3)[:2].clone())
    with pytest.raises(NotImplementedError, match="InitialStateBank"):  # the parameters ask for the buffer: refused without one
        learn.collect(env, actor, critic, T, params=p, seed=SEED, counter0=C0)
    with pytest.raises(NotImplementedError, match="InitialStateBank"):
        actor.rollout(env, 1)
    er, er2 = learn.EpisodeReturns(env), learn.EpisodeReturns(env2)
    g, g2 = torch.Generator(device="cuda").manual_seed(9), torch.Generator(device="cuda").manual_seed(9)
    batch, infos, stats = learn.train_iteration(env, actor, critic, amod, cmod, opt, er, p, i_iter=1, seed=SEED, counter0=C0, generator=g, initial_states=bank)
    assert getattr(env, "_initial_states", None) is None  # detached again
    with bank2.attached():
        batch2 = learn.collect(env2, actor2, critic2, T, params=p2, seed=SEED, counter0=C0, returns=er2)
    infos2 = learn.update(env2, actor2, critic2, amod2, cmod2, opt2, batch2, params=p2, seed=SEED, counter0=C0, generator=g2)
    torch.cuda.synchronize()
    for k in ("slab", "advantage", "td_error", "observation", "action"):
        assert torch.equal(_bits(batch[k]), _bits(batch2[k])), k
    assert len(infos) == len(infos2) and all(torch.equal(_bits(a[k]), _bits(b[k])) for a, b in zip(infos, infos2) for k in a)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(list(amod.parameters()) + list(cmod.parameters()), list(amod2.parameters()) + list(cmod2.parameters())))
    got, want = _bank_words(bank), _bank_words(bank2)
    for k in got:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
    assert _same_envs(env, env2) == [] and batch["slab"][:, :, -1].sum().item() >= B
    for x in (bank, bank2, actor, actor2, env, env2):
        x.close()


# ---- 4. a run that really records ----------------------------------------------------------------------------------------------------------------
def test_a_run_that_really_records_and_restarts():
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.initial_states import InitialStateBank

    r = ic.RECORDING_RUN
    env = _env(r["N"], r["B"])
    env.reset_random(seed=r["seed"], counter=0)
    bank = InitialStateBank(env, capacity=r["capacity"], n_steps_stored=r["n_steps_stored"], probability_record=1.0, probability_use_recording=r["p_use"])
    act = torch.zeros(r["B"], r["N"], 2, device="cuda")
    act[..., 0] = capi.AGENTS["max_speed"]  # full speed, zero steering
    recorded = restarted = 0
    count = 0
    for t in range(r["T"]):
        env.step(act)
        bank.record(r["seed"], 1 + t)
        now = bank.count
        recorded += now - count  # (capacity 100 is never reached: count grows by R)
        count = now
        done = env.done.cpu().numpy()
        tw = ic.Twin(r["B"], r["N"], r["capacity"], r["n_steps_stored"], 1.0, r["p_use"])
        tw.count = count
        uses, j = tw.restart(done, r["seed"], 1 + t)
        bank.restart(r["seed"], 1 + t)
        env.sync()
        state, path = env.state.cpu().numpy(), env.buffer(capi.BUF_PATH).cpu().numpy()
        bs, bp = bank.view(capi.ISB_BANK_STATE).cpu().numpy(), bank.view(capi.ISB_BANK_PATH).cpu().numpy()
        for b in np.nonzero(uses)[0]:  # every restarted env's first post-reset rows are the chosen entry's
            assert np.array_equal(state[b].view(np.uint32), bs[j[b]].view(np.uint32)) and np.array_equal(path[b], bp[j[b]]), (t, b)
        assert not env.done.cpu().numpy()[uses].any() and env.done.cpu().numpy()[(done == 1) & ~uses].all()
        restarted += int(uses.sum())
        env.auto_reset(seed=r["seed"], counter=1 + t)
        bank.settle()
    print("recorded", recorded, "restarted", restarted)
    assert count < r["capacity"] and recorded >= 8 and restarted >= 2
    bank.close()
    env.close()
