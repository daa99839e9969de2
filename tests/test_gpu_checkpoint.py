"""Stop and go on: ``learn.train`` for 4 iterations straight against 2 iterations with ``checkpoint=``, then NEW env, modules, networks, optimisers, returns,
generator (and buffer / bank) built from nothing but the ``Parameters``, then ``learn.resume`` for iterations 3-4 -- 4 agents x 8 envs, 64 frames per batch,
minibatches of 32, 2 epochs.  Bit for bit equal: the list of episode means (NaN positions included), every parameter and both Adam moments of every network, ``t`` and
``lr``, the env snapshot, the ``EpisodeReturns`` carry, the last iteration's ``batch["slab"]``, the networks' arithmetic modes.  Once plain, once with ``is_prb``,
once with ``priority=(...)`` under ``wrapper="prioritized"``, once with an initial-state bank.  The file written after iteration 4 (``checkpoint_every=2``) equals the
straight run's state.  With the defaults ``train`` writes nothing and takes no snapshot."""
import os

import pytest

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)
B, SEED, C0 = 8, 4, 100
KINDS = {"plain": {}, "prb": dict(is_prb=True), "priority": dict(is_using_prioritized_marl=True), "bank": dict(is_challenging_initial_state_buffer=True)}


def _params(kind):
    from sigmarl_amd.params import Parameters

    p = Parameters(n_agents=4, num_vmas_envs=B, max_steps=8, n_iters=4, num_epochs=2, minibatch_size=32, lr=3e-4, lr_min=1e-5, **KW, **KINDS[kind])
    assert p.frames_per_batch == 64
    return p


def _bits(t):
    import torch

    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


class Run:
    """every object of a run, from the Parameters alone; ``fresh``: other initial weights, another placement of the agents, another generator seed"""

    def __init__(self, kind, fresh=False):
        import torch
        from sigmarl_amd import capi, learn
        from sigmarl_amd.actor import Actor, Critic, PriorityNet, make_mlp, make_priority_mlp
        from sigmarl_amd.env import SigmaEnv
        from sigmarl_amd.initial_states import InitialStateBank

        self.kind, self.p = kind, _params(kind)
        p = self.p
        self.env = env = SigmaEnv(p, n_envs=B, device="cuda:0")
        env.reset_random(seed=55 if fresh else 3)
        N, D, K = env.N, env.D, env.K
        Dc = D + 2 * K if kind == "priority" else D
        torch.manual_seed(123 if fresh else 1)
        self.modules = {"policy": make_mlp(Dc).cuda(), "critic": make_mlp(N * Dc, n_out=1).cuda()}
        self.actor, self.critic = Actor(self.modules["policy"], low=LOW, high=HIGH), Critic(self.modules["critic"])
        self.optim = learn.Adam(env, [(self.actor, self.modules["policy"]), (self.critic, self.modules["critic"])], lr=p.lr)
        self.optims, self.networks = {"base": self.optim}, {"policy": self.actor, "critic": self.critic}
        self.kw = dict(seed=SEED, counter0=C0, generator=torch.Generator(device="cuda").manual_seed(77 if fresh else 9))
        if kind == "priority":
            self.modules.update(priority_policy=make_priority_mlp(D).cuda(), priority_critic=make_mlp(N * D, n_out=1).cuda())
            self.pn, self.pc = PriorityNet(self.modules["priority_policy"]), Critic(self.modules["priority_critic"])
            self.optims["priority"] = learn.Adam(env, [(self.pn, self.modules["priority_policy"]), (self.pc, self.modules["priority_critic"])], lr=p.lr)
            self.networks.update(priority_policy=self.pn, priority_critic=self.pc)
            self.kw.update(rollout_kw=dict(wrapper="prioritized"), priority=(self.pn, self.pc, self.modules["priority_policy"], self.modules["priority_critic"], self.optims["priority"]))
        self.returns = learn.EpisodeReturns(env)
        self.buffer = learn.PrioritizedBuffer(env, p.frames_per_batch) if kind == "prb" else None
        self.bank = None
        if kind == "bank":
            self.bank = InitialStateBank(env, capacity=3, n_steps_stored=3, probability_use_recording=0.5)
            if not fresh:
                self.bank.load(env.state[:2].clone(), env.buffer(capi.BUF_PATH)[:2].clone())  # two scenes to restart from, from the first step on
        self.last = {}

    def args(self):
        return (self.env, self.actor, self.critic, self.modules["policy"], self.modules["critic"], self.optim, self.p)

    def train_kw(self):
        def on_iteration(i_iter, batch, infos, mean, improved):
            self.last = dict(i_iter=i_iter, slab=batch["slab"].clone(), lr_seen=self.optim.lr)

        return dict(self.kw, on_iteration=on_iteration, returns=self.returns, buffer=self.buffer, initial_states=self.bank)

    def state(self):
        """everything the next iteration depends on, on the host"""
        import torch

        torch.cuda.synchronize()
        snap = self.env.snapshot().cpu()
        st = {"env_blob": snap.blob, "carry": self.returns.carry.cpu(), "slab": self.last["slab"].cpu()}
        for k, m in self.modules.items():
            for n, t in m.state_dict().items():
                st[f"module {k} {n}"] = t.cpu()
        for k, o in self.optims.items():
            for a, mom in enumerate(o.state):
                for i, (m, v) in enumerate(mom):
                    st[f"optim {k} {a} {i} exp_avg"], st[f"optim {k} {a} {i} exp_avg_sq"] = m.cpu(), v.cpu()
        if self.bank is not None:
            st.update({f"bank {k}": v.cpu() for k, v in self.bank.state_dict().items() if isinstance(v, torch.Tensor)})
        plain = {"env_header": snap.header, "reset_counter": snap.reset_counter, "t": {k: o.t for k, o in self.optims.items()}, "lr": {k: o.lr for k, o in self.optims.items()},
                 "modes": {k: (n._mlp32.mode if hasattr(n, "_mlp32") else n.mode) for k, n in self.networks.items()},
                 "best": self.p.episode_reward_intermediate, "current": self.p.episode_reward_mean_current, "generator": self.kw["generator"].get_state().tolist()}
        return st, plain

    def close(self):
        for x in (self.buffer, self.bank, *self.networks.values(), self.env):
            if x is not None:
                x.close()


def same_means(a, b):
    return len(a) == len(b) and all(x == y or (x != x and y != y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_resumed_run_is_the_run_that_was_never_stopped(kind, tmp_path, monkeypatch):
    import torch
    from sigmarl_amd import checkpoint as ck
    from sigmarl_amd import learn

    # 4 iterations straight, with the defaults: no file, no snapshot
    straight = Run(kind)
    with monkeypatch.context() as m:
        m.setattr(type(straight.env), "snapshot", lambda *a, **k: pytest.fail("train() took a snapshot with the defaults"))
        means = learn.train(*straight.args(), **straight.train_kw())
    assert os.listdir(tmp_path) == [] and len(means) == 4 and straight.last["i_iter"] == 4
    want, want_plain = straight.state()
    # 2 iterations with checkpoint=
    path = tmp_path / "run.ckpt"
    first = Run(kind)
    means2 = learn.train(*first.args(), n_iters=2, checkpoint=path, checkpoint_every=2, **first.train_kw())
    assert os.listdir(tmp_path) == ["run.ckpt"] and same_means(means2, means[:2])
    at2 = ck.load(path)
    assert at2["i_iter"] == 2 and at2["next_iter"] == 3 and same_means(at2["means"], means[:2]) and at2["seed"] == SEED and at2["counter0"] == C0
    assert at2["optims"]["base"]["lr"] == learn.lr_at(first.p, 3) == first.optim.lr  # written AFTER set_lr: the moment before iteration 3
    assert sorted(at2["modules"]) == sorted(first.modules) and sorted(at2["optims"]) == sorted(first.optims)
    assert (at2["initial_states"] is not None) == (kind == "bank") and at2["generator"] is not None
    first.close()
    # new objects from nothing but the Parameters, then iterations 3-4
    again = Run(kind, fresh=True)
    kw = again.train_kw()
    for k in ("seed", "counter0"):  # (the file's)
        kw.pop(k)
    means4 = learn.resume(path, *again.args(), checkpoint=path, checkpoint_every=2, **kw)
    assert same_means(means4, means), (means4, means)
    assert again.last["i_iter"] == 4
    got, got_plain = again.state()
    assert sorted(got) == sorted(want)
    assert [k for k in want if not same(got[k], want[k])] == []
    assert got_plain == want_plain, (got_plain, want_plain)
    assert got_plain["t"]["base"] == 4 * learn.steps_per_iteration(straight.p, 64) == 16 and got_plain["lr"]["base"] == learn.lr_at(straight.p, 5)
    # the file written after iteration 4 equals the straight run's state
    at4 = ck.load(path)
    assert at4["i_iter"] == 4 and same_means(at4["means"], means)
    assert same(at4["env"]["blob"], want["env_blob"]) and at4["env"]["header"] == want_plain["env_header"] and same(at4["returns"]["carry"], want["carry"])
    for k, m in straight.modules.items():
        assert all(same(at4["modules"][k][n], t) for n, t in m.state_dict().items()), k
    for k, o in straight.optims.items():
        sd = at4["optims"][k]
        assert sd["t"] == o.t and sd["lr"] == o.lr
        assert all(same(x, y) for mom, mom2 in zip(sd["state"], o.state) for q, q2 in zip(mom, mom2) for x, y in zip(q, q2)), k
    assert ck.saved_parameters(at4).episode_reward_intermediate == straight.p.episode_reward_intermediate
    assert at4["generator"].tolist() == want_plain["generator"]
    if kind == "bank":
        assert all(same(v, want[f"bank {k}"]) for k, v in at4["initial_states"].items() if isinstance(v, torch.Tensor))
        assert int(straight.last["slab"][:, :, -1].sum().item()) >= 1  # envs finished: the restarts and resets ran
    # the run moved: the weights of iteration 2 are not those of iteration 4
    assert not same(at2["modules"]["policy"]["0.weight"], at4["modules"]["policy"]["0.weight"]) and not same(at2["env"]["blob"], at4["env"]["blob"])
    straight.close()
    again.close()


def test_resume_refuses_a_file_of_other_parameters_before_it_touches_anything(tmp_path):
    import torch
    from sigmarl_amd import learn

    run = Run("plain")
    path = tmp_path / "run.ckpt"
    learn.train(*run.args(), n_iters=1, checkpoint=path, checkpoint_every=1, **run.train_kw())
    run.p.minibatch_size = 16
    blob, w = run.env.snapshot().blob.clone(), run.modules["policy"][0].weight.detach().clone()
    with pytest.raises(ValueError, match="minibatch_size = 32, this run has minibatch_size = 16"):
        learn.resume(path, *run.args(), **{k: v for k, v in run.train_kw().items() if k not in ("seed", "counter0")})
    torch.cuda.synchronize()
    assert torch.equal(run.env.snapshot().blob, blob) and torch.equal(run.modules["policy"][0].weight.detach(), w)
    with pytest.raises(TypeError, match="learn.Adam"):  # a torch optimiser owns its moments: refused before the first iteration
        learn.train(run.env, run.actor, run.critic, run.modules["policy"], run.modules["critic"], torch.optim.Adam(run.modules["policy"].parameters()), run.p, n_iters=1,
                    checkpoint=path, checkpoint_every=1, seed=SEED, counter0=C0)
    torch.cuda.synchronize()
    assert torch.equal(run.env.snapshot().blob, blob)
    run.close()
