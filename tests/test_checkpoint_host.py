"""sigmarl_amd.checkpoint on the host (CPU tensors only, no GPU): the file's round trip, the temporary-name-then-os.replace discipline (a writer that raises midway
leaves the old file intact and no temporary behind), every refusal naming its field, export_reference's files loading into a fresh module of the reference's shape,
and learn.Adam.state_dict through to_torch / from_torch unchanged.  The device objects are built by hand (object.__new__) around CPU tensors: nothing here launches."""
import contextlib
import os
import types

import pytest
import torch

from sigmarl_amd import checkpoint as ck
from sigmarl_amd import learn
from sigmarl_amd.actor import make_mlp
from sigmarl_amd.env import Snapshot
from sigmarl_amd.params import Parameters


def cpu_adam(modules, seed, t=7, lr=1.5e-4):
    """A learn.Adam around CPU modules with random moments (no env, no device network: state_dict / load_state_dict / to_torch / from_torch touch neither)"""
    g = torch.Generator().manual_seed(seed)
    a = object.__new__(learn.Adam)
    a.env, a.lr, a.betas, a.eps, a.t = types.SimpleNamespace(device=torch.device("cpu")), lr, (0.9, 0.999), 1e-8, t
    a.networks = [(None, m) for m in modules]
    a.state = [[(torch.randn(p.shape, generator=g), torch.rand(p.shape, generator=g)) for p in m.parameters()] for m in modules]
    a._result = None
    return a


def zero_adam(modules):
    a = cpu_adam(modules, 0, t=0, lr=0.0)
    for mom in a.state:
        for m, v in mom:
            m.zero_()
            v.zero_()
    return a


def run_objects(seed, with_priority=True):
    torch.manual_seed(seed)
    modules = {"policy": make_mlp(32, 16, 4), "critic": make_mlp(128, 16, 1)}
    if with_priority:
        modules.update(priority_policy=make_mlp(32, 16, 2), priority_critic=make_mlp(128, 16, 1))
    optims = {"base": cpu_adam([modules["policy"], modules["critic"]], seed + 1)}
    if with_priority:
        optims["priority"] = cpu_adam([modules["priority_policy"], modules["priority_critic"]], seed + 2, t=3)
    returns = object.__new__(learn.EpisodeReturns)
    returns.env, returns.carry = None, torch.randn(8, 4)
    snap = Snapshot(dict(magic=0x50414E53, version=1, n_envs=8, n_agents=4, n_nearing=2, obs_dim=32, n_short_term=3, obs_flags=0, cbf=0, observe_calls=2,
                         cbf_groups_valid=0, total_bytes=64), torch.randint(0, 256, (64,), dtype=torch.uint8), reset_counter=5)
    gen = torch.Generator().manual_seed(seed + 3)
    torch.rand(3, generator=gen)
    return modules, optims, returns, snap, gen


def small_params(**kw):
    return Parameters(n_agents=4, num_vmas_envs=8, max_steps=8, minibatch_size=32, num_epochs=2, n_iters=4, is_obs_noise=False, **kw)


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return a == b


def test_the_file_round_trips(tmp_path):
    modules, optims, returns, snap, gen = run_objects(1)
    p = small_params()
    p.episode_reward_intermediate, p.episode_reward_mean_current = -1.25, -1.25
    means = [float("nan"), -1.25]
    path = tmp_path / "run.ckpt"
    wrote = ck.save(path, env=snap, modules=modules, optims=optims, returns=returns, i_iter=2, seed=9, counter0=100, params=p, means=means, generator=gen,
                    extra={"note": "x", "t": torch.arange(3)})
    assert os.listdir(tmp_path) == ["run.ckpt"]  # no temporary left
    got = ck.load(path)
    assert same(got, wrote) and got["format"] == ck.FORMAT
    assert got["i_iter"] == 2 and got["next_iter"] == 3 and got["seed"] == 9 and got["counter0"] == 100
    assert got["means"][0] != got["means"][0] and got["means"][1] == -1.25  # the NaN's position survives
    assert all(not t.is_cuda for t in [got["env"]["blob"], got["returns"]["carry"]])
    # into new objects built from nothing but the Parameters
    m2, o2, r2, _, g2 = run_objects(50)
    p2 = small_params()
    ck.restore(got, modules=m2, optims=o2, returns=r2, params=p2, generator=g2)
    for k in modules:
        assert same(dict(modules[k].state_dict()), dict(m2[k].state_dict())), k
    for k in optims:
        assert same(optims[k].state_dict(), o2[k].state_dict()), k
    assert o2["base"].t == 7 and o2["priority"].t == 3 and o2["base"].lr == 1.5e-4
    assert torch.equal(r2.carry, returns.carry)
    assert torch.equal(torch.rand(5, generator=g2), torch.rand(5, generator=gen))  # the generators go on alike
    assert (p2.episode_reward_intermediate, p2.episode_reward_mean_current) == (-1.25, -1.25)
    s2 = Snapshot.from_state_dict(got["env"])
    assert s2.header == snap.header and torch.equal(s2.blob, snap.blob) and s2.reset_counter == 5
    assert ck.saved_parameters(got).to_dict() == p.to_dict()


def test_an_interrupted_write_leaves_the_old_file_intact(tmp_path):
    modules, optims, returns, snap, gen = run_objects(2, with_priority=False)
    p = small_params()
    path = tmp_path / "run.ckpt"
    kw = dict(env=snap, modules=modules, optims=optims, returns=returns, seed=0, counter0=0, params=p, means=[0.5])
    ck.save(path, i_iter=1, **kw)
    old = path.read_bytes()

    def dies_midway(obj, f):
        f.write(b"half a file")
        f.flush()
        assert sorted(os.listdir(tmp_path)) != ["run.ckpt"]  # the bytes go to another name in the same directory
        raise OSError("disk full")

    with pytest.raises(OSError, match="disk full"):
        ck.save(path, i_iter=2, writer=dies_midway, **kw)
    assert path.read_bytes() == old and os.listdir(tmp_path) == ["run.ckpt"] and ck.load(path)["i_iter"] == 1
    seen = []
    real_replace = os.replace

    def spy(src, dst):
        seen.append((os.path.dirname(src) == os.path.dirname(dst), os.path.exists(src), os.fspath(dst)))
        real_replace(src, dst)

    os.replace = spy
    try:
        ck.save(path, i_iter=2, **kw)
    finally:
        os.replace = real_replace
    assert seen == [(True, True, str(path))] and ck.load(path)["i_iter"] == 2
    (tmp_path / "other.bin").write_bytes(b"not a checkpoint")
    with pytest.raises(Exception):
        ck.load(tmp_path / "other.bin")
    torch.save({"format": "something/0"}, tmp_path / "foreign.ckpt")
    with pytest.raises(ValueError, match="something/0"):
        ck.load(tmp_path / "foreign.ckpt")


@pytest.mark.parametrize("field,value", [
    ("n_agents", 5), ("is_obs_steering", True), ("is_ego_view", False), ("is_observe_distance_to_boundaries", False), ("is_using_opponent_modeling", True),
    ("n_nearing_agents_observed", 1), ("num_vmas_envs", 16), ("max_steps", 4), ("minibatch_size", 16), ("num_epochs", 3), ("n_iters", 5), ("gamma", 0.9),
    ("lmbda", 0.8), ("lr", 1e-3), ("lr_min", 1e-6)])
def test_a_file_of_other_parameters_is_refused_by_name(tmp_path, field, value):
    modules, optims, returns, snap, gen = run_objects(3, with_priority=False)
    p = small_params()
    path = tmp_path / "run.ckpt"
    ck.save(path, env=snap, modules=modules, optims=optims, returns=returns, i_iter=1, seed=0, counter0=0, params=p, means=[])
    other = Parameters(**{**p.to_dict(), field: value})
    named = "frames_per_batch" if field in ("num_vmas_envs", "max_steps") else field
    before = {k: v.clone() for k, v in modules["policy"].state_dict().items()}
    m2 = run_objects(4, with_priority=False)[0]
    theirs = {k: v.clone() for k, v in m2["policy"].state_dict().items()}
    with pytest.raises(ValueError, match=rf"\b{named} = "):
        ck.restore(ck.load(path), modules=m2, params=other)
    assert same(dict(m2["policy"].state_dict()), theirs) and same(dict(modules["policy"].state_dict()), before)  # refused before anything changed
    ck.restore(ck.load(path), modules=m2, params=Parameters(**{**p.to_dict(), "where_to_save": "elsewhere/", "episode_reward_intermediate": 3.0}))  # not a shaping field


def test_the_other_refusals_name_what_is_wrong(tmp_path):
    modules, optims, returns, snap, gen = run_objects(5, with_priority=False)
    p = small_params()
    path = tmp_path / "run.ckpt"
    kw = dict(env=snap, returns=returns, i_iter=1, seed=0, counter0=0, params=p, means=[])
    with pytest.raises(ValueError, match="actor"):
        ck.save(path, modules={"actor": modules["policy"]}, optims=optims, **kw)
    with pytest.raises(TypeError, match="'base'.*learn.Adam"):
        ck.save(path, modules=modules, optims={"base": torch.optim.Adam(modules["policy"].parameters())}, **kw)
    assert not path.exists()
    ck.save(path, modules=modules, optims=optims, **kw)
    got = ck.load(path)
    m_all, o_all, r2, _, g2 = run_objects(6, with_priority=True)
    with pytest.raises(KeyError, match="priority_policy"):
        ck.restore(got, modules=m_all)
    with pytest.raises(KeyError, match="priority"):
        ck.restore(got, optims=o_all)
    with pytest.raises(KeyError, match="generator"):
        ck.restore(got, generator=g2)
    with pytest.raises(KeyError, match="initial-state bank"):
        ck.restore(got, initial_states=object())
    with pytest.raises(ValueError, match="'policy'.*without its torch module"):
        ck.restore(got, networks={"policy": object()})
    # learn.Adam refuses other shapes, naming the tensor, before it copies anything
    wide = cpu_adam([make_mlp(32, 24, 4), modules["critic"]], 1)
    mine = wide.state_dict()
    with pytest.raises(ValueError, match="exp_avg of network 0 parameter 0"):
        wide.load_state_dict(got["optims"]["base"])
    assert same(wide.state_dict(), mine)
    with pytest.raises(ValueError, match="1 networks in the dict, 2 here"):
        wide.load_state_dict({**got["optims"]["base"], "state": got["optims"]["base"]["state"][:1]})
    with pytest.raises(ValueError, match="carry"):
        r2.load_state_dict({"carry": torch.zeros(3, 4)})
    with pytest.raises(ValueError, match="start_iter"):
        learn.train(None, None, None, None, None, None, p, start_iter=0)
    with pytest.raises(ValueError, match="checkpoint="):
        learn.train(None, None, None, None, None, None, p, checkpoint_every=2)


def test_export_reference_files_load_into_a_fresh_module(tmp_path):
    modules = run_objects(7)[0]
    out = ck.export_reference(tmp_path / "outputs", modules=modules)
    assert sorted(os.listdir(tmp_path / "outputs")) == ["final_critic.pth", "final_policy.pth", "final_priority_critic.pth", "final_priority_policy.pth"]
    fresh = {"policy": make_mlp(32, 16, 4), "critic": make_mlp(128, 16, 1), "priority_policy": make_mlp(32, 16, 2), "priority_critic": make_mlp(128, 16, 1)}
    for name, path in out.items():
        sd = torch.load(path, map_location="cpu", weights_only=True)  # plain tensors: loads under torch's safe loader
        fresh[name].load_state_dict(sd, strict=True)
        assert same(dict(fresh[name].state_dict()), dict(modules[name].state_dict())), name
    renamed = ck.export_reference(tmp_path / "wrapped", modules={"policy": modules["policy"]}, rename=lambda k: "module.0." + k)
    assert set(torch.load(renamed["policy"], weights_only=True)) == {"module.0." + k for k in modules["policy"].state_dict()}
    with pytest.raises(ValueError, match="actor"):
        ck.export_reference(tmp_path, modules={"actor": modules["policy"]})


def test_adam_state_dict_through_to_torch_and_from_torch_unchanged(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())  # (to_torch enters the env's device: there is none here)
    modules = [make_mlp(8, 6, 2), make_mlp(5, 6, 1)]
    a = cpu_adam(modules, 21, t=11)
    sd = a.state_dict()
    optim = torch.optim.Adam([p for m in modules for p in m.parameters()], lr=a.lr)
    a.to_torch(optim)
    b = zero_adam(modules)
    b.from_torch(optim)
    b.lr = a.lr
    assert same(b.state_dict(), sd) and b.t == 11
    assert all(x is not y for mom_a, mom_b in zip(a.state, b.state) for qa, qb in zip(mom_a, mom_b) for x, y in zip(qa, qb))  # copies
    sd["state"][0][0][0].add_(1.0)  # a state_dict is a copy: the optimiser does not move with it
    assert not same(a.state_dict(), sd)
    c = zero_adam(modules)
    c.load_state_dict(a.state_dict())
    assert same(c.state_dict(), a.state_dict())
