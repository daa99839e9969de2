"""What no GPU test can see going wrong: the hand-over between torch's current stream and the env's stream (``SigmaEnv._on_stream``) -- its order, what a failing
call leaves undone -- and that every learner-side launch goes through that one statement with the tensors it must record.  Fake streams, a fake library whose
entry points return 0, small CPU tensors that claim to be CUDA ones.  No GPU needed.  Routes not reached here: ``Adam.step`` (its parameter checks walk real
modules' ``is_cuda``) and ``SigmaEnv.snapshot`` / ``restore`` (they need a real handle's layout); the GPU suites run them."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest
import torch

from sigmarl_amd import capi, learn
from sigmarl_amd.actor import Mlp32
from sigmarl_amd.env import SigmaEnv

B, N, D, T, M = 2, 2, 3, 4, 3
W = N * (D + 1) + 1


class Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(("wait", self.name, other.name))


class Recorded:
    """A tensor as far as ``_on_stream`` looks at one."""

    def __init__(self, name, log):
        self.name, self.log = name, log

    def record_stream(self, stream):
        self.log.append(("record", self.name, stream.name))


class Cuda(torch.Tensor):
    """A CPU tensor that passes the argument checks' ``is_cuda`` (the fake env's device is the CPU, so ``device ==`` holds as it is)."""
    is_cuda = True


def cuda(t):
    return t.as_subclass(Cuda)


class Lib:
    """Every entry point returns 0 and logs its name; ``codes`` overrides the code, ``prb_create`` hands out a handle."""
    path = "fake"

    def __init__(self, log, codes=None):
        self.log, self.codes = log, codes or {}

    def last_error(self, h):
        return b"the message"

    def prb_create(self, h, capacity, alpha, beta, eps, out):
        out._obj.value = 11
        return 0

    def __getattr__(self, name):
        def call(*args):
            self.log.append(("call", name, args))
            return self.codes.get(name, 0)
        return call


@pytest.fixture
def env(monkeypatch):
    log = []
    e = types.SimpleNamespace(device=torch.device("cpu"), stream=Stream("env", log), lib=Lib(log), h=5, B=B, N=N, D=D, K=1, log=log)
    e._chk = types.MethodType(SigmaEnv._chk, e)
    e._on_stream = lambda what, fn, tensors: SigmaEnv._on_stream(e, what, fn, tensors)  # (looked up per call: the routes below replace it)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream("current", log))
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return e


@pytest.fixture
def sites(env, monkeypatch):
    """``SigmaEnv._on_stream`` replaced by a recorder that still makes the call: ``[(what, tensors)]`` of every launch that went through it."""
    got = []

    def recorder(self, what, fn, tensors):
        assert self is env and fn() == 0
        got.append((what, list(tensors)))

    monkeypatch.setattr(SigmaEnv, "_on_stream", recorder)
    return got


def entry_points(env):
    return [name for kind, name, *_ in env.log if kind == "call"]


def same(got, want):
    """The recorded tensors are ``want``, one for one: the same objects, or (a ``detach`` / ``reshape`` in between) the same memory and shape."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g is w or (g.data_ptr() == w.data_ptr() and g.shape == w.shape and g.dtype == w.dtype)


def test_on_stream_order(env):
    a, b = Recorded("a", env.log), Recorded("b", env.log)
    env._on_stream("x", lambda: env.lib.x(1, 2), (a, b))
    assert env.log == [("wait", "env", "current"), ("call", "x", (1, 2)), ("wait", "current", "env"), ("record", "a", "env"), ("record", "b", "env")]


def test_on_stream_failure_raises_before_the_second_wait_and_records_nothing(env):
    env.lib.codes["x"] = 7
    with pytest.raises(RuntimeError) as err:
        env._on_stream("x", lambda: env.lib.x(), (Recorded("a", env.log),))
    assert str(err.value) == "sigmaenv_x failed with code 7: the message"
    assert env.log == [("wait", "env", "current"), ("call", "x", ())]


@pytest.mark.parametrize("what, width, args", [("ppo_head", 4, capi.PpoHeadArgs), ("ppo_head_1d", 2, capi.PpoHead1dArgs)])
def test_ppo_head_function(env, sites, what, width, args):
    a, keep = args(), (torch.zeros(M, dtype=torch.int32), torch.zeros(T, B, N))
    out, value = torch.zeros((M, N, width), requires_grad=True), torch.zeros((M,), requires_grad=True)
    loss, result = learn._PpoHeadFunction.apply(env, what, a, keep, out, value)
    assert entry_points(env) == [what] and [w for w, _ in sites] == [what]
    ts = sites[0][1]
    same(ts[:2] + ts[6:], [out, value, *keep])
    assert [tuple(t.shape) for t in ts[2:6]] == [(M, N, width), (M,), (8,), (capi.PPO_SUMS * ((M * N + 255) // 256),)] and ts[4] is result
    assert [a.out, a.value, a.dout_actor, a.dout_critic, a.result, a.workspace] == [t.data_ptr() for t in ts[:6]]  # what the call touches is what is recorded
    assert loss.requires_grad and not result.requires_grad
    gout, gvalue = torch.autograd.grad(loss, (out, value))
    assert gout.shape == out.shape and gvalue.shape == value.shape


def test_episode_returns_update(env, sites):
    er, slab = learn.EpisodeReturns(env), cuda(torch.zeros((T, B, W)))
    rec, stats = er.update(slab)
    none, _ = er.update(slab, episode_reward=False)
    assert entry_points(env) == ["episode_return"] * 2 and [w for w, _ in sites] == ["episode_return"] * 2
    same(sites[0][1], [slab, er.carry, stats["episode_reward_mean"]._base, rec])
    assert none is None and len(sites[1][1]) == 3 and sites[1][1][:2] == [slab, er.carry]


def test_prioritized_buffer_extend_sample_refresh(env, sites):
    buf = learn.PrioritizedBuffer(env, T * B)
    td0 = cuda(torch.rand((T, B)))
    buf.extend(td0)
    index, weight = buf.sample(M, 1, 0)
    sv, nv = torch.zeros(M), torch.ones(M)
    values = iter((sv, nv))
    critic = types.SimpleNamespace(apply=lambda env, record, **kw: next(values))
    batch = {"observation": cuda(torch.zeros((T, B, N, D))), "slab": cuda(torch.zeros((T, B, W)))}
    index = cuda(index)
    td = buf.refresh(critic, batch, index)
    assert entry_points(env) == ["prb_extend", "prb_sample", "prb_refresh"] and [w for w, _ in sites] == ["prb_extend", "prb_sample", "prb_refresh"]
    same(sites[0][1], [td0])
    same(sites[1][1], [index, weight])
    same(sites[2][1], [index, sv, nv, batch["slab"], td])
    assert not hasattr(buf, "_call")


@pytest.fixture
def net(env):
    m = Mlp32.__new__(Mlp32)
    m._keep, m.in_dim, m.out_dim, m._input_grad = (np.asarray([D, 256, 256, 2], np.int32), [None] * 3, [None] * 3), D, 2, True
    m._handles, m._handle_version, m._version = {env.lib.path: (env.lib, 7)}, {env.lib.path: 0}, 0
    return m


def specs():
    base, index = torch.zeros((T * B, D)), torch.zeros((M,), dtype=torch.int32)
    return {"": (base, 0, B, D, T, B * D, None), "_indexed": (base, 0, B, D, T, B * D, index), "_indexed_pad": (base, 0, B, 1, T, B, index, (1, D))}


@pytest.mark.parametrize("suffix", ["", "_indexed", "_indexed_pad"])
def test_mlp32_forward_save_and_backward(env, sites, net, suffix):
    spec = specs()[suffix]
    base, index = spec[0], spec[6]
    n = B * (T if index is None else M)
    y, acts = net._forward_save(env, spec)
    dout = torch.ones((n, 2))
    gw, gb = net._backward(env, spec, acts, dout)
    assert entry_points(env) == ["mlp32_forward_save" + suffix, "mlp32_backward_workspace", "mlp32_backward" + suffix]
    assert [w for w, _ in sites] == ["mlp32_forward_save" + suffix, "mlp32_backward" + suffix]
    assert y.shape == (n, 2) and acts.shape == (2, n, 256) and [tuple(g.shape) for g in gw + gb] == [(256, D), (256, 256), (2, 256), (256,), (256,), (2,)]
    picked = [] if index is None else [index]
    same(sites[0][1], [base, y, acts] + picked)
    same(sites[1][1][:3] + sites[1][1][4:], [base, acts, dout] + gw + gb + picked)
    assert sites[1][1][3].shape == (4,)  # the workspace
    assert all(args[:2] == (env.h, 7) for kind, name, args in env.log if name != "mlp32_backward_workspace")


@pytest.mark.parametrize("want_params, want_dx, what", [(True, True, "mlp32_backward_dx"), (False, True, "mlp32_input_grad"), (True, False, "mlp32_backward"),
                                                       (False, False, None)])
def test_mlp32_backward_entry_point_by_case(env, sites, net, want_params, want_dx, what):
    spec = specs()[""]
    acts, dout = torch.zeros((2, T * B, 256)), torch.ones((T * B, 2))
    gw, gb, dx = net._backward_dx(env, spec, acts, dout, want_params, want_dx)
    assert [w for w, _ in sites] == ([what] if what else []) and entry_points(env)[1:] == ([what] if what else [])
    assert (gw is not None) == (gb is not None) == want_params and (dx is not None) == want_dx
    if what:
        same(sites[0][1][:3] + sites[0][1][4:], [spec[0], acts, dout] + ([dx] if want_dx else []) + (gw + gb if want_params else []))
    net._input_grad = False  # a handle made without input_grad launches what it did, and refuses dx
    if want_dx:
        with pytest.raises(RuntimeError, match="input_grad=True"):
            net._backward_dx(env, spec, acts, dout, want_params, want_dx)
    else:
        net._backward_dx(env, spec, acts, dout, want_params, want_dx)
        assert [w for w, _ in sites] == ([what] * 2 if what else [])
