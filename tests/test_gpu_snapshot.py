"""Snapshot and restore of an env handle on the device (sigmaenv_state_save / _restore, ``SigmaEnv.snapshot`` / ``restore``), compared as words, never with a tolerance.

Whole snapshot: 8 steps, a snapshot, 8 more steps with the record kept; a FRESH handle of the same configuration that has been stepped 5 steps under another seed takes
the snapshot and steps the same 8 steps under the same keys: its record rows, every ``sigmaenv_get`` buffer and its own snapshot (every device word of the state, the
ones ``sigmaenv_get`` does not reach included) at the end are bit for bit the first run's.  Shapes: 4 agents x 6 envs on intersection_4 (entry / exit resets, a
partial tile), 16 x 5 on CPM, 4 x 130 (more than one workgroup of 16-byte pieces per segment, an env count that is no multiple of any tile), 64 x 2; then, at 4 x 6:
the mtv distance, observation noise, boundary points (snapshot on a step that re-placed envs), the CBF-QP chain with grouping, the QP-free margin reward,
``Actor.rollout`` with ``wrapper="prioritized"`` and communication noise, and an ``InitialStateBank`` attached with p_use = 0.5 (restored through its
``load_state_dict``).
Masked restore: a third of the envs (env 0, env B - 1, two neighbours of one wavefront tile) rewound from S repeat their 8 steps bit for bit while, right after the
restore, every word of every other env is what it was; an all-zero mask changes no word, an all-ones mask equals the unmasked restore in every device word.
Guard bytes around the blob survive ``save``; a wrong size, a misaligned blob and a header of another shape are refused on the return path, nothing changed."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
KW = dict(is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=5)
SEED, T0, T1 = 5, 8, 8

SHAPES = {
    "4x6_intersection_4": dict(N=4, B=6, scen="intersection_4"),
    "16x5_cpm": dict(N=16, B=5, scen="cpm_entire"),
    "4x130_cpm": dict(N=4, B=130, scen="cpm_entire"),
    "64x2_cpm": dict(N=64, B=2, scen="cpm_entire"),
}
CBF = dict(rew_method="cbf", is_using_cbf_training=True, dt=0.05)
VARIANTS = {
    "mtv_distance": dict(pkw=dict(is_use_mtv_distance=True)),
    "observation_noise": dict(pkw=dict(is_obs_noise=True)),
    "boundary_points": dict(pkw=dict(is_observe_distance_to_boundaries=False), replaced=True),
    "cbf_qp_grouped": dict(pkw=dict(CBF, is_solve_qp=True, is_apply_cbf_action=True, is_grouping_agents=True, max_group_size=2), drive="cbf_qp"),
    "cbf_margin_reward": dict(pkw=dict(CBF, is_solve_qp=False), drive="cbf_rewards"),
    "prioritized_rollout_comm_noise": dict(pkw=dict(is_using_prioritized_marl=True), drive="rollout", in_extra=True,
                                           roll=dict(wrapper="prioritized", priority="random", communication_noise=0.1)),
    "initial_state_bank": dict(pkw=dict(), drive="rollout", roll=dict(), bank=True),
}


def _env(N, B, scen="cpm_entire", **pkw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    kw = dict(KW, n_agents=N, scenario_type=scen)
    kw.update(pkw)
    return SigmaEnv(Parameters(**kw), n_envs=B, device="cuda:0")


def _actor(env, in_extra=False):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp

    torch.manual_seed(1)
    mlp = make_mlp(env.D + (2 * env.K if in_extra else 0))
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    return Actor(mlp, low=LOW, high=HIGH)


def _bits(t):
    import torch

    return t.contiguous().reshape(-1).view(torch.uint8)


def _actions(env, seed=6):
    """[T0 + T1, B, N, 2] random commands: speed in [-0.2, 1.2), steering in [-0.5, 0.5)"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    n = T0 + T1
    return torch.stack([torch.rand(n, env.B, env.N, generator=g, device="cuda") * 1.4 - 0.2, torch.rand(n, env.B, env.N, generator=g, device="cuda") - 0.5], -1).contiguous()


def _words(env):
    """every sigmaenv_get buffer as bytes (copies)"""
    from sigmarl_amd.env import _buf_layout

    env.sync()
    return {w: _bits(env.buffer(w)).clone() for w in _buf_layout(env.B, env.N, env.K, env.D)}


def _env_words(env, words, envs):
    """the bytes of the envs `envs` (a bool [B] tensor) of every buffer: [B, ...] buffers by their first axis, SIGMAENV_BUF_REWARD_INFO [12, B, N] by its second"""
    from sigmarl_amd import capi

    out = {}
    for w, t in words.items():
        out[w] = t.reshape(12, env.B, -1)[:, envs] if w == capi.BUF_REWARD_INFO else t.reshape(env.B, -1)[envs]
    return out


class Drive:
    """steps t0 .. t0 + T of one of the per-step chains, keyed (seed, t); returns the record [T, B, W]"""

    def __init__(self, kind, acts=None, actor=None, roll=None, bank=None):
        self.kind, self.acts, self.actor, self.roll, self.bank = kind, acts, actor, roll or {}, bank

    def __call__(self, env, t0, T, seed=SEED, bank=None):
        import contextlib

        import torch

        slab = torch.zeros(T, env.B, env.N * (env.D + 1) + 1, device="cuda")
        if self.kind == "n":
            env.step_autoreset_n(self.acts[t0: t0 + T].contiguous(), slab, seed=seed, counter0=t0)
        elif self.kind == "rollout":
            with (bank.attached() if bank is not None else contextlib.nullcontext()):
                self.actor.rollout(env, T, slab=slab, seed=seed, counter0=t0, **self.roll)
        else:
            for t in range(T):
                act = self.acts[t0 + t].contiguous()
                env.set_slab(slab[t])
                if self.kind == "cbf_qp":
                    env.step(env.cbf_qp(act))
                else:
                    env.cbf_rewards(act)
                    env.step(act)
                env.auto_reset(seed=seed, counter=t0 + t)
            env.set_slab(None)
        env.sync()
        return slab


def _whole(N, B, scen="cpm_entire", pkw=None, drive="n", roll=None, in_extra=False, bank=False, replaced=False):
    import torch
    from sigmarl_amd import capi
    from sigmarl_amd.initial_states import InitialStateBank

    pkw = pkw or {}
    a, b = _env(N, B, scen, **pkw), _env(N, B, scen, **pkw)
    actor = _actor(a, in_extra) if drive == "rollout" else None
    go = Drive(drive, _actions(a), actor, roll)
    other = Drive(drive, _actions(a, seed=99), actor, roll)
    banks = [InitialStateBank(e, capacity=3, n_steps_stored=3, probability_use_recording=0.5) for e in (a, b)] if bank else [None, None]
    a.reset_random(seed=3, counter=1000)
    b.reset_random(seed=77, counter=2000)
    for e in (a, b):
        if drive in ("cbf_qp", "cbf_rewards"):
            e.cbf_attach()
    if bank:
        banks[0].load(a.state[:2].clone(), a.buffer(capi.BUF_PATH)[:2].clone())  # two scenes to restart from, from the first step on
        banks[1].reset()
    t_snap = T0
    if replaced:  # `fresh` matters right after a reset: the snapshot is taken behind the first step that re-placed envs (their step counter is 0 again)
        for t_snap in range(1, T0 + 1):
            go(a, t_snap - 1, 1)
            if bool((a.buffer(capi.BUF_TIMER)[:, 0] == 0).any()):
                break
        assert bool((a.buffer(capi.BUF_TIMER)[:, 0] == 0).any()) and bool((a.buffer(capi.BUF_TIMER)[:, 3] >= 2).any()) and t_snap >= 2
        assert a.state_header().obs_flags & capi.OBS_BOUNDARY_POINTS
    else:
        go(a, 0, T0, bank=banks[0])
    snap = a.snapshot()
    bank_sd = banks[0].state_dict() if bank else None
    at_snapshot = _words(a)
    rec_a = go(a, t_snap, T1, bank=banks[0])
    # a fresh handle of the same configuration whose buffers hold other content
    other(b, 0, 5, seed=SEED + 1, bank=banks[1])
    assert not torch.equal(b.snapshot().blob, snap.blob)
    assert snap.header == {**b.state_header().as_dict(), "observe_calls": snap.header["observe_calls"], "cbf_groups_valid": snap.header["cbf_groups_valid"]}
    b.restore(snap)
    if bank:
        banks[1].load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in bank_sd.items()})
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(banks[1].state_dict().values(), bank_sd.values()) if isinstance(x, torch.Tensor))
    got = _words(b)
    assert [w for w in got if not torch.equal(got[w], at_snapshot[w])] == []  # the handle's buffers are the snapshot's bits: nothing was re-derived
    back = b.snapshot()
    assert torch.equal(back.blob, snap.blob) and back.header == snap.header and back.reset_counter == snap.reset_counter
    rec_b = go(b, t_snap, T1, bank=banks[1])
    assert torch.equal(_bits(rec_b), _bits(rec_a))
    if bank:
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(banks[0].state_dict().values(), banks[1].state_dict().values()) if isinstance(x, torch.Tensor))
        assert not torch.equal(_bits(banks[0].state_dict()["ring_state"]), _bits(bank_sd["ring_state"]))  # (the rings moved on)
    wa, wb = _words(a), _words(b)
    assert [w for w in wa if not torch.equal(wa[w], wb[w])] == []
    end_a, end_b = a.snapshot(), b.snapshot()
    assert torch.equal(end_a.blob, end_b.blob) and end_a.header == end_b.header
    assert not torch.equal(end_a.blob, snap.blob) and rec_a[:, :, -1].sum().item() >= 1  # the 8 steps moved the state, and envs finished: resets ran
    if drive == "cbf_qp":
        assert snap.header["cbf"] == capi.STATE_CBF_GROUPED and snap.header["cbf_groups_valid"] == 1 and (a.cbf_groups() == b.cbf_groups()).all()
    if drive == "cbf_rewards":
        assert snap.header["cbf"] == capi.STATE_CBF_ATTACHED
    # the snapshot travels: to the host and back
    there = snap.cpu()
    assert not there.blob.is_cuda and torch.equal(there.to(a.device).blob, snap.blob) and there.header == snap.header
    for x in (*[k for k in banks if k is not None], *([actor] if actor is not None else []), a, b):
        x.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_restored_handle_repeats_the_run_bit_for_bit(shape):
    _whole(**SHAPES[shape])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_restored_handle_repeats_the_run_under(variant):
    _whole(4, 6, **VARIANTS[variant])


def _mask(B):
    """about a third of the envs: env 0, env B - 1, every third in between, and env 1 beside env 0 (4 agents: one wavefront tile holds them both)"""
    import torch

    m = torch.zeros(B, dtype=torch.bool, device="cuda")
    m[0::3] = True
    m[1] = True
    m[B - 1] = True
    return m


@pytest.mark.parametrize("shape", ["4x6_intersection_4", "4x130_cpm", "16x5_cpm"])
def test_a_masked_restore_rewinds_the_chosen_envs_and_no_word_of_the_others(shape):
    import torch

    c = SHAPES[shape]
    env = _env(c["N"], c["B"], c["scen"])
    B = env.B
    go = Drive("n", _actions(env))
    env.reset_random(seed=3, counter=1000)
    go(env, 0, T0)
    S = env.snapshot()
    at_S = _words(env)
    rec_a = go(env, T0, T1)
    before, before_blob = _words(env), env.snapshot().blob.clone()
    assert not torch.equal(before_blob, S.blob)
    on = _mask(B)
    assert bool(on[0]) and bool(on[1]) and bool(on[B - 1]) and 0 < int(on.sum()) < B
    env.restore(S, envs=torch.zeros(B, dtype=torch.uint8, device="cuda"))  # an all-zero mask changes no word
    assert torch.equal(env.snapshot().blob, before_blob)
    calls = env.state_header().observe_calls
    env.restore(S, envs=on)
    after = _words(env)
    kept, theirs = _env_words(env, after, ~on), _env_words(env, before, ~on)
    assert [w for w in kept if not torch.equal(kept[w], theirs[w])] == []  # every buffer word of every unmasked env is what it was
    rewound, want = _env_words(env, after, on), _env_words(env, at_S, on)
    assert [w for w in rewound if not torch.equal(rewound[w], want[w])] == []  # and the masked envs hold the snapshot's bits
    assert env.state_header().observe_calls == calls  # the host words stay under a mask
    rec_b = go(env, T0, T1)
    assert torch.equal(_bits(rec_b[:, on]), _bits(rec_a[:, on]))  # run B: the masked envs repeat run A
    assert not torch.equal(_bits(rec_b[:, ~on]), _bits(rec_a[:, ~on]))  # (the others went on from where they were)
    env.restore(S, envs=torch.ones(B, dtype=torch.bool, device="cuda"))  # an all-ones mask equals the unmasked restore in every device word
    assert torch.equal(env.snapshot().blob, S.blob)
    env.restore(S)
    assert torch.equal(env.snapshot().blob, S.blob)
    with pytest.raises(TypeError, match="envs"):
        env.restore(S, envs=torch.ones(B + 1, dtype=torch.bool, device="cuda"))
    with pytest.raises(TypeError, match="envs"):
        env.restore(S, envs=torch.ones(B, dtype=torch.int32, device="cuda"))
    env.close()


def test_guard_bytes_around_the_blob_survive_and_out_is_reused():
    import torch
    from sigmarl_amd.env import Snapshot

    env = _env(4, 130)
    env.reset_random(seed=3, counter=1000)
    Drive("n", _actions(env))(env, 0, 3)
    ref = env.snapshot()
    n = ref.blob.numel()
    assert n == ref.header["total_bytes"] and n % 16 == 0
    big = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    out = Snapshot(ref.header, big[64: 64 + n])
    assert env.snapshot(out=out) is out and out.blob.data_ptr() == big.data_ptr() + 64
    env.sync()
    assert bool((big[:64] == 0xA5).all()) and bool((big[64 + n:] == 0xA5).all()) and torch.equal(big[64: 64 + n], ref.blob)
    with pytest.raises(ValueError, match="out="):
        env.snapshot(out=Snapshot(ref.header, big[64: 64 + n - 16]))
    env.close()


def test_refusals_come_back_on_the_return_path_and_change_nothing():
    import torch
    from sigmarl_amd import capi

    env, other = _env(4, 6), _env(4, 7)
    for e in (env, other):
        e.reset_random(seed=3, counter=1000)
    ref, foreign = env.snapshot(), other.snapshot()
    n = ref.blob.numel()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    hdr = capi.StateHeader.from_dict(ref.header)
    p = work.data_ptr()
    assert p % 16 == 0
    cases = [
        ("a wrong size", lambda: env.lib.state_save(env.h, C.c_void_p(p), n - 16), "total"),
        ("a misaligned blob", lambda: env.lib.state_save(env.h, C.c_void_p(p + 4), n), "16-byte aligned"),
        ("a null blob", lambda: env.lib.state_save(env.h, None, n), "null blob"),
        ("restore: a wrong size", lambda: env.lib.state_restore(env.h, C.byref(hdr), C.c_void_p(ref.blob.data_ptr()), n + 16, None), "total"),
        ("restore: a misaligned blob", lambda: env.lib.state_restore(env.h, C.byref(hdr), C.c_void_p(p + 8), n, None), "16-byte aligned"),
        ("restore: a header of another shape", lambda: env.lib.state_restore(env.h, C.byref(capi.StateHeader.from_dict(foreign.header)), C.c_void_p(ref.blob.data_ptr()), n, None),
         "n_envs is 7, the handle's 6"),
        ("restore: another version", lambda: env.lib.state_restore(env.h, C.byref(capi.StateHeader.from_dict({**ref.header, "version": 2})), C.c_void_p(ref.blob.data_ptr()), n, None),
         "version is 2"),
        ("restore: no magic", lambda: env.lib.state_restore(env.h, C.byref(capi.StateHeader.from_dict({**ref.header, "magic": 0})), C.c_void_p(ref.blob.data_ptr()), n, None), "magic"),
    ]
    for k, (what, call, message) in enumerate(cases):
        counter += 1
        rc = call()
        counter += 1
        assert rc == -22 and message in env.lib.last_error(env.h).decode(), (what, rc, env.lib.last_error(env.h))
        assert int(counter.item()) == 2 * (k + 1)
    assert not work.any() and torch.equal(env.snapshot().blob, ref.blob)  # nothing was launched: the scratch blob and the handle are as they were
    with pytest.raises(RuntimeError, match="n_envs is 7"):
        env.restore(foreign)
    with pytest.raises(TypeError, match="Snapshot.to"):
        env.restore(ref.cpu())
    bird = _env(4, 6, is_ego_view=False)
    with pytest.raises(RuntimeError, match="obs_dim|obs_flags"):
        bird.restore(ref)
    for e in (env, other, bird):
        e.close()
