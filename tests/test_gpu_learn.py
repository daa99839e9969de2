"""Learner-ready rollouts on the device: the root-observation record of the rollout loop (sigmaenv_set_rollout_obs_record), the networks on record rows
(sigmaenv_mlp32_forward_rows), GAE and the TD-error priorities (sigmaenv_gae), and learn.collect end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
TENT = 1 << 63  # the tentative forward's key of opponent modelling (include/sigmaenv.h)
KW = dict(n_agents=16, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=6)  # short episodes: resets inside every rollout


def _actor(D, seed=1):
    import torch
    from sigmarl_amd.actor import Actor, make_mlp

    torch.manual_seed(seed)
    mlp = make_mlp(D)
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(1.7)
                m.bias.uniform_(-0.3, 0.3)
    return mlp, Actor(mlp, low=LOW, high=HIGH)


def _critic_mlp(in_dim, seed=4):
    import torch
    from sigmarl_amd.actor import make_mlp

    torch.manual_seed(seed)
    return make_mlp(in_dim, n_out=1)


def _env(B, **kw):
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    pk = dict(KW)
    pk.update(kw)
    ib = pk.pop("env_index_base", None)
    e = SigmaEnv(Parameters(**pk), n_envs=B, device="cuda:0", env_index_base=ib)
    e.reset_random(seed=3)
    return e


def _records_show_resets(torch, slab, obs_rec, N, D):
    """The workload must make the record necessary: an env finished, and the observation a later step acted on is not the previous record row's."""
    assert slab[..., -1].sum().item() >= 1, "no env finished: the test shows nothing"
    post = slab[:-1, :, : N * D]
    root = obs_rec[1:].reshape(post.shape)
    assert (post != root).any(dim=-1).any().item(), "no re-placed env: obs_rec[t + 1] equals the slab's observation of step t everywhere"


# ---- 1. the root-observation record ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapper", [None, "opponent"])
def test_obs_record_equals_the_host_loop(wrapper):
    """obs_rec[t] of a T-step device rollout == env.obs.clone() taken before step t in the host loop of single forward + step_autoreset calls (opponent modelling:
    after the placeholder columns were filled), bit for bit, on a workload with resets; and a rollout WITHOUT the record gives the same slab / actions /
    log-probabilities as the one with it."""
    import torch
    from sigmarl_amd.shard import slab_width

    okw = dict(is_using_opponent_modeling=True) if wrapper else {}
    env, env2, env3 = _env(48, **okw), _env(48, **okw), _env(48, **okw)
    mlp, actor = _actor(env.D)
    T, B, N, D, W = 10, env.B, env.N, env.D, slab_width(env.N, env.D)
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    slab, lp, acts, rec = z(T, B, W), z(T, B, N), z(T, B, N, 2), z(T, B, N, D)
    slab2, lp2, acts2, rec2 = z(T, B, W), z(T, B, N), z(T, B, N, 2), z(T, B, N, D)
    slab3, lp3, acts3 = z(T, B, W), z(T, B, N), z(T, B, N, 2)
    torch.cuda.synchronize()
    actor.rollout(env, T, slab=slab, log_prob=lp, actions=acts, obs_rec=rec, seed=9, counter0=100, wrapper=wrapper)
    actor.rollout(env3, T, slab=slab3, log_prob=lp3, actions=acts3, seed=9, counter0=100, wrapper=wrapper)  # no record
    env.sync()
    env3.sync()
    a, at = z(B, N, 2), z(B, N, 2)
    torch.cuda.synchronize()
    for t in range(T):
        if wrapper:
            actor.forward(env2, at, seed=9 ^ TENT, counter=100 + t)
            env2.opponent_fill(at)
        actor.forward(env2, a, lp2[t], seed=9, counter=100 + t)
        env2.sync()
        rec2[t] = env2.obs.clone()
        acts2[t] = a
        torch.cuda.synchronize()
        env2.set_slab(slab2[t])
        env2.step_autoreset(a, seed=9, counter=100 + t)
        env2.sync()
    env2.set_slab(None)
    assert torch.equal(slab, slab2) and torch.equal(lp, lp2) and torch.equal(acts, acts2)
    assert torch.equal(rec, rec2)
    _records_show_resets(torch, slab, rec, N, D)
    if wrapper:
        assert (rec[..., D - 2 * env.K:] != 0).float().mean() > 0.5  # the filled placeholder columns are part of the record
    assert torch.equal(slab, slab3) and torch.equal(lp, lp3) and torch.equal(acts, acts3)  # the record changes nothing else
    # the record was for that one call: a further rollout leaves `rec` alone
    keep = rec.clone()
    actor.rollout(env, 2, seed=9, counter0=200, wrapper=wrapper)
    env.sync()
    assert torch.equal(rec, keep)
    with pytest.raises(RuntimeError):
        env.set_rollout_obs_record(rec, B * N * D - 1)  # a stride below the handle's own block
    for e in (env, env2, env3):
        e.close()
    actor.close()


def test_two_env_shards_record_into_one_observation_buffer():
    """Shard k (envs [k Bs, (k + 1) Bs), env_index_base) records into obs_rec + k Bs N D with the stride B N D: the [T, B, N, D] buffer equals the unsharded handle's."""
    import torch
    from sigmarl_amd.shard import slab_width

    B, Bs, T = 64, 32, 10
    whole = _env(B)
    mlp, actor = _actor(whole.D)
    N, D, W = whole.N, whole.D, slab_width(whole.N, whole.D)
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    slab, rec, slab2, rec2 = z(T, B, W), z(T, B, N, D), z(T, B, W), z(T, B, N, D)
    torch.cuda.synchronize()
    actor.rollout(whole, T, slab=slab, obs_rec=rec, seed=9, counter0=100)
    whole.sync()
    shards = [_env(Bs, env_index_base=k * Bs) for k in range(2)]
    torch.cuda.synchronize()
    for k, e in enumerate(shards):
        e.set_rollout_slab_stride(B * W)
        e.set_rollout_obs_record(rec2.data_ptr() + 4 * k * Bs * N * D, B * N * D)
        actor.rollout(e, T, slab_ptr=slab2.data_ptr() + 4 * k * Bs * W, seed=9, counter0=100)
    for e in shards:
        e.sync()
        e.set_rollout_obs_record(None)
    assert torch.equal(slab, slab2)
    assert torch.equal(rec, rec2)
    _records_show_resets(torch, slab, rec, N, D)
    for e in shards + [whole]:
        e.close()
    actor.close()


# ---- 2. the networks on record rows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,mode", [(16, 32, "split"), (32, 32, "exact"), (16, 35, "split"), (16, 35, "exact"), (17, 35, "exact")])
def test_forward_rows_equals_forward_on_the_rows_copied_dense(N, D, mode):
    """sigmaenv_mlp32_forward_rows on the observation part of record rows -- W = N (D + 1) + 1 odd, the buffer starting at a 4-byte-only offset of its allocation, the
    two-level strides of a two-shard [T, B_total, W] buffer, 74 rows per block (not a multiple of 64) -- is bit for bit Mlp32.forward on the rows copied dense, in
    both arithmetic modes (N = 32: the exact kernel's chunked staging; D = 35: a wider row, N D = 595 not a multiple of 4: the element-wise staging); and the dense
    result is within tests/network_check.py's bound of torch.nn in fp64, as the critic tests hold it."""
    import network_check as nc
    import torch
    from sigmarl_amd.actor import Critic

    env = _env(8)  # (any handle: it lends its stream)
    mlp = _critic_mlp(N * D)
    critic = Critic(mlp, mode=mode)
    assert critic.set_mode(mode) == mode
    T, Bt, Bs, W = 3, 150, 74, N * (D + 1) + 1
    assert W % 2 == 1
    g = torch.Generator().manual_seed(7)
    for off in (1, 3, 0):  # floats between the (256-byte aligned) allocation and the record
        store = torch.full((off + T * Bt * W + 8,), float("nan"), device="cuda")
        slab = store[off: off + T * Bt * W].view(T, Bt, W)
        slab.copy_((torch.rand((T, Bt, W), generator=g) * 2 - 1).cuda())  # observations are normalised: |x| < 1 (rewards and flags in between)
        for k in range(2):  # shard k: rows [k Bs, (k + 1) Bs) of every step
            torch.cuda.synchronize()
            got = critic.forward_rows(env, store, off + k * Bs * W, Bs, W, T, Bt * W)
            env.sync()
            dense = slab[:, k * Bs: (k + 1) * Bs, : N * D].contiguous()
            want = critic.forward(env, dense.view(T * Bs, N * D))
            env.sync()
            assert torch.equal(got.view(-1), want.view(-1)), (off, k)
            if off == 1 and k == 1:
                nc.check(want, mlp, dense.view(T * Bs, N * D), what=f"critic {N}x{D} {mode} on record rows")
    # the aligned route of the same entry point: a dense 16-byte-aligned buffer with strides that are multiples of 4 floats
    if (N * D) % 4 == 0:
        x = (torch.rand((2, 70, N * D + 4), generator=g) * 2 - 1).cuda()
        torch.cuda.synchronize()
        got = critic.forward_rows(env, x, 0, 70, N * D + 4, 2, 70 * (N * D + 4))
        want = critic.forward(env, x[:, :, : N * D].contiguous().view(140, N * D))
        env.sync()
        assert torch.equal(got.view(-1), want.view(-1))
    with pytest.raises(ValueError):
        critic.forward_rows(env, store, 0, Bs, N * D - 1, T, Bt * W)  # rows would overlap the network's input
    with pytest.raises(ValueError):
        critic.forward_rows(env, store, off + Bs * W, Bt, W, T, Bt * W)  # the last row ends beyond the tensor
    env.close()
    critic.close()


def test_rollout_values_reads_a_real_record():
    """Critic.rollout_values on a real rollout's records (two shards' worth of strides included) == the critic on torch slices of the same records."""
    import torch
    from sigmarl_amd.actor import Critic
    from sigmarl_amd.shard import slab_width

    env = _env(48)
    mlp, actor = _actor(env.D)
    critic = Critic(_critic_mlp(env.N * env.D))
    T, B, N, D, W = 7, env.B, env.N, env.D, slab_width(env.N, env.D)
    Bt = B + 10  # the handle's envs sit at [6, 6 + B) of wider buffers
    slab, rec = torch.zeros((T, Bt, W), device="cuda"), torch.zeros((T, Bt, N, D), device="cuda")
    torch.cuda.synchronize()
    env.set_rollout_slab_stride(Bt * W)
    env.set_rollout_obs_record(rec.data_ptr() + 4 * 6 * N * D, Bt * N * D)
    actor.rollout(env, T, slab_ptr=slab.data_ptr() + 4 * 6 * W, seed=5, counter0=0)
    env.set_rollout_obs_record(None)
    env.set_rollout_slab_stride(0)
    sv, nv = critic.rollout_values(env, slab, rec, T, env_first=6)
    env.sync()
    want_s = critic.forward(env, rec[:, 6: 6 + B].reshape(T * B, N * D).contiguous())
    want_n = critic.forward(env, slab[:, 6: 6 + B, : N * D].reshape(T * B, N * D).contiguous())
    env.sync()
    assert torch.equal(sv.reshape(-1), want_s.reshape(-1)) and torch.equal(nv.reshape(-1), want_n.reshape(-1))
    assert sv.abs().sum().item() > 0 and not torch.equal(sv, nv)
    env.close()
    actor.close()
    critic.close()


# ---- 3. GAE and the TD-error priorities ---------------------------------------------------------------------------------------------
def gae_numpy(r, done, v, vn, gamma, lmbda):
    """The arithmetic contract of sigmaenv_gae (include/sigmaenv.h) in numpy fp32, operation by operation (numpy does not contract).  r [T,B,N]; done, v, vn [T,B]."""
    f = np.float32
    T, B, N = r.shape
    g, c = f(gamma), f(f(gamma) * f(lmbda))
    adv, vt = np.zeros((T, B, N), f), np.zeros((T, B, N), f)
    a_next = np.zeros((B, N), f)
    for t in range(T - 1, -1, -1):
        nd = (f(1) - done[t])[:, None]
        d = (r[t] + (g * vn[t])[:, None] * nd) - v[t][:, None]
        a = d + ((c * nd) * a_next)
        adv[t], vt[t] = a, a + v[t][:, None]
        a_next = a
    return adv, vt


def td_numpy(r, done, v, vn, td_gamma):
    """compute_td_error (helper_training.py:1029-1068) in numpy fp32 in the contract's order: the agents summed sequentially i = 0 .. N - 1, divided by N."""
    f = np.float32
    T, B, N = r.shape
    nd = f(1) - done
    boot = (f(td_gamma) * vn) * nd
    s = np.zeros((T, B), f)
    for i in range(N):
        s = s + np.abs((r[:, :, i] + boot) - v)
    x = s / f(N)
    mn, mx = x.min(), x.max()
    rng = np.maximum(mx - mn, f(1e-3))
    return np.clip(((x - mn) / rng) * f(10), f(1e-3), f(10)).astype(f), x


def gae_float64(r, done, v, vn, gamma, lmbda):
    """The same recursion in fp64 on the fp32 inputs (gamma, c as the fp32 numbers the device uses), and the magnitude sums of the running-error bound."""
    f = np.float32
    g, c = np.float64(f(gamma)), np.float64(f(f(gamma) * f(lmbda)))
    r, done, v, vn = (x.astype(np.float64) for x in (r, done, v, vn))
    T, B, N = r.shape
    adv, mag = np.zeros((T, B, N)), np.zeros((T, B, N))
    a_next, m_next = np.zeros((B, N)), np.zeros((B, N))
    for t in range(T - 1, -1, -1):
        nd = (1.0 - done[t])[:, None]
        adv[t] = (r[t] + (g * vn[t])[:, None] * nd) - v[t][:, None] + (c * nd) * a_next
        # sum of the magnitudes of every term that has entered A_t:  M_t = |r| + |g vn nd| + |v| + c nd M_{t+1}
        mag[t] = np.abs(r[t]) + np.abs((g * vn[t])[:, None] * nd) + np.abs(v[t])[:, None] + (c * nd) * m_next
        a_next, m_next = adv[t], mag[t]
    return adv, mag


def _device_gae(torch, env, r, done, v, vn, gamma, lmbda, td_gamma=0.9):
    """Packs (r, done) into record rows (observation part: NaN -- never read) and runs learn.gae."""
    from sigmarl_amd import learn

    T, B, N = r.shape
    D = env.D
    W = N * (D + 1) + 1
    slab = np.full((T, B, W), np.nan, np.float32)
    slab[:, :, N * D: N * D + N] = r
    slab[:, :, N * D + N] = done
    ts = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    slab_d, v_d, vn_d = ts(slab), ts(v), ts(vn)
    torch.cuda.synchronize()
    adv, vt, td = learn.gae(env, slab_d, v_d, vn_d, gamma, lmbda, td_error=True, td_gamma=td_gamma)
    env.sync()
    return adv.cpu().numpy(), vt.cpu().numpy(), td.cpu().numpy(), (slab_d, v_d, vn_d)


@pytest.mark.parametrize("T", [1, 7, 32])
@pytest.mark.parametrize("N,scen,pkw", [(4, "on_ramp_1", dict(is_testing_mode=True, is_observe_distance_to_boundaries=False)), (16, "cpm_entire", {}), (17, "cpm_entire", {})])
def test_gae_on_random_records(T, N, scen, pkw):
    """Device GAE / TD priorities == the numpy fp32 restatement of the contract, bit for bit, on random rewards / values / done flags (done rate 0.2); within the
    running-error bound of an fp64 evaluation; priorities in [1e-3, 10]; two runs give the same bits."""
    import torch
    from sigmarl_amd import learn

    env = _env(37, n_agents=N, scenario_type=scen, **pkw)
    B = env.B
    rng = np.random.default_rng(100 * T + N)
    r = rng.normal(0, 1.5, (T, B, N)).astype(np.float32)
    done = (rng.random((T, B)) < 0.2).astype(np.float32)
    v, vn = rng.normal(0, 3, (T, B)).astype(np.float32), rng.normal(0, 3, (T, B)).astype(np.float32)
    gamma, lmbda = 0.99, 0.9
    adv, vt, td, (slab_d, v_d, vn_d) = _device_gae(torch, env, r, done, v, vn, gamma, lmbda)
    want_a, want_vt = gae_numpy(r, done, v, vn, gamma, lmbda)
    want_td, _ = td_numpy(r, done, v, vn, 0.9)
    assert np.array_equal(adv.view(np.uint32), want_a.view(np.uint32))
    assert np.array_equal(vt.view(np.uint32), want_vt.view(np.uint32))
    assert np.array_equal(td.view(np.uint32), want_td.view(np.uint32))
    assert td.min() >= np.float32(1e-3) and td.max() <= np.float32(10) and td.max() == np.float32(10)
    # Running-error bound against fp64 (u = 2^-24, the unit roundoff of fp32; ~ marks computed values).  One step computes
    #     p~ = fl(fl(g vn) nd),  s1~ = fl(r + p~),  s2~ = fl(s1~ - v),  q~ = fl(fl(c nd) A~_{t+1}),  A~_t = fl(s2~ + q~).
    # nd is 0 or 1, so the products by nd are exact: p~ and q~ carry ONE rounding each (of g vn and of c A~_{t+1}), the three additions one each.  Hence
    #     e_t = |A~_t - A_t| <= u (|p| + |s1| + |s2| + |q| + |A_t|) (1 + O(u)) + c nd e_{t+1}.
    # With M_t = |r| + |p| + |v| + c nd M_{t+1} (the sum of the magnitudes of every term that enters A_t; gae_float64 evaluates it) each of the five magnitudes is
    # <= M_t (|q| = c nd |A_{t+1}| <= c nd M_{t+1}), and c nd <= 1:
    #     e_t <= 5 u M_t + e_{t+1} <= 5 u sum_{s >= t} M_s <= 5 u (T - t) max_{s >= t} M_s.
    # That last expression, times 1.01 for the O(u^2) terms, is the bound, per (step, env, agent).  value_target = fl(A~ + v) adds one rounding of a sum whose
    # magnitude is at most |A| + |v| <= 2 M_t.
    ref, mag = gae_float64(r, done, v, vn, gamma, lmbda)
    u = 2.0 ** -24
    steps_left = (T - np.arange(T))[:, None, None]
    chain_max = np.maximum.accumulate(mag[::-1], axis=0)[::-1]  # max over s >= t
    bound = 1.01 * 5 * u * steps_left * chain_max
    err = np.abs(adv.astype(np.float64) - ref)
    assert (err <= bound).all(), f"advantage: max error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}"
    err_vt = np.abs(vt.astype(np.float64) - (ref + v.astype(np.float64)[:, :, None]))
    assert (err_vt <= bound + 1.01 * 2 * u * mag).all()
    # the same inputs again: the same bits (the min / max reduction does not depend on scheduling)
    adv2, vt2, td2 = learn.gae(env, slab_d, v_d, vn_d, gamma, lmbda, td_error=True)
    env.sync()
    assert np.array_equal(adv2.cpu().numpy().view(np.uint32), adv.view(np.uint32)) and np.array_equal(td2.cpu().numpy().view(np.uint32), td.view(np.uint32))
    assert np.array_equal(vt2.cpu().numpy().view(np.uint32), vt.view(np.uint32))
    env.close()


def test_td_priorities_of_a_constant_batch():
    """max - min < 1e-3: the range is clamped to 1e-3 (compute_td_error's `max(td_error_range, 1e-3)`), so nothing divides by zero and every priority is the floor
    1e-3 or the small multiple the formula gives; still bit for bit the numpy restatement."""
    import torch

    env = _env(37)
    T, B, N = 5, env.B, env.N
    r = np.full((T, B, N), 0.25, np.float32)
    done = np.zeros((T, B), np.float32)
    v, vn = np.full((T, B), 1.5, np.float32), np.full((T, B), 1.25, np.float32)
    _, _, td, _ = _device_gae(torch, env, r, done, v, vn, 0.99, 0.9)
    want, raw = td_numpy(r, done, v, vn, 0.9)
    assert raw.max() - raw.min() < 1e-3
    assert np.array_equal(td.view(np.uint32), want.view(np.uint32))
    assert (td == np.float32(1e-3)).all()
    # nearly constant: a spread below the clamp
    v2 = v.copy()
    v2[2, 5] += np.float32(4e-4)
    _, _, td, _ = _device_gae(torch, env, r, done, v2, vn, 0.99, 0.9)
    want, raw = td_numpy(r, done, v2, vn, 0.9)
    assert 0 < raw.max() - raw.min() < 1e-3
    assert np.array_equal(td.view(np.uint32), want.view(np.uint32))
    assert td.min() >= np.float32(1e-3) and td.max() <= np.float32(10)
    env.close()


def _collect(torch, T=32, B=256):
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Critic

    env = _env(B)
    mlp, actor = _actor(env.D)
    critic = Critic(_critic_mlp(env.N * env.D))
    torch.cuda.synchronize()
    out = learn.collect(env, actor, critic, T, seed=5, counter0=0)
    env.sync()
    return env, actor, critic, out


def test_gae_on_a_real_rollout():
    """learn.gae on a real rollout's record and the critic's values: bit for bit the numpy restatement (rewards and done flags read in place from the rows)."""
    import torch

    env, actor, critic, out = _collect(torch, T=32, B=64)
    N, D = env.N, env.D
    slab = out["slab"].cpu().numpy()
    r, done = slab[:, :, N * D: N * D + N], slab[:, :, N * D + N]
    assert np.array_equal(r, out[("next", "reward")].cpu().numpy()) and np.array_equal(done, out[("next", "done")].cpu().numpy())
    assert 0 < done.sum() < done.size
    v, vn = out["state_value"].cpu().numpy(), out[("next", "state_value")].cpu().numpy()
    p = env.parameters
    want_a, want_vt = gae_numpy(r, done, v, vn, p.gamma, p.lmbda)
    want_td, _ = td_numpy(r, done, v, vn, 0.9)
    assert np.array_equal(out["advantage"].cpu().numpy().view(np.uint32), want_a.view(np.uint32))
    assert np.array_equal(out["value_target"].cpu().numpy().view(np.uint32), want_vt.view(np.uint32))
    assert np.array_equal(out["td_error"].cpu().numpy().view(np.uint32), want_td.view(np.uint32))
    env.close()
    actor.close()
    critic.close()


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------
def test_collect_end_to_end():
    """learn.collect at 16 agents x 256 envs, T = 32: the batch is consistent with itself -- value_target - state_value reproduces advantage to the rounding of that
    one subtraction, the last step's advantage is its delta, and state_value[t + 1] == next_state_value[t] bit for bit exactly where nothing was re-placed at
    step t (same row, same network, same bits) while an env that finished gets a different value."""
    import torch

    T = 32
    env, actor, critic, out = _collect(torch, T=T, B=256)
    B, N, D = env.B, env.N, env.D
    for k, shape in (("observation", (T, B, N, D)), ("action", (T, B, N, 2)), ("sample_log_prob", (T, B, N)), (("next", "observation"), (T, B, N, D)),
                     (("next", "reward"), (T, B, N)), (("next", "done"), (T, B)), ("state_value", (T, B)), (("next", "state_value"), (T, B)),
                     ("advantage", (T, B, N)), ("value_target", (T, B, N)), ("td_error", (T, B))):
        assert tuple(out[k].shape) == shape and out[k].is_cuda and torch.isfinite(out[k]).all(), k
    for k in (("next", "observation"), ("next", "reward"), ("next", "done")):  # zero-copy views of the record
        assert out[k].untyped_storage().data_ptr() == out["slab"].untyped_storage().data_ptr(), k
    adv, vt = out["advantage"].double(), out["value_target"].double()
    sv, nv = out["state_value"], out[("next", "state_value")]
    # value_target = fl(A + v): (value_target - v) differs from A by at most the rounding of the addition, u (|A + v|) (1 + u), u = 2^-24 -- the subtraction
    # here is done in fp64 (exact for these operands' magnitudes to far below that)
    u = 2.0 ** -24
    assert ((vt - sv.double()[:, :, None] - adv).abs() <= 1.01 * u * vt.abs()).all()
    # the last step: A_next = 0, so A = d + (c nd) 0 = d (adding +-0 is exact): the delta in the contract's operation order
    p = env.parameters
    g = torch.tensor(p.gamma, dtype=torch.float32, device="cuda")
    nd = 1.0 - out[("next", "done")][-1]
    delta = (out[("next", "reward")][-1] + ((g * nv[-1]) * nd)[:, None]) - sv[-1][:, None]
    assert torch.equal(out["advantage"][-1], delta)
    # where nothing was re-placed the next root observation IS the record row: same bits in, same bits out
    same_row = (out["observation"][1:] == out[("next", "observation")][:-1]).all(dim=-1).all(dim=-1)  # [T - 1, B]
    done = out[("next", "done")][:-1] > 0.5
    assert same_row.any() and done.any()
    assert not (same_row & done).any()  # a finished env was re-placed
    assert torch.equal(sv[1:][same_row], nv[:-1][same_row])
    assert (sv[1:][done] != nv[:-1][done]).any()
    _records_show_resets(torch, out["slab"], out["observation"], N, D)
    env.close()
    actor.close()
    critic.close()
