"""The policy heads on the device against fp64, every row: the draw a row made is recomputed on the host from its key (seed, counter, env_index_base + env, agent)
with the restated generator (tests/policy_head_check.py), and the action and the log-probability follow from the head's own inputs (the device's loc / scale) in
closed form.  All four epilogues -- the bf16 kernel, the split fp32 kernel (also through its row map), the exact fp32 path's head kernel, the 1-D priority
head -- and the Fisher-Yates kernel; shapes from 1 x 1 to 4096 x 16, shards (env_index_base), seeds with the high word set, counters across 2^32, symmetric
and asymmetric bounds, deterministic actions, optional outputs; three regimes of the last layer (x 1 moderate; x 8 tanhf = 1, the clamp, the -2 x > 20 shortcut,
the scale floor; x 30 raw + bias > 20, most rows saturated).  No row is left out of any comparison.

Tolerances (policy_head_check.compare): |lp_dev - lp_64| <= 4 c 2^-23 S(row), |a_dev - a_64| <= 4 c_a 2^-23 A(row), c and c_a measured on the float32 twin of the
head on the CPU over the very rows of the case (a case of fewer than 1000 rows also takes those of its calibration case: 257 x 16 rows of the same network, key and
bounds); saturated rows' actions exact.  Twin, 257 x 16 rows, last layer x 1 / x 8 / x 30: actor c = 0.34 / 0.46 / 0.55 (2.4e-6 / 9.3e-6 / 2.5e-5 absolute at the worst
row), c_a = 0.86 / 0.94 / 0.97 (1.3e-6 to 3.1e-6 absolute); priority c = 0.36 / 0.62 / 0.96 (2.1e-6 / 1.1e-5 / 5.0e-5), c_a = 0.47 to 0.49; |z_32 - z_64| <= 1.3e-6.  On
the x 1 case the bound of every row is at least 100 x below the statistical tests' 5e-3 (actor: 4.7e-6 at the median row, 3.1e-5 at the largest S) and 2e-3 (priority:
3.0e-6, 1.7e-5).  
The device's observed maxima (MI355X; x 1 / x 8 / x 30, in brackets the largest ratio device / twin of the path, allowed to reach 4): bf16 c = 0.31 / 0.54 / 0.65
(1.29), c_a = 0.59 / 0.70 / 0.72 (0.92); split 0.22 / 0.55 / 0.56 (1.32), 0.69 / 0.84 / 0.85 (0.90); split over the 216 cases of the cross 0.74 (1.94), 0.85 (1.05);
split 4096 x 16 0.32 (1.12), 0.79 (0.82); row map 0.40 (1.00), 0.83 (0.86); exact 0.23 / 0.43 / 0.44 (1.09), 0.73 / 0.83 / 0.83 (0.88); priority on the split network
0.35 / 0.52 / 0.61 (0.93), 0.41 / 0.38 / 0.57 (1.00); on the exact network 0.40 / 0.65 / 0.73 (1.14), 0.51 / 0.42 / 0.39 (0.94).  Worst absolute error of a
log-probability 5.3e-5 (priority, x 30), of an action 1.0e-5.  Every test prints its figures; POLICY_HEAD_REPORT=path collects them.  DESIGN.md section 2 has the table.
"""
import numpy as np
import pytest

import network_check as nc
import policy_head_check as ph

pytestmark = pytest.mark.gpu

HI_SEED = (0xABCD1234 << 32) | 77
SEEDS = [0, 12345, HI_SEED]
COUNTERS = [0, 2 ** 32 - 1, 2 ** 32 + 5]
BOUNDS = [([-1.0, -0.6], [1.0, 0.6]), ([-0.2, 0.1], [1.5, 0.3])]  # (low, high): the reference's, and an asymmetric pair
SHAPES = [(1, 1), (51, 5), (16, 16), (257, 1), (257, 16), (129, 32)]
BASES = [0, 100000]
PAD = 1024  # NaN sentinels behind every output


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def envs():
    """env handles by (B, N, env_index_base), created on first use (a handle created as a shard keys its draws by env_index_base + env)"""
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters
    made = {}

    def get(B, N, base=0):
        if (B, N, base) not in made:
            made[(B, N, base)] = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=B,
                                          device="cuda:0", env_index_base=base)
            assert made[(B, N, base)].cfg.env_index_base == base
        return made[(B, N, base)]

    yield get
    for e in made.values():
        e.close()


def _actor(mlp, bounds, path):
    from sigmarl_amd.actor import Actor
    if path == "bf16":
        return Actor(mlp, low=bounds[0], high=bounds[1], precision="bf16")
    a = Actor(mlp, low=bounds[0], high=bounds[1], mode=path)
    assert a._mlp32.set_mode(path) == path
    return a


def _sentinel(n):
    import torch
    return torch.full((n + PAD,), float("nan"), device="cuda")


def _forward(actor, env, obs, seed, counter, deterministic=False, want_lp=True, want_ls=True):
    """Actor.forward into NaN-filled buffers with PAD sentinels behind each; returns (actions [R, 2], log_prob [R] | None, loc_scale [R, 4] | None) as numpy, after
    asserting that nothing but the asked-for outputs was written"""
    import torch
    R = env.B * env.N
    ba, bl, bs = _sentinel(2 * R), _sentinel(R), _sentinel(4 * R)
    act, lp, ls = ba[:2 * R].view(env.B, env.N, 2), bl[:R].view(env.B, env.N), bs[:4 * R].view(env.B, env.N, 4)
    actor.forward(env, act, lp if want_lp else None, ls if want_ls else None, obs=obs, seed=seed, counter=counter, deterministic=deterministic)
    env.sync()
    assert torch.isnan(ba[2 * R:]).all() and torch.isnan(bl[R:]).all() and torch.isnan(bs[4 * R:]).all(), "a head wrote beyond its outputs"
    assert not torch.isnan(act).any() and (want_lp or torch.isnan(bl).all()) and (want_ls or torch.isnan(bs).all())
    return act.reshape(R, 2).cpu().numpy(), lp.reshape(R).cpu().numpy() if want_lp else None, ls.reshape(R, 4).cpu().numpy() if want_ls else None


RECORDS = []  # the figures of every comparison of the module (POLICY_HEAD_REPORT=path: appended there as JSON lines when the module is done)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    import json
    import os
    path = os.environ.get("POLICY_HEAD_REPORT")
    if path and RECORDS:
        with open(path, "a") as f:
            for r in RECORDS:
                f.write(json.dumps(r) + "\n")


def _note(r):
    RECORDS.append(r)
    print({k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in r.items()})
    return r


def _check_actor(actor, env, obs, seed, counter, bounds, what, deterministic=False, net=None):
    a, lp, ls = _forward(actor, env, obs, seed, counter, deterministic)
    r, ref, z = ph.check_rows(a, lp, ls[:, :2], ls[:, 2:], seed, counter, env.B, env.N, env.cfg.env_index_base, bounds[0], bounds[1], deterministic=deterministic, what=what,
                              net=net)
    _note(r)
    assert r["ok"], r
    assert ls[:, 2:].min() >= np.float32(0.01)
    return r, ref, z, ls


def _obs(rows, seed=5):
    import torch
    return torch.from_numpy(ph.regime_input(rows, seed)).cuda()


# ---- the split fp32 kernel's epilogue: shapes x shards x seeds x counters x bounds -----------------------------------------------------------
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_head_every_row_full_cross(envs, shape, base):
    """Last layer x 8 (saturated rows, shortcut rows and rows at the scale floor among the larger shapes), every seed x counter x pair of bounds."""
    import torch
    B, N = shape
    env, mlp, obs = envs(B, N, base), ph.regime_net(8), _obs(B * N, seed=5 + B)
    worst = dict(c_dev=0.0, c_a_dev=0.0)
    for bounds in BOUNDS:
        actor = _actor(mlp, bounds, "split")
        for seed in SEEDS:
            for counter in COUNTERS:
                r = _check_actor(actor, env, obs, seed, counter, bounds, f"split {B}x{N} base {base}", net=mlp)[0]
                worst = {k: max(v, r[k]) for k, v in worst.items()}
        # the counter enters with its low 32 bits: 2^32 + 5 draws what 5 draws (include/sigmaenv.h)
        a5, a5w = torch.zeros((B, N, 2), device="cuda"), torch.zeros((B, N, 2), device="cuda")
        actor.forward(env, a5, obs=obs, seed=12345, counter=5)
        actor.forward(env, a5w, obs=obs, seed=12345, counter=2 ** 32 + 5)
        env.sync()
        assert torch.equal(a5, a5w)
        actor.close()
    print("worst over the cross:", worst)


# ---- every path x every regime ------------------------------------------------------------------------------------------------------------------
# each path with a key and bounds of its own, so that every seed, counter, shard and pair of bounds also runs outside the split path
PATH_CASES = {"bf16": (100000, HI_SEED, 2 ** 32 - 1, BOUNDS[1]), "split": (0, 0, 0, BOUNDS[0]), "exact": (100000, 12345, 2 ** 32 + 5, BOUNDS[0])}
REGIME_NEEDS = {1: dict(inside=16), 8: dict(tanh_is_one=16, shortcut_jacobian=16, scale_floor=16, inside=16),
                30: dict(tanh_is_one=16, shortcut_jacobian=16, shortcut_scale=16, scale_floor=16, inside=16)}


@pytest.mark.parametrize("last", ph.LAST_LAYER_SCALES, ids=lambda s: f"last-x{s}")
@pytest.mark.parametrize("path", list(PATH_CASES))
def test_actor_head_in_every_regime(envs, path, last):
    """257 x 16 rows.  Every row's action and log-probability against fp64; the regime the case is meant for holds at least 16 values; on the fp32 paths the scale
    against scale_of(raw) of the fp64 network within the network criterion's bound on raw (|d scale / d raw| <= 1) plus one float32 rounding.  The bf16 path's
    scale is only held to >= 0.01 HERE (on these dense weights its raw output carries the bf16 network's error, which has no derived bound); it is held to
    scale_of(raw) with a raw bound of 0 in tests/test_gpu_bf16_actor_exact.py, on a network and on rows where the bf16 kernel's raw output is exact."""
    base, seed, counter, bounds = PATH_CASES[path]
    env, mlp, x = envs(257, 16, base), ph.regime_net(last), ph.regime_input(257 * 16)
    actor = _actor(mlp, bounds, path)
    r, ref, z, ls = _check_actor(actor, env, _obs(257 * 16), seed, counter, bounds, f"{path} last x{last}")
    n = ph.regime_counts(ref["x"], ls[:, 2:], z)
    print(n)
    for k, least in REGIME_NEEDS[last].items():
        assert n[k] >= least, (k, n)
    if path != "bf16":
        ref64, t32, s = nc.references(mlp, x)
        sc = ph.compare_scale(ls[:, 2:], ref64[:, 2:], nc.A * np.abs(t32 - ref64)[:, 2:].max() + nc.B * nc.ulp32(s))
        print(sc)
        assert sc["ok"], sc
    actor.close()


def test_split_head_4096_x_16_with_tail_draws(envs):
    """131072 draws: about 8 beyond |z| = 4 (this key: 7), where the head's x leaves the range a sampled test otherwise sees."""
    env, bounds = envs(4096, 16, 0), BOUNDS[0]
    actor = _actor(ph.regime_net(1), bounds, "split")
    r, ref, z, ls = _check_actor(actor, env, _obs(4096 * 16), 12345, 0, bounds, "split 4096x16 last x1")
    assert ph.regime_counts(ref["x"], ls[:, 2:], z)["tail_draw"] >= 1
    actor.close()


@pytest.mark.parametrize("path", list(PATH_CASES))
def test_deterministic_action_is_the_squashed_loc(envs, path):
    """deterministic: z = 0 whatever the key -- action = squash(loc), the log-probability that of the mode; last layer x 8, 51 x 5 rows of a shard."""
    bounds = BOUNDS[1]
    env, mlp = envs(51, 5, 100000), ph.regime_net(8)
    actor = _actor(mlp, bounds, path)
    obs = _obs(51 * 5, seed=9)
    r, ref, z, ls = _check_actor(actor, env, obs, HI_SEED, 2 ** 32 - 1, bounds, f"{path} deterministic", deterministic=True, net=mlp)
    a2 = _forward(actor, env, obs, 0, 77, deterministic=True)[0]
    a1 = _forward(actor, env, obs, HI_SEED, 2 ** 32 - 1, deterministic=True)[0]
    assert np.array_equal(a1, a2)
    assert np.abs(z).max() == 0.0
    actor.close()


@pytest.mark.parametrize("path", list(PATH_CASES))
def test_optional_outputs_leave_their_neighbours_untouched(envs, path):
    """log_prob = None and / or loc_scale = None: the same actions bit for bit, and NaN-filled buffers that were not handed over stay NaN (as do the sentinels
    behind every output: _forward); 257 x 1 rows: a ragged last tile on every path."""
    bounds = BOUNDS[0]
    env, obs = envs(257, 1, 0), _obs(257, seed=3)
    actor = _actor(ph.regime_net(8), bounds, path)
    full = _forward(actor, env, obs, 12345, 7)
    for want_lp, want_ls in ((False, True), (True, False), (False, False)):
        got = _forward(actor, env, obs, 12345, 7, want_lp=want_lp, want_ls=want_ls)
        assert np.array_equal(got[0], full[0])
        assert not want_lp or np.array_equal(got[1], full[1])
        assert not want_ls or np.array_equal(got[2], full[2])
    actor.close()


# ---- the priority head and the shuffle ----------------------------------------------------------------------------------------------------------
PRIORITY_NEEDS = {1: dict(inside=16), 8: dict(tanh_is_one=16, shortcut_jacobian=16, inside=16),  # (this network reaches the scale floor at x 30 only)
                  30: dict(tanh_is_one=16, shortcut_jacobian=16, shortcut_scale=16, scale_floor=16, inside=16)}


@pytest.mark.parametrize("last", ph.LAST_LAYER_SCALES, ids=lambda s: f"last-x{s}")
@pytest.mark.parametrize("mode", ["split", "exact"])
def test_priority_head_every_row(envs, mode, last):
    """PriorityNet.scores: the 1-D head draws the cosine branch of (7100, 7101).  Its inputs are the bits PriorityNet.forward gives (loc, raw): score and
    log-probability of every row against fp64 (the twin forms the scale in float32 as the kernel does), saturated scores exactly the clamp."""
    import torch
    from sigmarl_amd.actor import PriorityNet
    base, seed, counter = (100000, HI_SEED, 2 ** 32 + 5) if mode == "split" else (0, 12345, 2 ** 32 - 1)
    B, N = (257, 16) if last != 1 else (129, 32)
    env, mlp, obs = envs(B, N, base), ph.regime_net(last, "priority"), _obs(B * N)
    pn = PriorityNet(mlp, mode=mode)
    assert pn.set_mode(mode) == mode
    out = pn.forward(env, obs)
    sc, lp, rk = pn.scores(env, obs=obs, seed=seed, counter=counter)
    env.sync()
    o = out.cpu().numpy()
    r, ref, z = ph.check_rows(sc.reshape(-1, 1).cpu().numpy(), lp.reshape(-1).cpu().numpy(), o[:, :1], None, seed, counter, B, N, base, draws=ph.PRIORITY_DRAWS,
                              raw=o[:, 1:], what=f"priority {mode} last x{last}")
    _note(r)
    assert r["ok"], r
    n = ph.regime_counts(ref["x"], ph.scale_of(o[:, 1:]), z)
    print(n)
    for k, least in PRIORITY_NEEDS[last].items():
        assert n[k] >= least, (k, n)
    assert torch.equal(rk.long(), torch.sort(sc, dim=1, descending=True, stable=True).indices)
    # deterministic: the mode
    sc, lp, rk = pn.scores(env, obs=obs, seed=seed, counter=counter, deterministic=True)
    env.sync()
    r = ph.check_rows(sc.reshape(-1, 1).cpu().numpy(), lp.reshape(-1).cpu().numpy(), o[:, :1], None, seed, counter, B, N, base, draws=ph.PRIORITY_DRAWS, raw=o[:, 1:],
                      deterministic=True, what=f"priority {mode} last x{last} deterministic")[0]
    assert r["ok"], r
    pn.close()


@pytest.mark.parametrize("B,N,base", [(1, 1, 0), (51, 5, 100000), (16, 16, 0), (257, 1, 100000), (257, 16, 100000), (129, 32, 0), (4096, 16, 0)])
def test_random_ranks_equal_the_host_shuffle(envs, B, N, base):
    """sigmaenv_priority_random: every env's permutation == the inside-out Fisher-Yates shuffle restated on the host, exactly, at every seed and counter."""
    from sigmarl_amd.actor import random_ranks
    env = envs(B, N, base)
    for seed in SEEDS:
        for counter in COUNTERS:
            r = random_ranks(env, seed=seed, counter=counter)
            env.sync()
            assert np.array_equal(r.cpu().numpy(), ph.random_ranks(seed, counter, base + np.arange(B), N)), (seed, counter)


# ---- the row map of the prioritized wrapper -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["split", "exact"])
def test_row_map_epilogue_keys_the_draw_by_the_agent(mode):
    """Prioritized action propagation runs turn k on B compact rows and maps network row b back to agent row b N + ranks[b, k]: the recorded actions and
    log-probabilities of step 0 against fp64 with every row's draw keyed by ITS (env_index_base + env, agent).  loc / scale of an acting row: the full-batch
    forward on the observation it saw (its base observation + the neighbour actions of the tentative record), which the compact turn equals bit for bit
    (tests/test_gpu_rollout_wrappers.py asserts that equality; the wrapper records no loc / scale of its own, so if it ever loosens, this test fails first and
    the cause is there).  The same comparison with the network row as the key fails."""
    import torch
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    B, base, seed, counter, bounds = 40, 100000, HI_SEED, 2 ** 32 - 1, BOUNDS[0]
    env = SigmaEnv(Parameters(n_agents=16, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, is_using_prioritized_marl=True),
                   n_envs=B, device="cuda:0", env_index_base=base)
    env.reset_random(seed=3)
    N, K, D = env.N, env.K, env.D
    mlp = ph.regime_net(8, obs_dim=D + 2 * K)
    actor = _actor(mlp, bounds, mode)
    g = torch.Generator().manual_seed(5)
    ranks = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32).cuda()
    obs0 = env.obs.clone()
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    lp, acts, tent = z(1, B, N), z(1, B, N, 2), z(1, B, N, K, 2)
    actor.rollout(env, 1, log_prob=lp, actions=acts, seed=seed, counter0=counter, wrapper="prioritized", priority=ranks, tentative=tent)
    env.sync()
    seen = torch.cat([obs0, tent[0].reshape(B, N, 2 * K)], dim=-1).reshape(B * N, D + 2 * K).contiguous()
    ls = _forward(actor, env, seen, seed, counter, deterministic=True)[2]
    a, l = acts[0].reshape(B * N, 2).cpu().numpy(), lp[0].reshape(B * N).cpu().numpy()
    r = ph.check_rows(a, l, ls[:, :2], ls[:, 2:], seed, counter, B, N, base, bounds[0], bounds[1], what=f"row map {mode}", net=mlp)[0]
    _note(r)
    assert r["ok"], r
    assert (tent != 0).any()
    by_network_row = ph.check_rows(a, l, ls[:, :2], ls[:, 2:], seed, counter, B, N, base, bounds[0], bounds[1], rows=np.repeat(np.arange(B), N), net=mlp)[0]
    assert not by_network_row["ok"]
    env.close()
    actor.close()
