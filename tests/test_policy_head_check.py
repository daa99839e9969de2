"""The restatement of the policy heads (tests/policy_head_check.py) held to what it restates, without a GPU: its generator equals the oracle's C function (the
specification the HIP kernels are held to through resets and sensor noise); the criterion the GPU tests use passes a float32 evaluation in another operation
order and rejects every wrong head that was thought of; the sampler's statistics at a size the GPU tests cannot afford; and how well the generator tells
(env, agent) streams apart."""
import math

import numpy as np
import pytest

import network_check as nc
import policy_head_check as ph

HI_SEED = (0xABCD1234 << 32) | 77  # a seed with its high word set


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _oracle_rng(seed, counter, env, agent, draw):
    import oracle_binding as ob
    lib = ob.load_oracle()
    arrs = [np.ascontiguousarray(seed, np.uint64), np.ascontiguousarray(counter, np.uint64)] + [np.ascontiguousarray(v, np.uint32) for v in (env, agent, draw)]
    out = np.zeros(arrs[0].size, np.uint32)
    lib.rng_u32(arrs[0].size, *[ob.ptr(a) for a in arrs], ob.ptr(out))
    return out


# every draw id the project uses: reset tries 2 t / 2 t + 1 and 2000 + ..(64 tries), 1000, 3000, 5000, the policy heads, 9000 + k (sensor noise of a 4096-wide row)
DRAW_IDS = np.concatenate([np.arange(128), [1000], 2000 + np.arange(128), [3000, 5000, 7000, 7001, 7100, 7101, 7200], 9000 + np.arange(4096)]).astype(np.uint32)


def test_rng_u32_equals_the_oracles():
    g = np.random.default_rng(1)
    n = 1 << 20
    seeds = np.array([0, 12345, HI_SEED, 2 ** 64 - 1, 1 << 63, 1 << 32], np.uint64)
    counters = np.array([0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 5, 2 ** 64 - 1], np.uint64)
    seed = np.where(g.random(n) < 0.5, seeds[g.integers(0, seeds.size, n)], g.integers(0, 2 ** 64, n, dtype=np.uint64))
    counter = np.where(g.random(n) < 0.5, counters[g.integers(0, counters.size, n)], g.integers(0, 2 ** 64, n, dtype=np.uint64))
    env = g.integers(0, 2 ** 18 + 1, n, dtype=np.uint32)
    env[:8] = [0, 1, 2 ** 18, 2 ** 18 - 1, 100000, 100256, 2 ** 32 - 1, 2 ** 31]
    agent = g.integers(0, 64, n, dtype=np.uint32)
    draw = DRAW_IDS[g.integers(0, DRAW_IDS.size, n)]
    assert np.array_equal(ph.rng_u32(seed, counter, env, agent, draw), _oracle_rng(seed, counter, env, agent, draw))
    # the full cross of the special values, every draw id (python ints as scalars take the same path as the GPU tests' calls)
    for s in seeds.tolist():
        for c in counters.tolist():
            want = _oracle_rng(np.full(DRAW_IDS.size, s, np.uint64), np.full(DRAW_IDS.size, c, np.uint64), np.full(DRAW_IDS.size, 100000), np.full(DRAW_IDS.size, 3), DRAW_IDS)
            assert np.array_equal(ph.rng_u32(s, c, np.uint32(100000), 3, DRAW_IDS), want)
    # the counter enters with its low word only, the seed with both
    e, a = ph.row_keys(64, 16)
    assert np.array_equal(ph.rng_u32(7, 2 ** 32 + 5, e, a, 7000), ph.rng_u32(7, 5, e, a, 7000))
    assert not np.array_equal(ph.rng_u32(7, 5, e, a, 7000), ph.rng_u32(7 + (1 << 32), 5, e, a, 7000))


def test_uniform_is_the_kernels_float32_expression():
    k = np.array([0, 255, 256, (2 ** 23 - 1) << 8, 2 ** 23 << 8, (2 ** 23 + 1) << 8, (2 ** 23 + 2) << 8, 0xFFFFFFFF], np.uint32)
    u = ph.uniform(k)
    assert u.dtype == np.float32
    # below 2^23 the + 0.5f is exact; from 2^23 on it rounds to even: 2^23 + 0.5 -> 2^23, 2^23 + 1.5 -> 2^23 + 2, 2^24 - 0.5 -> 2^24 (u = 1.0f)
    want = np.array([0.5, 0.5, 1.5, 2 ** 23 - 0.5, 2 ** 23, 2 ** 23 + 2, 2 ** 23 + 2, 2 ** 24], np.float64) * 2.0 ** -24
    assert np.array_equal(u.astype(np.float64), want)
    assert u[-1] == np.float32(1.0) and u.min() == np.float32(2.0 ** -25)
    z0, z1 = ph.normals(0, 0, np.arange(8, dtype=np.uint32), 0)
    assert np.isfinite(z0).all() and np.isfinite(z1).all()


def test_random_ranks_is_the_inside_out_shuffle():
    """The vectorised shuffle against the kernel's loop written out for one env at a time, and a permutation in every row."""
    N, envs = 16, np.arange(100000, 100040, dtype=np.uint32)
    got = ph.random_ranks(21, 5, envs, N)
    for b, e in enumerate(envs.tolist()):
        r = [0] * N
        for i in range(N):
            j = (int(ph.rng_u32(21, 5, np.uint32(e), i, 7200)) * (i + 1)) >> 32
            if j != i:
                r[i] = r[j]
            r[j] = i
        assert got[b].tolist() == r
    assert np.array_equal(np.sort(got, axis=1), np.broadcast_to(np.arange(N), got.shape))
    assert ph.random_ranks(21, 5, envs, 1).tolist() == [[0]] * envs.size


# ---- the criterion: what it passes and what it rejects ------------------------------------------------------------------------------------
LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
B_, N_, BASE, SEED, COUNTER = 257, 16, 100000, 12345, 2 ** 32 + 5


def _head32(loc, scale, z, low, high, mut=None):
    """ph.head(..., float32) written out again with the defects as switches (without one it is bit for bit ph.head: asserted below)"""
    f = np.float32
    loc, scale, z = loc.astype(f), scale.astype(f), z.astype(f)
    low, high = np.asarray(low, f), np.asarray(high, f)
    if mut == "fma":  # another float32 evaluation: x with one rounding
        x = (loc.astype(np.float64) + scale.astype(np.float64) * z.astype(np.float64)).astype(f)
    else:
        x = loc + scale * z
    eps = f(1e-7) if mut == "clamp at 1 - 1e-7" else f(1e-6)
    y = np.minimum(np.maximum(np.tanh(x), f(-1.0) + eps), f(1.0) - eps)
    h = f(0.5) * (high - low)
    action = low + (y + f(1.0)) * h

    def softplus(v):
        with np.errstate(over="ignore"):
            s = np.log1p(np.exp(np.minimum(v, f(80.0))))
        return np.where(v > f(20.0), f(0.0) if mut == "softplus = 0 above 20" else v, s)

    xl = np.arctanh(y) if mut == "log-probability from atanh(clamped y)" else x
    zl = (xl - loc) / scale if mut == "log-probability from atanh(clamped y)" else z
    jac = f(2.0) * (f(ph.LOG2) - xl - softplus(f(-2.0) * xl))
    lp_d = f(-0.5) * zl * zl - np.log(scale) - f(ph.LOG_SQRT_2PI) - jac
    if mut != "- log h missing":
        lp_d = lp_d - np.log(h)
    lp = lp_d[:, 1] + lp_d[:, 0] if mut == "fma" else lp_d[:, 0] + lp_d[:, 1]
    return action, lp


def _scale32(raw, mut=None):
    f = np.float32
    v = raw.astype(f) + f(ph.BIAS)
    with np.errstate(over="ignore"):
        s = np.log1p(np.exp(np.minimum(v, f(80.0))))
    s = np.where(v > f(20.0), f(0.0) if mut == "softplus = 0 above 20" else v, s)
    return np.maximum(s + (f(0.0) if mut == "0.01 floor missing" else f(0.01)), f(1e-4))


def _model(out32, mut=None):
    """What a device with the defect ``mut`` would hand back for the network outputs ``out32`` [rows, 4]: (action, log_prob, loc, scale)"""
    env, agent = ph.row_keys(B_, N_, BASE)
    if mut == "env index without its base":
        env = env - np.uint32(BASE)
    if mut == "agent and env swapped":
        env, agent = agent, env
    draws = (7001, 7000) if mut == "draw ids swapped" else (7000, 7001)
    z0, z1 = ph.normals(SEED, COUNTER + (1 if mut == "counter + 1" else 0), env, agent, draws, np.float32)
    if mut == "sine and cosine swapped":
        z0, z1 = z1, z0
    loc, scale = out32[:, :2], _scale32(out32[:, 2:], mut)
    action, lp = _head32(loc, scale, np.stack([z0, z1], -1), LOW, HIGH, mut)
    return action, lp, loc, scale


def _verdict(out32, raw64, raw_bound, mut=None):
    """The comparison of tests/test_gpu_policy_head.py: every row's action and log-probability from the device's own loc / scale, and the scale itself"""
    action, lp, loc, scale = _model(out32, mut)
    r, _, _ = ph.check_rows(action, lp, loc, scale, SEED, COUNTER, B_, N_, BASE, LOW, HIGH)
    s = ph.compare_scale(scale, raw64, raw_bound)
    return r["ok"] and s["ok"], r, s


DEFECTS = ["sine and cosine swapped", "draw ids swapped", "env index without its base", "counter + 1", "agent and env swapped",
           "log-probability from atanh(clamped y)", "- log h missing", "0.01 floor missing", "softplus = 0 above 20", "clamp at 1 - 1e-7"]


@pytest.fixture(scope="module", params=ph.LAST_LAYER_SCALES, ids=lambda s: f"last-x{s}")
def case(request):
    mlp, x = ph.regime_net(request.param), ph.regime_input(B_ * N_)
    ref64, t32, s = nc.references(mlp, x)
    raw_bound = nc.A * np.abs(t32 - ref64)[:, 2:].max() + nc.B * nc.ulp32(s)  # the network criterion's bound on the raw output
    return request.param, t32.astype(np.float32), ref64[:, 2:], raw_bound


def test_the_float32_twin_and_another_operation_order_pass(case):
    last, out32, raw64, raw_bound = case
    ok, r, s = _verdict(out32, raw64, raw_bound)
    assert ok, (r, s)
    assert r["c_dev"] <= r["c"] and r["c_a_dev"] <= r["c_a"]  # (the twin against itself)
    ok, r2, s2 = _verdict(out32, raw64, raw_bound, "fma")
    assert ok, (r2, s2)
    # the written-out head is the module's
    env, agent = ph.row_keys(B_, N_, BASE)
    z32 = np.stack(ph.normals(SEED, COUNTER, env, agent, dtype=np.float32), -1)
    tw = ph.head(out32[:, :2], ph.scale_of(out32[:, 2:], np.float32), z32, LOW, HIGH, np.float32)
    a, lp = _head32(out32[:, :2], _scale32(out32[:, 2:]), z32, LOW, HIGH)
    assert np.array_equal(a, tw["action"]) and np.array_equal(lp, tw["log_prob"])


def test_the_regimes_hold_their_rows(case):
    """Each regime of the head has at least 16 values in the case that is meant to cover it (counted on the CPU with the GPU tests' own inputs and key)."""
    last, out32, raw64, raw_bound = case
    action, lp, loc, scale = _model(out32)
    r, ref, z = ph.check_rows(action, lp, loc, scale, SEED, COUNTER, B_, N_, BASE, LOW, HIGH)
    n = ph.regime_counts(ref["x"], scale, z)
    print(last, n, {k: v for k, v in r.items() if k != "what"})
    need = {1: dict(inside=16), 8: dict(tanh_is_one=16, shortcut_jacobian=16, scale_floor=16, inside=16),
            30: dict(tanh_is_one=16, shortcut_jacobian=16, shortcut_scale=16, scale_floor=16, inside=16)}[last]
    for k, least in need.items():
        assert n[k] >= least, (last, k, n)
    if last == 1:  # the statistical test of tests/test_gpu_actor.py allows 5e-3 on this regime: the bound of EVERY row is at least 100 x below it
        assert r["lp_bound_median"] <= r["lp_bound_max"] <= 5e-3 / 100


# last layer x 1 has no saturated row and nothing above 20: these defects change nothing there (asserted below), x 8 and x 30 cover them
INVISIBLE_AT_X1 = ["softplus = 0 above 20", "clamp at 1 - 1e-7"]


@pytest.mark.parametrize("case,defect", [(last, d) for last in ph.LAST_LAYER_SCALES for d in DEFECTS if not (last == 1 and d in INVISIBLE_AT_X1)], indirect=["case"],
                         ids=lambda v: f"last-x{v}" if isinstance(v, int) else v)
def test_wrong_heads_are_rejected(case, defect):
    last, out32, raw64, raw_bound = case
    ok, r, s = _verdict(out32, raw64, raw_bound, defect)
    assert not ok, (defect, r, s)


@pytest.mark.parametrize("case", [1], indirect=True, ids=["last-x1"])
@pytest.mark.parametrize("defect", INVISIBLE_AT_X1)
def test_defects_that_need_saturation_are_invisible_without_it(case, defect):
    """Why the two combinations are not among the rejections: the defective head returns the very bits of the sound one on this case."""
    last, out32, raw64, raw_bound = case
    ok, r, s = _verdict(out32, raw64, raw_bound, defect)
    assert ok and r["saturated"] == 0
    assert all(np.array_equal(a, b) for a, b in zip(_model(out32, defect), _model(out32)))


def test_clamp_defect_is_caught_by_the_exact_rows_alone(case):
    """A clamp at another epsilon moves a saturated action by less than 1e-6: only the exact comparison of the saturated rows sees it."""
    last, out32, raw64, raw_bound = case
    ok, r, s = _verdict(out32, raw64, raw_bound, "clamp at 1 - 1e-7")
    if last == 1:
        assert r["saturated"] == 0
    else:
        assert r["saturated"] >= 16 and r["saturated_wrong"] == r["saturated"]


def test_priority_head_variant_and_its_defects():
    """The 1-D head: the twin passes; drawing the actor's ids (7000 / 7001), the sine branch, and a wrong scale fail."""
    mlp, x = ph.regime_net(8, "priority"), ph.regime_input(B_ * N_)
    ref64, t32, _ = nc.references(mlp, x)
    out32 = t32.astype(np.float32)
    env, agent = ph.row_keys(B_, N_, BASE)

    def device(draws=ph.PRIORITY_DRAWS, branch=0, floor=0.01):
        z = ph.normals(SEED, COUNTER, env, agent, draws, np.float32)[branch][:, None]
        sc = np.maximum(ph.scale_of(out32[:, 1:], np.float32) - np.float32(0.01) + np.float32(floor), np.float32(1e-4))
        t = ph.head(out32[:, :1], sc, z, None, None, np.float32)
        return t["action"], t["log_prob"]

    def ok(score, lp):
        return ph.check_rows(score, lp, out32[:, :1], None, SEED, COUNTER, B_, N_, BASE, draws=ph.PRIORITY_DRAWS, raw=out32[:, 1:])[0]["ok"]

    assert ok(*device())
    # last layer x 1: the statistical test of tests/test_gpu_rollout_wrappers.py allows 2e-3 (and leaves |x| > 4 out): the bound of every row is 100 x below
    m1 = ph.regime_net(1, "priority")
    o1 = nc.references(m1, x)[1].astype(np.float32)
    t1 = ph.head(o1[:, :1], ph.scale_of(o1[:, 1:], np.float32), ph.normals(SEED, COUNTER, env, agent, ph.PRIORITY_DRAWS, np.float32)[0][:, None], None, None, np.float32)
    r1 = ph.check_rows(t1["action"], t1["log_prob"], o1[:, :1], None, SEED, COUNTER, B_, N_, BASE, draws=ph.PRIORITY_DRAWS, raw=o1[:, 1:])[0]
    assert r1["ok"] and r1["lp_bound_median"] <= r1["lp_bound_max"] <= 2e-3 / 100, r1
    assert not ok(*device(draws=ph.ACTOR_DRAWS))
    assert not ok(*device(branch=1))
    assert not ok(*device(floor=0.0))


# ---- the sampler's statistics ---------------------------------------------------------------------------------------------------------------
def _normal_quantile(p_two_sided):
    """q with P(|Z| > q) = p for a standard normal Z (bisection on erfc)"""
    lo, hi = 0.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / math.sqrt(2.0)) > p_two_sided else (lo, mid)
    return 0.5 * (lo + hi)


def test_sampler_statistics_of_four_million_draws():
    """16 counters x 2048 envs x 64 agents x (z0, z1) = 4.2e6 draws of the restated sampler (seed with the high word set, counters across 2^32, envs of a shard
    at 100000).  Every bound is that of an ideal standard normal sample of this size at the two-sided quantile 1e-6, computed here."""
    P = 1e-6
    q = _normal_quantile(P)
    assert 4.89 < q < 4.90
    C, E, N = 16, 2048, 64
    counter = (2 ** 32 - 8 + np.arange(C, dtype=np.uint64))[:, None, None]
    env = (100000 + np.arange(E, dtype=np.uint32))[None, :, None]
    agent = np.arange(N, dtype=np.uint32)[None, None, :]
    z0, z1 = ph.normals(HI_SEED, counter, env, agent)
    z = np.stack([z0, z1], -1)
    n = z.size
    assert n >= 4_000_000 and z.shape == (C, E, N, 2)
    # moments: mean (variance 1), second (variance of z^2: 2), fourth (variance of z^4: 105 - 9 = 96)
    assert abs(z.mean()) <= q / math.sqrt(n)
    assert abs((z ** 2).mean() - 1.0) <= q * math.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) <= q * math.sqrt(96.0 / n)
    # Kolmogorov distance to the normal CDF: P(D > d) <= 2 exp(-2 n d^2) (Dvoretzky-Kiefer-Wolfowitz)
    zs = np.sort(z.reshape(-1))
    cdf = 0.5 * (1.0 + _erf(zs / math.sqrt(2.0)))
    k = np.arange(1, n + 1)
    D = max(float((k / n - cdf).max()), float((cdf - (k - 1) / n).max()))
    assert D <= math.sqrt(math.log(2.0 / P) / (2.0 * n)), D
    # correlations of an ideal sample: r sqrt(m) is standard normal to first order
    def corr(a, b):
        return float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]), a.size

    for name, (r, m) in {"z0-z1": corr(z[..., 0], z[..., 1]), "neighbouring agents": corr(z[:, :, :-1], z[:, :, 1:]), "neighbouring envs": corr(z[:, :-1], z[:, 1:]),
                         "consecutive counters": corr(z[:-1], z[1:]), "z0 of agent i - z1 of agent i + 1": corr(z[:, :, :-1, 0], z[:, :, 1:, 1])}.items():
        assert abs(r) <= q / math.sqrt(m), (name, r, m)
    # the 24-bit uniforms bound the radius: u1 >= 2^-25
    zmax = float(np.abs(z).max())
    assert zmax <= math.sqrt(2.0 * math.log(2.0 ** 25)) < 5.89
    assert zmax > 4.5  # (an ideal sample of this size stays below 4.5 with probability exp(-n P(|Z| > 4.5)) = exp(-28))
    # the float32 draws of the twin are the float64 ones to a few float32 roundings of the radius
    t0, t1 = ph.normals(HI_SEED, counter[:2], env, agent, dtype=np.float32)
    assert max(np.abs(t0 - z0[:2]).max(), np.abs(t1 - z1[:2]).max()) <= 2e-6


def _erf(x):
    """erf on an array without scipy: numpy has none, math.erf is scalar -- evaluated on a grid fine enough for linear interpolation (error <= h^2 / 8 * max|erf''|
    = 1e-9 at h = 1e-4) where |x| < 6, +-1 beyond."""
    h = 1e-4
    grid = np.arange(-6.0, 6.0 + h, h)
    vals = np.fromiter((math.erf(v) for v in grid), np.float64, grid.size)
    return np.interp(x, grid, vals, left=-1.0, right=1.0)


# ---- how well the key tells streams apart -----------------------------------------------------------------------------------------------------
def _duplicate_streams(N, B):
    env, agent = ph.row_keys(B, N)
    keys = ph.stream_key(env, agent)
    uniq, counts = np.unique(keys, return_counts=True)
    return keys.size - uniq.size, int(counts.max())


@pytest.mark.parametrize("N,B,duplicates", [(16, 4096, 4), (16, 32768, 14), (16, 262144, 1571)])
def test_stream_key_collisions_are_what_the_specification_gives(N, B, duplicates):
    """Two (env, agent) streams with the same key receive the same noise at every step.  The counts are a property of the generator's pre-mix (DESIGN.md has the
    table): an ideal 32-bit key would give about n^2 / 2^33 = 0.5, 32, 2048.  Asserted exactly, so that a change of the mixing is a visible decision."""
    dup, mult = _duplicate_streams(N, B)
    assert dup == duplicates and mult <= 3


def test_no_two_agents_of_one_env_share_a_stream():
    """Inside one env the key differs by the agent term alone, an odd multiple: a bijection of the agent index."""
    for N in range(1, 65):
        env, agent = ph.row_keys(64, N, 100000)
        k = ph.stream_key(env, agent).reshape(64, N)
        assert all(np.unique(row).size == N for row in k)
    # and equal keys mean equal draws at any seed, counter and draw id
    env, agent = ph.row_keys(4096, 16)
    keys = ph.stream_key(env, agent)
    order = np.argsort(keys, kind="stable")
    same = np.flatnonzero(keys[order][1:] == keys[order][:-1])
    assert same.size == 4
    i, j = order[same], order[same + 1]
    for draw in (7000, 7001, 7100):
        assert np.array_equal(ph.rng_u32(HI_SEED, 9, env[i], agent[i], draw), ph.rng_u32(HI_SEED, 9, env[j], agent[j], draw))
