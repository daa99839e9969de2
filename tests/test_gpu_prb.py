"""The prioritized replay buffer on the device (sigmaenv_prb_*, ``learn.PrioritizedBuffer``, ``learn.update(buffer=)``) held to tests/prb_check.py: the levels, total,
q_min, the sampled indices and the refresh's td bit for bit to the float32 twin fed the DEVICE's own leaves (the twin cannot reproduce the device's powf: it starts one
step later), the two powers -- the leaves and the weights -- to float64 within the power's bar.

The bar of the two powers.  The documentation installed with ROCm states no maximum ulp error for powf, so the bar is measured: ``measure_powers`` runs every
power-producing call of this module's cases once on the GPU and ``tools/prb_timing.py`` writes the worst error against float64 to profiles/prb_ratios.json
(``pow_max_ulp_measured``); the bar is TWICE that, capped at 16 ulp (prb_check.POW_CAP_ULP: the eps-dropped defect moves a priority by about 60 ulp at td = 1e-3).

Sizes: the smallest at which each kernel can still go wrong -- len 1, 255, 256, 257 (a second level), 65537 (a third); capacity 512 with len 300; M = 1, 64, 65, 512
slots of the sampler (one wavefront each, four per workgroup); refresh with M = 1, 64, 257 and 16640 = 65 workgroups of 256 (more partials than one wavefront folds
in a single pass)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import prb_check as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]
SEED, COUNTER = 0xA5A5A5A55A5A5A5A, 12
f32 = np.float32

EXTEND_CASES = [(1, 1), (255, 255), (256, 256), (257, 257), (65537, 65537), (512, 300)]  # (capacity, len)
SAMPLE_SHAPES = [(1, 1), (257, 64), (257, 65), (65537, 512)]  # (len, M)
SAMPLE_KINDS = ["random", "all_equal", "one_huge", "chunk_edge"]
REFRESH_CASES = {  # name: (N, F, M, make_refresh_case's switches)
    "n2_m1": (2, 40, 1, {}), "n4_m64": (4, 300, 64, {}), "n2_m257": (2, 100, 257, {}), "n4_m16640": (4, 5000, 16640, {}),
    "duplicates": (4, 300, 64, {"dup": True}), "out_of_range": (4, 300, 64, {"out_of_range": True}), "all_equal": (2, 300, 64, {"equal": True}),
    "done_all": (4, 300, 64, {"done_all": True}),
}


def pow_bar():
    """twice the measured worst error of the device's powf against float64 over this module's inputs, at most 16 ulp"""
    path = os.path.join(ROOT, "profiles", "prb_ratios.json")
    measured = json.load(open(path)).get("pow_max_ulp_measured") if os.path.exists(path) else None
    assert measured is not None, "profiles/prb_ratios.json holds no pow_max_ulp_measured: run tools/prb_timing.py --powers on the GPU first"
    return min(2.0 * float(measured), pc.POW_CAP_ULP)


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def bits(a):
    return np.ascontiguousarray(np.asarray(a), f32).view(np.uint32)


def make_envs():
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters

    return {n: SigmaEnv(Parameters(n_agents=n, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False, max_steps=6), n_envs=8,
                        device="cuda:0") for n in (2, 4)}


@pytest.fixture(scope="module")
def envs():
    es = make_envs()
    for e in es.values():
        e.reset_random(seed=3)
    yield es
    for e in es.values():
        e.close()


def host_levels(buf):
    lv = buf.levels()
    return {"sum": [t.numpy() for t in lv["sum"]], "min": [t.numpy() for t in lv["min"]], "total": lv["total"].numpy(), "q_min": lv["q_min"].numpy()}


def assert_levels_equal_the_twin(buf, leaves):
    got, want = host_levels(buf), pc.build(leaves, buf.len, buf.capacity)
    assert len(got["sum"]) == len(want["sum"]) - 1
    for k in range(len(got["sum"])):
        assert np.array_equal(bits(got["sum"][k]), bits(want["sum"][k + 1])) and np.array_equal(bits(got["min"][k]), bits(want["min"][k + 1])), k + 1
    assert bits(got["total"]) == bits(want["total"]) and bits(got["q_min"]) == bits(want["q_min"])
    return want


def run_extend(env, kind, capacity, length, seed=0):
    """(buffer, td, the device's leaves) after extend of the TD errors of a leaf set"""
    import torch
    from sigmarl_amd import learn

    td = pc.make_td(kind, length, seed)
    buf = learn.PrioritizedBuffer(env, capacity)
    buf.extend(torch.from_numpy(td).cuda())
    return buf, td, buf.priorities().numpy()


def run_sample(buf, M, seed=SEED, counter=COUNTER):
    import torch

    idx, w = buf.sample(M, seed, counter)
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), w.cpu().numpy()


def run_refresh(env, name):
    """A refresh through the C-ABI on synthetic records (the observation part of the rows is NaN: the kernel reads rewards and done flags only).  Returns the case,
    the leaves before and after, td_out and the buffer."""
    import torch
    from sigmarl_amd import capi, learn

    N, F, M, kw = REFRESH_CASES[name]
    assert env.N == N
    D = env.D
    W = N * (D + 1) + 1
    case = pc.make_refresh_case(F, N, M, 100 + len(name) + M, **kw)
    slab = np.full((F, W), np.nan, f32)
    slab[:, N * D:N * D + N], slab[:, N * (D + 1)] = case["reward"], case["done"]
    buf = learn.PrioritizedBuffer(env, F)
    buf.extend(torch.from_numpy(pc.make_td("random", F, 9)).cuda())
    before = buf.priorities().numpy().copy()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in (("slab", slab), ("index", case["index"]), ("v", case["v"]), ("vn", case["vn"]))}
    td = torch.full((M,), -7.0, device="cuda")
    a = capi.PrbRefreshArgs()
    a.n_index, a.index, a.state_value, a.next_state_value, a.slab, a.td_out = M, dev["index"].data_ptr(), dev["v"].data_ptr(), dev["vn"].data_ptr(), dev["slab"].data_ptr(), td.data_ptr()
    a.td_gamma = float(case["td_gamma"])
    torch.cuda.synchronize()
    rc = env.lib.prb_refresh(env.h, buf._h, C.byref(a))
    assert rc == 0, env.lib.last_error(env.h).decode()
    env.sync()
    return case, before, buf.priorities().numpy(), td.cpu().numpy(), buf


def measure_powers(envs):
    """The worst error in ulp of the device's two powers against float64 over every power-producing call of this module's cases (tools/prb_timing.py --powers)."""
    worst = 0.0
    for capacity, length in EXTEND_CASES:
        buf, td, leaves = run_extend(envs[2], "random", capacity, length)
        worst = max(worst, float(pc.ulp_of(leaves, pc.ref_priority(td)).max()))
        buf.close()
    for length, M in SAMPLE_SHAPES:
        for kind in SAMPLE_KINDS:
            buf, td, leaves = run_extend(envs[2], kind, length, length)
            worst = max(worst, float(pc.ulp_of(leaves, pc.ref_priority(td)).max()))
            idx, w = run_sample(buf, M)
            worst = max(worst, float(pc.ulp_of(w, pc.ref_weight(leaves[idx], leaves.min())).max()))
            buf.close()
    for name, (N, F, M, kw) in REFRESH_CASES.items():
        case, before, after, td, buf = run_refresh(envs[N], name)
        ok = (case["index"] >= 0) & (case["index"] < F)
        worst = max(worst, float(pc.ulp_of(after[case["index"][ok]], pc.ref_priority(td[ok])).max()))
        buf.close()
    return worst


@pytest.mark.parametrize("capacity,length", EXTEND_CASES)
def test_extend_leaves_hold_fp64_and_the_levels_equal_the_twin(envs, capacity, length):
    buf, td, leaves = run_extend(envs[2], "random", capacity, length)
    assert leaves.shape == (length,) and buf.len == length and buf.level_sizes == pc.level_sizes(capacity)
    err = pc.ulp_of(leaves, pc.ref_priority(td))
    print("extend", capacity, length, "worst ulp", err.max())
    assert err.max() <= pow_bar()
    lv = assert_levels_equal_the_twin(buf, leaves)
    assert float(lv["q_min"]) == float(leaves.min())
    buf.close()


@pytest.mark.parametrize("kind", SAMPLE_KINDS)
@pytest.mark.parametrize("length,M", SAMPLE_SHAPES)
def test_sample_indices_equal_the_twin_and_the_weights_hold_fp64(envs, length, M, kind):
    buf, td, leaves = run_extend(envs[2], kind, length, length)
    lv = assert_levels_equal_the_twin(buf, leaves)
    idx, w = run_sample(buf, M)
    want, mass, u = pc.sample(lv, length, SEED, COUNTER, M)  # (the host generator's draw 7400)
    assert np.array_equal(idx, want)
    assert pc.admissible(leaves, length, idx, u, lv["total"], len(lv["n"])).all()
    idx2, w2 = run_sample(buf, M)
    assert np.array_equal(idx2, idx) and np.array_equal(bits(w2), bits(w))  # a repeated call repeats its bits
    idx3, _ = run_sample(buf, M, counter=COUNTER + 1)
    assert np.array_equal(idx3, pc.sample(lv, length, SEED, COUNTER + 1, M)[0])
    if M >= 64 and length > 1 and kind == "random":
        assert not np.array_equal(idx3, idx)
    err = pc.ulp_of(w, pc.ref_weight(leaves[idx], lv["q_min"]))
    print("sample", length, M, kind, "worst ulp", err.max())
    assert err.max() <= pow_bar()
    assert np.all(w <= 1.0) and np.all(w[leaves[idx] == lv["q_min"]] == 1.0)
    if kind in ("all_equal", "chunk_edge") or length == 1:
        assert (leaves[idx] == lv["q_min"]).any()
    buf.close()


def test_sample_with_a_nan_leaf_stays_in_range(envs):
    buf, td, leaves = run_extend(envs[2], "nan_leaf", 257, 257)
    assert np.isnan(leaves).sum() == 1
    idx, _ = run_sample(buf, 512)
    assert np.all((idx >= 0) & (idx < 257))
    buf.close()


@pytest.mark.parametrize("name", list(REFRESH_CASES))
def test_refresh(envs, name):
    N, F, M, kw = REFRESH_CASES[name]
    case, before, after, td, buf = run_refresh(envs[N], name)
    idx = case["index"]
    ok = (idx >= 0) & (idx < F)
    tx, ttd = pc.twin_refresh(case)
    assert np.array_equal(bits(td[ok]), bits(ttd[ok]))  # td_out: the twin's x_m and normalisation, bit for bit
    assert np.all(td[~ok] == -7.0)  # an entry outside [0, len) writes nothing
    touched = np.zeros(F, bool)
    touched[idx[ok]] = True
    assert np.array_equal(bits(after[~touched]), bits(before[~touched]))  # the untouched leaves keep their bits
    err = pc.ulp_of(after[idx[ok]], pc.ref_priority(td[ok]))
    print("refresh", name, "worst ulp", err.max())
    assert err.max() <= pow_bar()
    assert_levels_equal_the_twin(buf, after)  # what extend builds from the same leaves (test_extend: extend == the twin)
    if name == "out_of_range":
        assert (~ok).sum() == 2
    if name == "duplicates":
        assert np.unique(idx).size <= M // 4 + 1
    if name == "all_equal":  # the range floor 1e-3 acts: every priority is (1e-3 + eps)^alpha
        assert np.all(td == f32(1e-3)) and np.unique(bits(after[touched])).size == 1
        assert pc.ulp_of(after[touched][:1], pc.ref_priority(np.asarray([1e-3], f32))).max() <= pow_bar()
    if name == "done_all":
        assert np.all(case["done"] == 1.0)
    buf.close()


def _networks(env, seed=1):
    import torch
    from sigmarl_amd.actor import Actor, Critic, make_mlp

    torch.manual_seed(seed)
    amod, cmod = make_mlp(env.D).cuda(), make_mlp(env.N * env.D, n_out=1).cuda()
    return amod, cmod, Actor(amod, low=LOW, high=HIGH), Critic(cmod)


@pytest.mark.parametrize("route", ["device", "torch"])
def test_update_with_a_buffer_equals_the_loop_written_out(envs, route):
    """learn.update(buffer=) on a tiny batch (T = 4, B = 8, minibatches of 8, 2 epochs): bit for bit the loop written out with the buffer's own methods; the sampled
    frames' priorities have moved; update without buffer= still equals ITS loop written out (the permutation route is untouched)."""
    import torch
    from sigmarl_amd import learn

    env = envs[4]
    T, B, N, D, mb = 4, env.B, env.N, env.D, 8
    amod, cmod, actor, critic = _networks(env)
    amod2, cmod2 = copy.deepcopy(amod), copy.deepcopy(cmod)
    from sigmarl_amd.actor import Actor, Critic

    actor2, critic2 = Actor(amod2, low=LOW, high=HIGH), Critic(cmod2)
    env.reset_random(seed=3)
    batch = learn.collect(env, actor, critic, T, gamma=0.99, lmbda=0.9, seed=5, counter0=0)
    env.sync()
    kw = dict(num_epochs=2, minibatch_size=mb, clip_epsilon=0.2, entropy_coeff=1e-2, max_grad_norm=1.0)

    def optimiser(a, am, c, cm):
        return learn.Adam(env, [(a, am), (c, cm)], lr=3e-4) if route == "device" else torch.optim.Adam(list(am.parameters()) + list(cm.parameters()), lr=3e-4)

    buf, buf2 = learn.PrioritizedBuffer(env, T * B), learn.PrioritizedBuffer(env, T * B)
    buf.extend(batch["td_error"])
    buf2.extend(batch["td_error"])
    q0 = buf.priorities().clone()
    assert torch.equal(q0, buf2.priorities())
    opt = optimiser(actor, amod, critic, cmod)
    infos = learn.update(env, actor, critic, amod, cmod, opt, batch, seed=4, counter0=100, buffer=buf, **kw)
    torch.cuda.synchronize()
    assert len(infos) == 2 * (T * B // mb) and all(tuple(i["_weight"].shape) == (mb,) and tuple(i["td_error"].shape) == (mb,) for i in infos)
    # the loop written out
    opt2 = optimiser(actor2, amod2, critic2, cmod2)
    pars2 = list(amod2.parameters()) + list(cmod2.parameters())
    obs, sampled = batch["observation"], []
    for k in range(len(infos)):
        idx, w = buf2.sample(mb, 4, 100 + k)
        sampled.append(idx.cpu())
        out = actor2.apply(env, rows=(obs, 0, N, D, T * B, N * D), index=idx)
        value = critic2.apply(env, obs, index=idx)
        loss, info = learn.ppo_head(env, out, value, batch, idx, low=LOW, high=HIGH, clip_epsilon=0.2, entropy_coeff=1e-2, seed=4, counter=100 + k)
        loss.backward()
        if route == "device":
            opt2.step(1.0)
        else:
            torch.nn.utils.clip_grad_norm_(pars2, 1.0)
            opt2.step()
            opt2.zero_grad()
            actor2.load(env, amod2)
            critic2.load(env, cmod2)
        td = buf2.refresh(critic2, batch, idx)
        assert same(w, infos[k]["_weight"]) and same(td, infos[k]["td_error"]) and same(info["loss_objective"], infos[k]["loss_objective"]), k
        assert float(w.max()) <= 1.0 and 1e-3 <= float(td.min()) and float(td.max()) <= 10.0
    if route == "device":
        opt2.resolve()
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(list(amod.parameters()) + list(cmod.parameters()), pars2))
    q1 = buf.priorities()
    assert same(q1, buf2.priorities())
    hit = torch.unique(torch.cat(sampled)).long()
    assert not torch.equal(q1[hit], q0[hit])  # the sampled frames' priorities are the updated critic's
    rest = torch.ones(T * B, dtype=torch.bool)
    rest[hit] = False
    assert torch.equal(q1[rest], q0[rest])
    assert_levels_equal_the_twin(buf, q1.numpy())
    # without buffer=: the permutation route as before, equal to its loop written out
    amod3, cmod3 = copy.deepcopy(amod), copy.deepcopy(cmod)
    actor3, critic3 = Actor(amod3, low=LOW, high=HIGH), Critic(cmod3)
    opt, opt3 = optimiser(actor, amod, critic, cmod), optimiser(actor3, amod3, critic3, cmod3)
    plain = learn.update(env, actor, critic, amod, cmod, opt, batch, seed=4, counter0=200, generator=torch.Generator(device="cuda").manual_seed(9), **kw)
    assert "_weight" not in plain[0] and "td_error" not in plain[0]
    gen3, k, pars3 = torch.Generator(device="cuda").manual_seed(9), 0, list(amod3.parameters()) + list(cmod3.parameters())
    for _ in range(2):
        for idx in learn.minibatches(T * B, mb, gen3):
            out = actor3.apply(env, rows=(obs, 0, N, D, T * B, N * D), index=idx)
            value = critic3.apply(env, obs, index=idx)
            loss, info = learn.ppo_head(env, out, value, batch, idx, low=LOW, high=HIGH, clip_epsilon=0.2, entropy_coeff=1e-2, seed=4, counter=200 + k)
            loss.backward()
            if route == "device":
                opt3.step(1.0)
            else:
                torch.nn.utils.clip_grad_norm_(pars3, 1.0)
                opt3.step()
                opt3.zero_grad()
                actor3.load(env, amod3)
                critic3.load(env, cmod3)
            assert same(info["loss_objective"], plain[k]["loss_objective"])
            k += 1
    if route == "device":
        opt3.resolve()
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(list(amod.parameters()) + list(cmod.parameters()), pars3))
    assert same(buf.priorities(), q1)  # (a run without buffer= does not touch a buffer)
    for n in (actor, critic, actor2, critic2, actor3, critic3, buf, buf2):
        n.close()


def test_refusals_before_any_launch(envs):
    import torch
    from sigmarl_amd import capi, learn

    env = envs[2]
    EINVAL = -22
    for bad in (dict(capacity=0), dict(capacity=8, alpha=1.5), dict(capacity=8, alpha=-0.1), dict(capacity=8, beta=-1.0), dict(capacity=8, eps=-1e-8)):
        with pytest.raises(ValueError):
            learn.PrioritizedBuffer(env, **bad)
    h = C.c_void_p()
    assert env.lib.prb_create(env.h, 8, 1.5, 0.6, 1e-8, C.byref(h)) == EINVAL and not h.value and b"alpha" in env.lib.last_error(env.h)
    assert env.lib.prb_create(env.h, 8, 0.7, -0.5, 1e-8, C.byref(h)) == EINVAL and env.lib.prb_create(None, 8, 0.7, 0.6, 1e-8, C.byref(h)) == EINVAL
    buf = learn.PrioritizedBuffer(env, 8)
    with pytest.raises(ValueError):
        buf.sample(4, 0, 0)  # empty
    with pytest.raises(TypeError):
        buf.extend(torch.ones(8))  # a CPU tensor
    with pytest.raises(TypeError):
        buf.extend(torch.ones(8, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        buf.extend(torch.ones(9, device="cuda"))  # beyond the capacity
    td = torch.ones(8, device="cuda")
    assert env.lib.prb_extend(env.h, buf._h, None, 8) == EINVAL and env.lib.prb_extend(env.h, buf._h, C.c_void_p(td.data_ptr()), 0) == EINVAL
    assert env.lib.prb_extend(env.h, buf._h, C.c_void_p(td.data_ptr()), 9) == EINVAL and env.lib.prb_extend(env.h, buf._h, C.c_void_p(td.data_ptr() + 2), 4) == EINVAL
    assert env.lib.prb_extend(env.h, None, C.c_void_p(td.data_ptr()), 8) == EINVAL
    buf.extend(td)
    with pytest.raises(ValueError):
        buf.sample(0, 0, 0)
    idx, w = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda")
    assert env.lib.prb_sample(env.h, buf._h, 0, 0, 0, C.c_void_p(idx.data_ptr()), C.c_void_p(w.data_ptr())) == EINVAL
    assert env.lib.prb_sample(env.h, buf._h, 4, 0, 0, None, C.c_void_p(w.data_ptr())) == EINVAL
    assert env.lib.prb_sample(env.h, buf._h, 4, 0, 0, C.c_void_p(idx.data_ptr()), C.c_void_p(w.data_ptr() + 1)) == EINVAL
    a = capi.PrbRefreshArgs()
    assert env.lib.prb_refresh(env.h, buf._h, C.byref(a)) == EINVAL  # M = 0, null tensors
    a.n_index, a.index, a.state_value, a.next_state_value, a.td_gamma = 4, idx.data_ptr(), w.data_ptr(), w.data_ptr(), 0.9
    assert env.lib.prb_refresh(env.h, buf._h, C.byref(a)) == EINVAL and b"slab" in env.lib.last_error(env.h)  # a null record
    out = (C.c_float * 8)()
    assert env.lib.prb_get(env.h, buf._h, 99, out) == EINVAL and env.lib.prb_get(env.h, buf._h, capi.PRB_LEAVES, None) == EINVAL
    with pytest.raises(TypeError):
        buf.refresh(None, {"observation": None, "slab": None}, torch.zeros(4, dtype=torch.int64, device="cuda"))  # index is not int32
    with pytest.raises(TypeError):
        learn.update(env, None, None, torch.nn.Linear(1, 1), torch.nn.Linear(1, 1), None, {"observation": torch.zeros(1, 8, 2, env.D)}, num_epochs=1, minibatch_size=4,
                     clip_epsilon=0.2, entropy_coeff=0.0, max_grad_norm=1.0, buffer="not a buffer")
    torch.cuda.synchronize()
    assert torch.equal(buf.priorities(), torch.ones(8))  # (the refusals launched nothing: the leaves are extend's, fl(1 + 1e-8)^0.7 = 1)
    buf.close()
    buf.close()  # (idempotent)
    with pytest.raises(RuntimeError):
        buf.sample(4, 0, 0)
