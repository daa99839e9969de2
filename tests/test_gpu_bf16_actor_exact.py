"""sigmaenv_actor_kernel -- what Actor(precision="bf16") and sigmaenv_rollout run -- BIT FOR BIT against the float64 restatement of tests/bf16_actor_check.py, on a
network whose dot products are exact in fp32 in any summation order and on rows none of whose 768 hidden activations lies within twice the error bound of fast_tanh
of a bf16 rounding midpoint: such a row has one possible result.  At every width the kernel takes (D = 8, 16, 24, 32: the K padding of layer 1) and at 1, 255, 256,
257 and 1120 rows (one workgroup holds 256; 1120 is no multiple of it), for a created actor, for its sampled forward and for an actor that got the same weights by
Actor.load (the device pack kernel).  The rows are chosen by the reference's certificate alone, before anything runs; every row the device computes is compared.  No
tolerance: loc with == on the words, the scale within the fp32 softplus's own roundings (policy_head_check.compare_scale with a raw bound of 0).
tests/test_bf16_actor_check.py shows on the host which defects this catches, and which of them the flat bar of the dense-network tests lets through."""
import copy

import numpy as np
import pytest

import bf16_actor_check as bc

pytestmark = pytest.mark.gpu

POOL = 1536  # rows drawn per width: at least 1120 of them are certified (held on the host, tests/test_bf16_actor_check.py)
ROWS = [(1, (1, 1)), (255, (51, 5)), (256, (16, 16)), (257, (257, 1)), (1120, (70, 16))]  # (rows, (n_envs, n_agents))
PAD = 1024   # NaN sentinels behind every output
LOW, HIGH = [-1.0, -0.6], [1.0, 0.6]


@pytest.fixture(scope="module")
def envs():
    from sigmarl_amd.env import SigmaEnv
    from sigmarl_amd.params import Parameters
    made = {}

    def get(B, N):
        if (B, N) not in made:
            made[(B, N)] = SigmaEnv(Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False), n_envs=B,
                                    device="cuda:0")
        return made[(B, N)]

    yield get
    for e in made.values():
        e.close()


def forward(actor, env, obs, **kw):
    """loc_scale [R, 4] (numpy) of Actor.forward into NaN-filled buffers, PAD sentinels behind each of the three outputs"""
    import torch
    R = env.B * env.N
    bufs = [torch.full((k * R + PAD,), float("nan"), device="cuda") for k in (2, 1, 4)]
    act, lp, ls = bufs[0][:2 * R].view(env.B, env.N, 2), bufs[1][:R].view(env.B, env.N), bufs[2][:4 * R].view(env.B, env.N, 4)
    actor.forward(env, act, lp, ls, obs=obs, **kw)
    env.sync()
    for k, b in zip((2, 1, 4), bufs):
        assert torch.isnan(b[k * R:]).all() and not torch.isnan(b[:k * R]).any(), "the kernel wrote beyond an output, or left some of it unwritten"
    return ls.reshape(R, 4).cpu().numpy()


@pytest.mark.parametrize("D", [8, 16, 24, 32])
def test_certified_rows_bit_for_bit(envs, D):
    import torch
    from sigmarl_amd.actor import Actor
    c = bc.case(D, POOL)
    assert c.certified.size >= ROWS[-1][0]
    created = Actor(c.net, LOW, HIGH, precision="bf16")
    loaded = Actor(bc.make_net(D, c.seed + 1000), LOW, HIGH, precision="bf16")  # other weights of the same construction
    try:
        for n, (B, N) in ROWS:
            env = envs(B, N)
            rows = c.certified[:n] if n == ROWS[-1][0] else c.certified[-n:]
            obs = torch.from_numpy(c.x[rows]).cuda()
            det = forward(created, env, obs, deterministic=True)
            r = bc.compare(det, c, rows, f"created, {n} rows")
            print({k: r[k] for k in ("what", "rows", "loc_wrong", "scale_wrong", "scale_ratio_max")})
            assert r["ok"], r["message"]
            sampled = forward(created, env, obs, seed=12345, counter=7)
            assert np.array_equal(sampled.view(np.uint32), det.view(np.uint32)), "a sampled forward's loc_scale differs from the deterministic one's"
            if n == ROWS[0][0]:  # (the first use of the other actor: before its load it computes something else)
                assert not np.array_equal(forward(loaded, env, obs, deterministic=True)[:, :2], det[:, :2])
                loaded.load(env, copy.deepcopy(c.net).cuda())
                env.sync()  # (the load is ordered on this env's stream; the other envs' forwards follow on theirs)
            r = bc.compare(forward(loaded, env, obs, deterministic=True), c, rows, f"loaded, {n} rows")
            assert r["ok"], r["message"]
    finally:
        created.close()
        loaded.close()
