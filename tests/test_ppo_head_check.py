"""tests/ppo_head_check.py on the host: the float64 reference's analytical gradients against torch float64 autograd of the same formulas, the float32 twin inside
the criterion, every planted defect outside it, and the branch populations of the case that decides it."""
import numpy as np
import pytest

import policy_head_check as phc
import ppo_head_check as pc


@pytest.fixture(scope="module")
def case():
    return pc.synthetic_case()


@pytest.fixture(scope="module")
def ref(case):
    return pc.head(case)


def test_every_branch_is_populated_by_the_reference_alone(case, ref):
    p = pc.populations(ref)
    print(p)
    for k in ("inside_pos", "inside_neg", "above_pos", "above_neg", "below_pos", "below_neg", "e_small", "e_large", "sigma_floor"):
        assert p[k] >= 8, (k, p)
    assert p["y_max"] <= 0.999 + 1e-6                    # the inverse transform is not in its clamp
    assert ref["rows"] >= pc.FULL_ROWS
    idx = case["index"]
    assert len(np.unique(idx)) < len(idx) and not np.array_equal(idx, np.arange(len(idx)))  # duplicates, and not the identity
    # both sides of a strict minimum occur: rows whose gradient is cut, rows whose gradient flows
    assert 0 < int(ref["dlw_on"].sum()) < ref["dlw_on"].size


def test_the_entropy_draws_are_their_own_stream(case):
    z = pc.draws(case)
    M, N = case["out"].shape[:2]
    f = np.repeat(case["index"].astype(np.uint32), N)
    n = np.tile(np.arange(N), M).astype(np.uint32)
    za = np.stack(phc.normals(case["seed"], case["counter"], f, n, phc.ACTOR_DRAWS), -1).reshape(M, N, 2)
    assert np.isfinite(z).all() and not np.allclose(z, za)
    assert pc.ENTROPY_DRAWS == (7300, 7301)
    # a frame picked twice draws the same numbers in both slots (the key is the frame, not the slot)
    i, j = 0, 2
    assert case["index"][i] == case["index"][j] and np.array_equal(z[i], z[j])


def test_analytical_gradients_equal_torch_float64_autograd(case, ref):
    import torch

    out = torch.from_numpy(case["out"]).double().requires_grad_()
    value = torch.from_numpy(case["value"]).double().requires_grad_()
    z = torch.from_numpy(pc.draws(case))
    lo, le, lc = pc.torch_head(out, value, torch.from_numpy(case["index"].astype(np.int64)), case, z, torch.float64)
    (lo + le + lc).backward()
    for got, want in ((float(lo.detach()), ref["result"]["loss_objective"]), (float(le.detach()), ref["result"]["loss_entropy"]), (float(lc.detach()), ref["result"]["loss_critic"])):
        assert abs(got - float(want)) <= 1e-12 * max(1.0, abs(got))
    # (2^-30 of S: torch's softplus is the identity beyond its threshold of 20, so its derivative there is 1 instead of 1 - e^-20 = 1 - 2.1e-9)
    assert (np.abs(ref["dout_actor"] - out.grad.numpy()) <= 2.0 ** -30 * ref["S_dout_actor"]).all()
    assert (np.abs(ref["dout_critic"] - value.grad.numpy()) <= 2.0 ** -30 * ref["S_dout_critic"]).all()


def test_the_twin_passes(case):
    r, _ = pc.check(*pc.twin_outputs(case), case, what="twin")
    assert r["ambiguous_rows"] == 0
    assert max(r["dloc"], r["draw"], r["dcritic"]) <= 1.0 + 1e-12  # (the twin defines the constants)


@pytest.mark.parametrize("defect", pc.DEFECTS)
def test_a_planted_defect_fails(case, defect):
    r, _ = pc.compare(*pc.twin_outputs(case, defect), case, what=defect)
    print(defect, {k: r[k] for k in ("dloc", "draw", "dcritic")}, {k: (v["err"], v["bound"]) for k, v in r["scalars"].items()})
    assert not r["ok"]


def test_a_small_case_takes_the_calibration_constants():
    small = pc.synthetic_case(M=5, N=5, F=37, seed=9, floor_rows=1)
    r, ref = pc.check(*pc.twin_outputs(small), small, what="small twin")
    cal = pc.calibration()
    assert ref["rows"] < pc.FULL_ROWS and all(r["c"][k] >= cal[k] for k in cal)
    for defect in ("no_dsigma_draw", "critic_mean", "smooth_l1_half"):
        assert not pc.compare(*pc.twin_outputs(small, defect), small)[0]["ok"], defect


def test_ordered_sum_is_the_stated_tree():
    g = np.random.default_rng(0)
    for n in (1, 5, 64, 65, 256, 260, 300 * 256 + 7):
        t = g.standard_normal(n).astype(np.float32)
        s = pc.ordered_sum(t)
        assert s.dtype == np.float32
        assert abs(float(s) - float(t.astype(np.float64).sum())) <= pc.sum_depth(n) * 2.0 ** -24 * float(np.abs(t).sum()) * 1.01
        assert float(pc.ordered_sum(t.astype(np.float64))) == pytest.approx(float(t.astype(np.float64).sum()), rel=1e-12, abs=1e-12)
    assert pc.sum_depth(260) == 6 + 3 + 1 + 6 and pc.sum_depth(65 * 256) == 6 + 3 + 2 + 6
    # one wavefront of ones and a lone row in the next workgroup: exact
    t = np.zeros(257, np.float32)
    t[:64], t[256] = 1.0, 0.5
    assert float(pc.ordered_sum(t)) == 64.5


def test_clip_bounds_are_rounded_once():
    lo, hi = pc.clip_bounds(0.2)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert lo == np.float32(np.log1p(-np.float64(np.float32(0.2)))) and hi == np.float32(np.log1p(np.float64(np.float32(0.2))))
