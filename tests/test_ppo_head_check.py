"""tests/ppo_head_check.py on the host: the float64 reference's analytical gradients against torch float64 autograd of the same formulas, the float32 twin inside
the criterion, every planted defect outside it, and the branch populations of the case that decides it.  Past 64 workgroups (the sizes the device test runs: 64, 65
and 129) the twin passes and counts the reference's clipped rows, and two faults of the final sum that no smaller size can show fail."""
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


@pytest.mark.parametrize("pattern", pc.BIG_PATTERNS)
@pytest.mark.parametrize("M", list(pc.BIG_M))
def test_the_twin_passes_past_64_workgroups_and_clips_the_references_rows(M, pattern):
    """The sizes of tests/test_gpu_ppo_update.py's large cases on the host: no row is left in the branch band, the float32 twin clips exactly the rows the float64
    reference clips, passes the criterion and gives the exact clip_fraction."""
    rows, groups, chain = pc.BIG_M[M]
    case, ref, c, moved = pc.big_case(M, pattern)
    assert ref["rows"] == rows == M * pc.BIG_N and -(-rows // 256) == groups and -(-groups // 64) == chain == pc.sum_depth(rows) - 15
    assert not pc.in_the_band(ref, c).any()
    idx = case["index"]
    assert (len(np.unique(idx)) < M) == (pattern == "duplicates") and not np.array_equal(idx, np.sort(idx))
    twin = pc.head(case, np.float32)
    print(f"M={M} {pattern}: {moved} rows moved out of the band, {ref['clipped']} of {rows} rows clipped")
    assert twin["clipped"] == ref["clipped"] and 0 < ref["clipped"] < rows
    da, dc, res = pc.twin_outputs(case)
    r, _ = pc.check(da, dc, res, case, what=f"twin M={M} {pattern}")
    assert r["ambiguous_rows"] == 0
    assert res[4].tobytes() == pc.exact_clip_fraction(ref).tobytes()


def test_a_row_planted_in_the_band_is_moved_out_of_it():
    small = pc.synthetic_case(M=300, N=4, F=320, seed=5, floor_rows=2)
    ref = pc.head(small)
    m, n = (int(v) for v in np.argwhere(ref["lw"] > 0.3)[0])  # a row above the band ...
    small["sample_log_prob"][small["index"][m], n] += np.float32(ref["lw"][m, n] - float(ref["hi"]))  # ... put on the upper clip bound, to rounding
    ref = pc.head(small)
    assert pc.in_the_band(ref, pc.constants_in_force(small, ref))[m, n]
    moved_case, ref2, c2, moved = pc.clear_of_the_band(small)
    assert moved >= 1 and not pc.in_the_band(ref2, c2).any() and ref2["lw"][m, n] > float(ref["hi"]) + 0.04
    assert small["sample_log_prob"] is not moved_case["sample_log_prob"] and pc.in_the_band(pc.head(small), pc.constants_in_force(small, pc.head(small)))[m, n]


@pytest.mark.parametrize("defect", pc.SUM_DEFECTS)
def test_a_fault_of_the_final_sum_fails_past_its_threshold(case, defect):
    """first_64 is the gap the large cases close: it passes every size the suite had (the host's 1536 and 25 rows, the device's 5 .. 260 rows: at most 6 workgroups)
    with the very bits of the sound twin, and fails once a 65th workgroup exists.  stride_32 needs a 33rd."""
    small = pc.synthetic_case(M=5, N=5, F=37, seed=9, floor_rows=1)
    for old in (case, small, pc.synthetic_case(N=5, F=37, seed=72, index=np.arange(52, dtype=np.int32) % 37, floor_rows=2)):
        assert -(-old["out"].shape[0] * old["out"].shape[1] // 256) <= 6
        got, sound = pc.twin_outputs(old, defect), pc.twin_outputs(old)
        assert all(np.array_equal(a, b) for a, b in zip(got, sound)) and pc.compare(*got, old)[0]["ok"]
    for M, (rows, groups, chain) in pc.BIG_M.items():
        big, ref, c, _ = pc.big_case(M, "duplicates")
        da, dc, res = pc.twin_outputs(big, defect)
        r, _ = pc.compare(da, dc, res, big, what=f"{defect} M={M}")
        exact = res[4].tobytes() == pc.exact_clip_fraction(ref).tobytes()
        print(defect, M, r["ok"], exact, {k: (v["err"], v["bound"]) for k, v in r["scalars"].items()})
        if defect == "first_64" and groups <= 64:
            assert r["ok"] and exact  # (every lane has one workgroup: nothing is lost)
        else:
            assert not r["ok"] and not exact


def test_ordered_sum_is_the_stated_tree():
    g = np.random.default_rng(0)
    for n in (1, 5, 64, 65, 256, 260, 64 * 256 + 1, 128 * 256 + 5, 300 * 256 + 7):
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
    # G = 65 and G = 129: lane 0's chain has a second and a third term; a lone row in the 65th and in the 129th workgroup arrives, every row counts once
    assert -(-(64 * 256 + 1) // 256) == 65 and -(-(128 * 256 + 5) // 256) == 129 and pc.sum_depth(128 * 256 + 5) == 6 + 3 + 3 + 6
    t = np.zeros(128 * 256 + 5, np.float32)
    t[0], t[64 * 256], t[128 * 256 + 4] = 1.0, 0.5, 0.25
    assert float(pc.ordered_sum(t)) == 1.75 and float(pc.ordered_sum(t[: 64 * 256 + 1])) == 1.5
    assert float(pc.ordered_sum(t, "first_64")) == 1.0 and float(pc.ordered_sum(t, "stride_32")) == 2.5  # (never read; read by the lanes 0 and 32)
    for n in (64 * 256, 64 * 256 + 1, 128 * 256 + 5):
        assert float(pc.ordered_sum(np.ones(n, np.float32))) == n
        assert float(pc.ordered_sum(np.ones(n, np.float32), "stride_32")) > n


def test_clip_bounds_are_rounded_once():
    lo, hi = pc.clip_bounds(0.2)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert lo == np.float32(np.log1p(-np.float64(np.float32(0.2)))) and hi == np.float32(np.log1p(np.float64(np.float32(0.2))))
