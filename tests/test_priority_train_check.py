"""tests/priority_train_check.py on the host (no GPU): the float64 reference's analytical gradients against torch float64 autograd of the same formulas, the float32
twin inside the criterion, every planted defect outside it, the cases the device test runs, the new draw id against the table of sigmarl_amd/csrc/sigmaenv_dist.h
compiled ALONE into a stand-alone program (tests/host_program.py: with AddressSanitizer + UBSan where the compiler has them), and the ctypes mirrors of the new
arguments against the header as the host C compiler lays them out."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import host_program
import observation_check
import policy_head_check as phc
import ppo_head_check as pc
import prb_check
import priority_train_check as pt
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return pt.synthetic_case()


@pytest.fixture(scope="module")
def ref(case):
    return pt.head(case)


def test_every_branch_is_populated_by_the_reference_alone(case, ref):
    p = pc.populations(ref)
    print(p)
    for k in ("inside_pos", "inside_neg", "above_pos", "above_neg", "below_pos", "below_neg", "e_small", "e_large", "sigma_floor"):
        assert p[k] >= 8, (k, p)
    assert p["y_max"] <= 0.999 + 1e-6 and ref["rows"] >= pt.FULL_ROWS
    idx = case["index"]
    assert len(np.unique(idx)) < len(idx) and not np.array_equal(idx, np.arange(len(idx)))
    assert 0 < int(ref["dlw_on"].sum()) < ref["dlw_on"].size
    # the rows that tell clamp(score) from the affine map: tiny scores at the scale's floor, inside the band, the gradient flowing
    rows = np.isin(idx, case["small"])
    assert rows.sum() >= 8 and np.abs(ref["y"][rows]).max() < 1e-3 and ref["sigma"][rows].max() < 0.0101 and ref["dlw_on"][rows].all()


def test_analytical_gradients_equal_torch_float64_autograd(case, ref):
    import torch

    out = torch.from_numpy(case["out"]).double().requires_grad_()
    value = torch.from_numpy(case["value"]).double().requires_grad_()
    z = torch.from_numpy(pt.draws(case))
    lo, le, lc = pt.torch_head(out, value, torch.from_numpy(case["index"].astype(np.int64)), case, z, torch.float64)
    (lo + le + lc).backward()
    for got, want in ((float(lo.detach()), ref["result"]["loss_objective"]), (float(le.detach()), ref["result"]["loss_entropy"]), (float(lc.detach()), ref["result"]["loss_critic"])):
        assert abs(got - float(want)) <= 1e-12 * max(1.0, abs(got))
    # (2^-30 of S: ppo_head_check's allowance for torch's softplus threshold)
    assert (np.abs(ref["dout_actor"] - out.grad.numpy()) <= 2.0 ** -30 * ref["S_dout_actor"]).all()
    assert (np.abs(ref["dout_critic"] - value.grad.numpy()) <= 2.0 ** -30 * ref["S_dout_critic"]).all()


def test_the_twin_passes(case):
    r, _ = pt.check(*pt.twin_outputs(case), case, what="twin")
    assert r["ambiguous_rows"] == 0
    assert max(r["dloc"], r["draw"], r["dcritic"]) <= 1.0 + 1e-12  # (the twin defines the constants)


@pytest.mark.parametrize("defect", pt.DEFECTS)
def test_a_planted_defect_fails(case, defect):
    r, _ = pt.compare(*pt.twin_outputs(case, defect), case, what=defect)
    print(defect, {k: r[k] for k in ("dloc", "draw", "dcritic")}, {k: (v["err"], v["bound"]) for k, v in r["scalars"].items()})
    assert not r["ok"]


def test_the_entropy_draws_are_their_own_stream_and_the_cosine_branch(case):
    M, N = case["out"].shape[:2]
    f = np.repeat(case["index"].astype(np.uint32), N)
    n = np.tile(np.arange(N), M).astype(np.uint32)
    z = pt.draws(case)
    pair = phc.normals(case["seed"], case["counter"], f, n, pt.ENTROPY_DRAWS)
    assert np.array_equal(z.reshape(-1), pair[0]) and not np.allclose(z.reshape(-1), pair[1])
    for other in (pc.ENTROPY_DRAWS, phc.PRIORITY_DRAWS, phc.ACTOR_DRAWS):
        assert not np.allclose(z.reshape(-1), phc.normals(case["seed"], case["counter"], f, n, other)[0])
    i, j = 0, 2  # a frame picked twice draws the same number in both slots (the key is the frame, not the slot)
    assert case["index"][i] == case["index"][j] and np.array_equal(z[i], z[j])


@pytest.mark.parametrize("M,N", pt.DEVICE_CASES)
@pytest.mark.parametrize("out_of_range", [False, True])
def test_the_twin_passes_the_device_cases_and_clips_the_references_rows(M, N, out_of_range):
    case, ref, c, moved = pt.device_case(M, N, out_of_range)
    assert ref["rows"] == M * N and not pt.in_the_band(ref, c).any()
    idx, F = case["index"], case["scores"].shape[0]
    outside = (idx < 0) | (idx >= F)
    assert int(outside.sum()) == int(out_of_range) and (M == 1 or len(np.unique(idx)) < M)
    twin = pt.head(case, np.float32)
    assert twin["clipped"] == ref["clipped"]
    da, dc, res = pt.twin_outputs(case)
    r, _ = pt.check(da, dc, res, case, what=f"twin M={M} N={N} out_of_range={out_of_range}")
    assert r["ambiguous_rows"] == 0 and res[4].tobytes() == pt.exact_clip_fraction(ref).tobytes()
    # an entry outside the records: zero gradients, and the sums are those of the case without its rows' terms (the means still divide by M N)
    assert not da[outside].any() and not dc[outside].any() and not ref["dout_actor"][outside].any()
    if M > 8000:
        assert pc.sum_depth(M * N) == 6 + 3 + 3 + 6  # the final sum's third pass


def test_the_device_cases_lie_where_they_are_said_to():
    groups = [-(-M * N // 256) for M, N in pt.DEVICE_CASES]
    assert groups == [1, 1, 2, 1, 1, 129, 130] and (85 * 3, 86 * 3) == (255, 258)


def test_a_small_case_takes_the_calibration_constants():
    small = pt.synthetic_case(M=5, N=5, F=37, seed=9, floor_rows=1, small_rows=1)
    r, ref = pt.check(*pt.twin_outputs(small), small, what="small twin")
    cal = pt.calibration()
    assert ref["rows"] < pt.FULL_ROWS and all(r["c"][k] >= cal[k] for k in cal)
    for defect in ("no_slope", "critic_sum_over_m", "draw_entropy", "sine", "base_advantage"):
        assert not pt.compare(*pt.twin_outputs(small, defect), small)[0]["ok"], defect


# ---- the draw table ---------------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_dist.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
#define ROW(name) printf("table " #name " %%u\n", (unsigned)(name))
  ROW(AUTO_RESET_MAX_TRIES); ROW(DRAW_RESET_TRY); ROW(DRAW_RESET_SPEED); ROW(DRAW_AGENT_TRY); ROW(DRAW_AGENT_SPEED); ROW(DRAW_SCENARIO); ROW(DRAW_ACTOR);
  ROW(DRAW_PRIORITY); ROW(DRAW_SHUFFLE); ROW(DRAW_ENTROPY); ROW(DRAW_PRIORITY_ENTROPY); ROW(DRAW_REPLAY); ROW(DRAW_OBS_NOISE);
  int32_t K = 0;
  uint64_t seed = 0, counter = 0;
  if (fread(&K, 4, 1, in) != 1 || fread(&seed, 8, 1, in) != 1 || fread(&counter, 8, 1, in) != 1) return 2;
  std::vector<uint32_t> env((size_t)K), agent((size_t)K), w0((size_t)K), w1((size_t)K);
  std::vector<float> z((size_t)K);
  if (fread(env.data(), 4, (size_t)K, in) != (size_t)K || fread(agent.data(), 4, (size_t)K, in) != (size_t)K) return 2;
  for (int k = 0; k < K; ++k) {
    w0[k] = rng_u32(seed, counter, env[k], agent[k], DRAW_PRIORITY_ENTROPY);
    w1[k] = rng_u32(seed, counter, env[k], agent[k], DRAW_PRIORITY_ENTROPY + 1u);
    z[k] = rng_normal_cos(seed, counter, env[k], agent[k], DRAW_PRIORITY_ENTROPY);
  }
  fwrite(w0.data(), 4, (size_t)K, out); fwrite(w1.data(), 4, (size_t)K, out); fwrite(z.data(), 4, (size_t)K, out);
  fclose(in); fclose(out);
  printf("ok %%d keys\n", (int)K);
  return 0;
}
"""


def test_the_new_draw_id_is_disjoint_from_every_other_in_the_table(tmp_path):
    """sigmaenv_dist.h compiled alone: the table with the new entry, its words equal to the Python generator's bit for bit, and the normal the cosine branch of them"""
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    seed, counter = (0xABCD1234 << 32) | 77, 5
    env, agent = phc.row_keys(300, 7, 4096)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<iQQ", env.size, seed, counter))
        f.write(env.tobytes() + agent.tobytes())
    stdout = host_program.build_and_run(tmp_path, "draw_table", PROGRAM % dict(inp=str(tmp_path / "in.bin"), out=str(tmp_path / "out.bin")))
    assert f"ok {env.size} keys" in stdout
    t = {p[1]: int(p[2]) for p in (line.split() for line in stdout.splitlines()) if len(p) == 3 and p[0] == "table"}
    assert (t["DRAW_PRIORITY_ENTROPY"], t["DRAW_PRIORITY_ENTROPY"] + 1) == pt.ENTROPY_DRAWS and t["DRAW_PRIORITY_ENTROPY"] == capi.PRIORITY_ENTROPY_DRAW
    # every id of the table: the try ranges, the pairs, the single draws, the open-ended noise range from its base on
    tries = 2 * t["AUTO_RESET_MAX_TRIES"]
    ids = (list(range(t["DRAW_RESET_TRY"], t["DRAW_RESET_TRY"] + tries)) + [t["DRAW_RESET_SPEED"]] + list(range(t["DRAW_AGENT_TRY"], t["DRAW_AGENT_TRY"] + tries))
           + [t["DRAW_AGENT_SPEED"], t["DRAW_SCENARIO"], t["DRAW_SHUFFLE"], t["DRAW_REPLAY"]]
           + [t[k] + d for k in ("DRAW_ACTOR", "DRAW_PRIORITY", "DRAW_ENTROPY", "DRAW_PRIORITY_ENTROPY") for d in (0, 1)])
    assert len(set(ids)) == len(ids) and max(ids) < t["DRAW_OBS_NOISE"]
    assert (t["DRAW_ACTOR"], t["DRAW_ACTOR"] + 1) == phc.ACTOR_DRAWS and (t["DRAW_PRIORITY"], t["DRAW_PRIORITY"] + 1) == phc.PRIORITY_DRAWS
    assert (t["DRAW_ENTROPY"], t["DRAW_ENTROPY"] + 1) == pc.ENTROPY_DRAWS and t["DRAW_REPLAY"] == prb_check.DRAW and t["DRAW_OBS_NOISE"] == observation_check.NOISE_DRAW
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    K = env.size
    assert np.array_equal(raw[:K], phc.rng_u32(seed, counter, env, agent, pt.ENTROPY_DRAWS[0])) and np.array_equal(raw[K:2 * K], phc.rng_u32(seed, counter, env, agent, pt.ENTROPY_DRAWS[1]))
    z = raw[2 * K:].view(np.float32).astype(np.float64)
    z64, _ = phc.normals(seed, counter, env, agent, pt.ENTROPY_DRAWS)
    zm, _ = phc.normals(seed, counter, env, agent, pt.ENTROPY_DRAWS, magnitude=True)
    assert (np.abs(z - z64) <= pt.MARGIN * pt.U23 * zm).all()  # (the host's libm is not numpy's: a few roundings of the draw's own magnitude)


# ---- the arguments' layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("cc") is None, reason="no host C compiler")
def test_the_new_arguments_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    f1 = [f[0] for f in capi.PpoHead1dArgs._fields_]
    f2 = [f[0] for f in capi.RolloutOpts._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n'
                   '  printf("size1 %zu\\n", sizeof(sigmaenv_ppo_head_1d_args_t));\n  printf("size2 %zu\\n", sizeof(sigmaenv_rollout_opts_t));\n'
                   + "".join(f'  printf("a.{f} %zu\\n", offsetof(sigmaenv_ppo_head_1d_args_t, {f}));\n' for f in f1)
                   + "".join(f'  printf("o.{f} %zu\\n", offsetof(sigmaenv_rollout_opts_t, {f}));\n' for f in f2) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size1"]) == ctypes.sizeof(capi.PpoHead1dArgs) and int(got["size2"]) == ctypes.sizeof(capi.RolloutOpts)
    for f in f1:
        assert int(got["a." + f]) == getattr(capi.PpoHead1dArgs, f).offset, f
    for f in f2:
        assert int(got["o." + f]) == getattr(capi.RolloutOpts, f).offset, f
    assert f2[-1] == "base_obs_rec"  # the new field is the last one: every earlier offset is what it was
    assert "sigmaenv_ppo_head_1d" in capi.exported_symbols() and "ppo_head_1d" in capi._PRODUCT_ONLY
    assert "int sigmaenv_ppo_head_1d(" in open(os.path.join(ROOT, "include", "sigmaenv.h")).read()


# ---- the padded critic rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", [(1, 7, 0), (3, 5, 2), (4, 32, 2), (16, 35, 3)])
def test_padded_rows_are_the_torch_pad_of_every_agents_segment(N, D, K):
    import torch

    Dc, W = D + 2 * K, N * (D + 1) + 1
    rec = np.random.default_rng(N).standard_normal((9, W)).astype(np.float32)  # record rows: N D next observations, then rewards and the done flag
    got = pt.padded_rows(rec, N, D, Dc)
    want = torch.nn.functional.pad(torch.from_numpy(rec[:, : N * D]).reshape(9, N, D), (0, 2 * K)).reshape(9, N * Dc).numpy()
    assert got.shape == (9, N * Dc) and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not got.reshape(9, N, Dc)[:, :, D:].any() and np.array_equal(got.reshape(9, N, Dc)[:, :, :D].reshape(9, N * D), rec[:, : N * D])


def test_the_padded_entry_points_are_bound():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ("mlp32_forward_rows_pad", "mlp32_forward_save_indexed_pad", "mlp32_backward_indexed_pad"):
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f"int sigmaenv_{name}(" in header
