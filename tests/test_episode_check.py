"""The episode return's arithmetic and the training loop's host parts (no GPU): sigmarl_amd/csrc/sigmaenv_episode.h compiled ALONE into a stand-alone program
(tests/host_program.py: with AddressSanitizer + UBSan where the compiler has them) against tests/episode_check.py -- the header's record, carry, sum, count and
mean equal the float32 twin bit for bit and hold the derived float64 bound, and every planted defect of the twin misses a bar; learn.lr_at against the loop of
_update_learning_rate written out; the ctypes mirror of sigmaenv_episode_args_t against the header as the host C compiler lays it out; the bound entry point and the
build id's source list; the argument refusals that happen before any device call.

Cases (hand-made records, no env): done at t = 0, at t = T - 1, on consecutive steps, nowhere (K = 0: NaN mean, the carry grows), in every frame, at random; each with
a zero and with a non-zero incoming carry; T = 1; a single env and a single agent; more envs than the 256 lanes of the last sum (257, 600); a record buffer wider
than the case's envs.  Rewards of mixed sign over 2^-20 .. 2^4."""
import ctypes
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import episode_check as ec
import host_program
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    c = {}
    for k, pattern in enumerate(ec.PATTERNS):
        c[pattern] = ec.make_case(7, 5, 3, 2, pattern, seed=10 + k)
        c[pattern + "_carry"] = ec.make_case(9, 6, 4, 3, pattern, seed=30 + k, carry=True)
    c["one_step"] = ec.make_case(1, 4, 3, 2, "mixed", seed=50, carry=True)
    c["one_step_done"] = ec.make_case(1, 4, 3, 2, "all", seed=51, carry=True)
    c["one_env_one_agent"] = ec.make_case(12, 1, 1, 4, "mixed", seed=52)
    c["envs_257"] = ec.make_case(5, 257, 2, 1, "mixed", seed=53, carry=True)
    c["envs_600_all"] = ec.make_case(3, 600, 2, 1, "all", seed=54, carry=True)
    c["wider_buffer"] = ec.make_case(6, 5, 3, 2, "mixed", seed=55, carry=True, Bt=12, env_first=4)
    c["sixteen_agents"] = ec.make_case(33, 48, 16, 1, "mixed", seed=56, carry=True)
    return c


NAMES = [p + s for p in ec.PATTERNS for s in ("", "_carry")] + ["one_step", "one_step_done", "one_env_one_agent", "envs_257", "envs_600_all", "wider_buffer",
                                                                  "sixteen_agents"]

PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_episode.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  rd(in, &n_cases, 4);
  for (int c = 0; c < n_cases; ++c) {
    int32_t d[6];  // T, B, N, D, Bt, env_first
    rd(in, d, sizeof d);
    const int T = d[0], B = d[1], N = d[2], D = d[3], Bt = d[4], e0 = d[5];
    const int64_t W = (int64_t)N * (D + 1) + 1;
    std::vector<float> slab((size_t)T * Bt * W), carry((size_t)B * N), carry2, E((size_t)T * B * N), s(B);
    std::vector<int32_t> k(B);
    float result[4], result2[4];
    rd(in, slab.data(), 4 * slab.size());
    rd(in, carry.data(), 4 * carry.size());
    carry2 = carry;
    epr_run(slab.data() + (int64_t)e0 * W, (int64_t)Bt * W, T, B, N, D, carry.data(), E.data(), result, s.data(), k.data());
    epr_run(slab.data() + (int64_t)e0 * W, (int64_t)Bt * W, T, B, N, D, carry2.data(), nullptr, result2, s.data(), k.data());  // without the record
    fwrite(E.data(), 4, E.size(), out);
    fwrite(carry.data(), 4, carry.size(), out);
    fwrite(result, 4, 4, out);
    fwrite(carry2.data(), 4, carry2.size(), out);
    fwrite(result2, 4, 4, out);
    const int32_t chain = epr_longest_chain(T, B, N);
    fwrite(&chain, 4, 1, out);
  }
  fclose(in); fclose(out);
  printf("ok %%d cases, lanes %%d, max frames %%d\n", (int)n_cases, (int)EPR_LANES, (int)EPR_MAX_FRAMES);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    """every case through the header compiled alone: {name: {"E", "carry", "S", "mean", "K", "result", "no_record": (carry, result), "chain"}}"""
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("episode_header")
    cs = cases()
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for case in cs.values():
            f.write(struct.pack("<6i", case["T"], case["B"], case["N"], case["D"], case["slab"].shape[1], case["env_first"]))
            f.write(np.ascontiguousarray(case["slab"], np.float32).tobytes())
            f.write(np.ascontiguousarray(case["carry"], np.float32).tobytes())
    stdout = host_program.build_and_run(tmp, "episode_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(cs)} cases, lanes {ec.LANES}, max frames {ec.MAX_FRAMES}" in stdout
    raw = np.fromfile(tmp / "out.bin", np.float32)
    res, at = {}, 0
    for name, case in cs.items():
        T, B, N = case["T"], case["B"], case["N"]
        E = raw[at: at + T * B * N].reshape(T, B, N)
        at += T * B * N
        carry = raw[at: at + B * N].reshape(B, N)
        at += B * N
        result = raw[at: at + 4]
        at += 4
        carry2 = raw[at: at + B * N].reshape(B, N)
        at += B * N
        result2 = raw[at: at + 4]
        at += 4
        chain = int(raw[at: at + 1].view(np.int32)[0])
        at += 1
        res[name] = dict(E=E, carry=carry, mean=result[0], S=result[1], K=int(result[2]), result=result, no_record=(carry2, result2), chain=chain)
    assert at == raw.size
    return cs, res


def test_the_cases_cover_what_they_claim():
    cs = cases()
    assert list(cs) == NAMES
    K = lambda n: int((cs[n]["done"] != 0).sum())  # noqa: E731
    assert cs["done_t0"]["done"][0].all() and not cs["done_t0"]["done"][1:].any()
    assert cs["done_last"]["done"][-1].all() and not cs["done_last"]["done"][:-1].any()
    d = cs["consecutive"]["done"]
    assert ((d[:-1] != 0) & (d[1:] != 0)).any()
    assert K("none") == 0 and K("all") == 7 * 5 and 0 < K("mixed") < 7 * 5
    assert cs["mixed_carry"]["carry"].all() and not cs["mixed"]["carry"].any()
    r = np.abs(cs["mixed"]["reward"])
    assert r.min() < 2.0 ** -16 and r.max() > 2.0 and (cs["mixed"]["reward"] < 0).any() and (cs["mixed"]["reward"] > 0).any()
    assert cs["envs_257"]["B"] == ec.LANES + 1 and cs["envs_600_all"]["B"] > 2 * ec.LANES
    # fp32 order matters on these inputs: the float64 sum of the record differs from the twin's S
    tw = ec.twin(cs["sixteen_agents"])
    assert float(tw["S"]) != ec.reference64(cs["sixteen_agents"], tw["E"])["S"]


@pytest.mark.parametrize("name", NAMES)
def test_header_equals_the_twin_bit_for_bit_and_holds_the_fp64_bound(header_results, name):
    cs, res = header_results
    case, got = cs[name], res[name]
    bars = ec.check(got, case)
    ref = ec.reference64(case, got["E"])
    print(name, bars, "S", got["S"], "S64", ref["S"], "bound", ref["bound_S"], "mean", got["mean"], "mean64", ref["mean"], "bound", ref["bound_mean"])
    assert all(bars.values()), bars
    assert got["chain"] == ec.longest_chain(case["T"], case["B"], case["N"])
    assert got["result"][3] == 0.0
    carry2, result2 = got["no_record"]  # without the record: the same carry and result
    assert ec.same_bits(carry2, got["carry"]) and ec.same_bits(result2, got["result"])
    assert ec.twin_holds_the_recurrence64(case)


def test_no_done_frame_gives_a_nan_mean_and_a_growing_carry(header_results):
    cs, res = header_results
    for name in ("none", "none_carry"):
        case, got = cs[name], res[name]
        assert got["K"] == 0 and got["S"] == 0.0 and np.isnan(got["mean"])
        assert ec.same_bits(got["carry"], got["E"][-1])  # nothing was reset: the carry is the last frame's running return
        assert not ec.same_bits(got["carry"], case["carry"])


def test_the_done_frame_carries_the_episode_and_the_next_starts_from_zero(header_results):
    cs, res = header_results
    case, got = cs["all_carry"], res["all_carry"]
    assert ec.same_bits(got["E"][0], case["carry"] + case["reward"][0])  # the incoming carry belongs to the first frame's episode
    assert ec.same_bits(got["E"][1:], case["reward"][1:])                # every later frame is an episode of one step
    assert not got["carry"].any()


@pytest.mark.parametrize("defect", ec.DEFECTS)
def test_every_planted_defect_misses_a_bar(defect):
    """the sound twin holds every bar in every case; the defective twin misses one in at least one case"""
    cs = cases()
    missed = {}
    for name in ("done_t0_carry", "consecutive_carry", "mixed_carry", "mixed", "sixteen_agents"):
        assert all(ec.check(ec.twin(cs[name]), cs[name]).values())
        bars = ec.check(ec.twin(cs[name], defect=defect), cs[name])
        if not all(bars.values()):
            missed[name] = [k for k, v in bars.items() if not v]
    print(defect, missed)
    assert missed, defect


# ---- the schedule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iters", [1, 2, 250])
def test_lr_at_equals_the_loop_of_update_learning_rate(n_iters):
    """sigmarl/mappo_cavs.py:126-150 with :517-525 written out: the rate iteration i_iter trains at is what the previous iteration's end set, from pbar.n BEFORE
    pbar.update()"""
    from sigmarl_amd import learn
    from sigmarl_amd.params import Parameters

    p = Parameters(n_iters=n_iters)
    lr_now, n, trained_at = p.lr, 0, []
    for _ in range(n_iters + 2):  # (two more than the reference runs: the formula is held there too)
        trained_at.append(lr_now)
        lr_decay = (p.lr - p.lr_min) * (1 - (n / p.n_iters))  # _update_learning_rate
        lr_now = p.lr_min + lr_decay
        n += 1                                                 # pbar.update()
    for k, want in enumerate(trained_at, start=1):
        assert learn.lr_at(p, k) == want, k
    assert learn.lr_at(p, 1) == p.lr and abs(learn.lr_at(p, 2) - p.lr) <= 2.0 ** -52 * p.lr  # the one-iteration lag
    if n_iters >= 2:
        assert learn.lr_at(p, 3) < learn.lr_at(p, 2) and learn.lr_at(p, n_iters) > p.lr_min


def test_set_lr_writes_both_kinds_of_optimiser():
    from sigmarl_amd import learn

    w = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.Adam([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}], lr=1.0)
    learn.set_lr(opt, 0.25)
    assert [g["lr"] for g in opt.param_groups] == [0.25, 0.25]
    mine = learn.Adam.__new__(learn.Adam)
    mine.lr = 1.0
    learn.set_lr(mine, 0.125)
    assert mine.lr == 0.125


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_episode_args_layout_and_constants_match_the_header(tmp_path):
    if shutil.which("cc") is None:
        pytest.fail("no host C compiler: the header's layout cannot be checked")
    fields = [f[0] for f in capi.EpisodeArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sigmaenv_episode_args_t));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(sigmaenv_episode_args_t, {f}));\n' for f in fields)
                   + '  printf("abi %d\\n", SIGMAENV_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(capi.EpisodeArgs)
    for f in fields:
        assert int(got[f]) == getattr(capi.EpisodeArgs, f).offset, f
    assert int(got["abi"]) == capi.ABI_VERSION == 5  # a new entry point only: no existing structure changed
    hdr = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_episode.h")).read()
    assert f"#define EPR_LANES {capi.EPR_LANES} " in hdr and "#define EPR_MAX_FRAMES (1 << 24)" in hdr
    assert capi.EPR_LANES == ec.LANES and capi.EPR_MAX_FRAMES == ec.MAX_FRAMES == 1 << 24


def test_the_entry_point_is_bound_and_hashed_into_the_build_id():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    assert "sigmaenv_episode_return" in capi.exported_symbols() and "episode_return" in capi._PRODUCT_ONLY and "int sigmaenv_episode_return(" in header
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_episode.h" in src and "sigmaenv_episode.inc" in src
    hip = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv.hip")).read()
    assert '#include "sigmaenv_episode.h"' in hip and '#include "sigmaenv_episode.inc"' in hip
    if os.path.exists(capi.DEFAULT_LIB):
        assert hasattr(ctypes.CDLL(capi.DEFAULT_LIB), "sigmaenv_episode_return")


# ---- refusals before any device call -------------------------------------------------------------------------------------------------------
def _fake_env(B=4, N=3, D=5):
    return types.SimpleNamespace(B=B, N=N, D=D, device=torch.device("cpu"), parameters=None)


def test_refusals_before_any_device_call():
    """learn.episode_args makes the library's refusals on the host, before the call: an env without a library is never reached"""
    from sigmarl_amd import learn

    env = _fake_env()
    own = env.B * (env.N * (env.D + 1) + 1)
    good = dict(T=2, slab_ptr=4096, slab_stride=own, carry_ptr=8192, result_ptr=12288)
    a = learn.episode_args(env, **good)
    assert (a.n_steps, a.slab, a.slab_stride, a.carry, a.result, a.episode_reward) == (2, 4096, own, 8192, 12288, None) and not any(a.reserved) and a.reserved0 == 0
    assert learn.episode_args(env, **dict(good, slab_stride=0)).slab_stride == 0 and learn.episode_args(env, **dict(good, slab_stride=2 * own)).slab_stride == 2 * own
    for bad in (dict(T=0), dict(T=-3), dict(T=(1 << 24) // env.B), dict(slab_stride=own - 1), dict(carry_ptr=None), dict(carry_ptr=0), dict(slab_ptr=None),
                dict(result_ptr=None), dict(carry_ptr=8194), dict(episode_reward_ptr=6)):
        with pytest.raises(ValueError, match="episode return"):
            learn.episode_args(env, **dict(good, **bad))
    assert learn.episode_args(env, **dict(good, T=(1 << 24) // env.B - 1)).n_steps == (1 << 22) - 1  # the largest T * B below 2^24
    er = learn.EpisodeReturns(env)
    assert er.carry.shape == (4, 3) and not er.carry.any()
    er.carry += 1.0
    er.reset()
    assert not er.carry.any()
    W = env.N * (env.D + 1) + 1
    with pytest.raises(TypeError, match="slab"):
        er.update(torch.zeros(2, 4, W))       # host memory
    with pytest.raises(TypeError, match="slab"):
        er.update(torch.zeros(2, 4, W + 1))
    with pytest.raises(TypeError, match="returns"):
        learn.collect(env, None, None, 2, gamma=0.99, lmbda=0.9, returns=object())
    with pytest.raises(TypeError, match="returns"):
        learn.collect(env, None, None, 2, gamma=0.99, lmbda=0.9, returns=learn.EpisodeReturns(_fake_env()))  # another env's


def test_train_iteration_refuses_before_any_device_call():
    from sigmarl_amd import learn
    from sigmarl_amd.params import Parameters

    env = _fake_env(B=8)
    er = learn.EpisodeReturns(env)
    p = Parameters(num_vmas_envs=8, max_steps=6)
    with pytest.raises(ValueError, match="multiple"):
        learn.train_iteration(env, None, None, None, None, None, er, p, frames_per_batch=50)
    with pytest.raises(ValueError, match="multiple"):
        learn.train_iteration(env, None, None, None, None, None, er, p, frames_per_batch=4)
    with pytest.raises(ValueError, match="1-based"):
        learn.train_iteration(env, None, None, None, None, None, er, p, i_iter=0)
    with pytest.raises(ValueError, match="is_prb"):
        learn.train_iteration(env, None, None, None, None, None, er, Parameters(num_vmas_envs=8, max_steps=6, is_prb=True))
    assert learn.steps_per_iteration(p, 48, num_epochs=2, minibatch_size=16) == 6 and learn.steps_per_iteration(Parameters(num_epochs=3, minibatch_size=20), 48) == 6


def test_train_tracks_the_best_mean_as_save_intermediate_model_does(monkeypatch):
    """sigmarl/mappo_cavs.py:468-515 on a stubbed iteration: the rounded mean is compared AFTER the rounding, a NaN never improves, and where nothing improved
    episode_reward_mean_current falls back to the best so far"""
    from sigmarl_amd import learn
    from sigmarl_amd.params import Parameters

    raw = [1.004, 1.0049, 0.5, float("nan"), 1.006, -3.0]
    seen = []
    monkeypatch.setattr(learn, "train_iteration", lambda *a, i_iter, **k: (seen.append((i_iter, k)), ({"i": i_iter}, [i_iter], {"episode_reward_mean": torch.tensor(raw[i_iter - 1])}))[1])
    p = Parameters()
    assert p.episode_reward_intermediate == -1e3
    calls, track = [], []
    env = _fake_env()

    def on_iteration(i_iter, batch, infos, mean, improved):
        calls.append((i_iter, batch["i"], infos[0], improved))
        track.append((p.episode_reward_mean_current, p.episode_reward_intermediate))

    means = learn.train(env, None, None, None, None, None, p, n_iters=len(raw), on_iteration=on_iteration, seed=3, counter0=7)
    assert means[:3] == [1.0, 1.0, 0.5] and np.isnan(means[3]) and means[4:] == [1.01, -3.0]
    assert [c[3] for c in calls] == [True, False, False, False, True, False]  # 1.0049 rounds to 1.00: not above the best 1.00
    assert [c[:3] for c in calls] == [(k, k, k) for k in range(1, 7)]
    assert track == [(1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.01, 1.01), (1.01, 1.01)]
    assert [s[0] for s in seen] == list(range(1, 7)) and all(s[1]["seed"] == 3 and s[1]["counter0"] == 7 and s[1]["buffer"] is None for s in seen)
    given = []
    assert learn.train(env, None, None, None, None, None, p, n_iters=1, episode_reward_mean_list=given) is given and given == [1.0]


def test_mean_is_the_reported_number():
    from sigmarl_amd import learn

    assert learn.EpisodeReturns.mean({"episode_reward_mean": torch.tensor(1.23456)}) == 1.23
    assert learn.EpisodeReturns.mean({"episode_reward_mean": torch.tensor(-0.005001)}) == round(float(torch.tensor(-0.005001)), 2)
    assert np.isnan(learn.EpisodeReturns.mean({"episode_reward_mean": torch.tensor(float("nan"))}))
