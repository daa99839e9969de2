"""The study metrics' arithmetic and host parts (no GPU): the second half of sigmarl_amd/csrc/sigmaenv_eval.h compiled ALONE into a stand-alone program
(tests/host_program.py) against tests/eval_study_check.py -- accumulators, carry, metrics and counts equal the float32 twin bit for bit and hold the derived bars at
(N, B, F) = (1,1,1), (3,5,2), (3,5,3), (6,3,37), (16,257,5), (33,2,4), (64,3,4); every planted defect of the twin misses a bar of its own; the reference's formulas in
fp32 torch hold the looser bar of an fp32 sum; torch's scalar semantics the header relies on; the ctypes mirrors against the header as the host C compiler lays it out;
the bound entry points and the build id's source list; the refusals made before any device call; ``study_summary`` on a result built by hand."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import eval_study_check as sc
import host_program
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["%dx%dx%d" % s for s in sc.SHAPES]


def cases():
    return {name: sc.make_case(*shape, seed=300 + k) for k, (name, shape) in enumerate(zip(NAMES, sc.SHAPES))}


PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_eval.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  rd(in, &n_cases, 4);
  for (int c = 0; c < n_cases; ++c) {
    int32_t d[3];  // N, B, F
    rd(in, d, sizeof d);
    const size_t N = d[0], B = d[1], F = d[2];
    std::vector<float> applied(F * B * N * 2), nominal(F * B * N * 2), rinfo(F * 12 * B * N), carry(B * N * 2, 0.0f), metrics(B * EVL_STUDY_METRICS);
    std::vector<int32_t> t0(B * 4), t1(B * 4);
    std::vector<uint32_t> counts(B * EVL_STUDY_COUNTS);
    rd(in, applied.data(), 4 * applied.size());
    rd(in, nominal.data(), 4 * nominal.size());
    rd(in, rinfo.data(), 4 * rinfo.size());
    rd(in, t0.data(), 4 * t0.size());
    rd(in, t1.data(), 4 * t1.size());
    std::vector<evl_study_acc_t> acc(B);
    for (size_t b = 0; b < B; ++b) { for (int k = 0; k < EVL_STUDY_SUMS; ++k) acc[b].sum[k] = 0.0; acc[b].n_act = 0u; }
    for (size_t f = 0; f < F; ++f)
      for (size_t b = 0; b < B; ++b) {
        const size_t a = (f * B + b) * N;
        const float* ri = rinfo.data() + f * 12 * B * N + b * N;
        evl_study_frame(f == 0, applied.data() + a * 2, nominal.data() + a * 2, ri + EVL_REW_GOAL * B * N, ri + EVL_REW_AGENTS * B * N, ri + EVL_REW_LANE * B * N, (int)N,
                        carry.data() + b * N * 2, &acc[b]);
      }
    for (int k = 0; k < EVL_STUDY_SUMS; ++k)
      for (size_t b = 0; b < B; ++b) fwrite(&acc[b].sum[k], 8, 1, out);
    for (size_t b = 0; b < B; ++b) fwrite(&acc[b].n_act, 4, 1, out);
    for (size_t b = 0; b < B; ++b)
      evl_study_finish(acc[b].sum, acc[b].n_act, t1[b * 4 + 1] - t0[b * 4 + 1], t1[b * 4 + 2] - t0[b * 4 + 2], (uint32_t)F, (int)N, metrics.data() + b * EVL_STUDY_METRICS,
                       counts.data() + b * EVL_STUDY_COUNTS);
    fwrite(carry.data(), 4, carry.size(), out);
    fwrite(metrics.data(), 4, metrics.size(), out);
    fwrite(counts.data(), 4, counts.size(), out);
  }
  const double zero[EVL_STUDY_SUMS] = {0, 0, 0, 0, 0, 0, 0};
  float none[EVL_STUDY_METRICS];
  evl_study_finish(zero, 0u, 0, 0, 0u, 3, none, nullptr);  // F = 0, no try
  fwrite(none, 4, EVL_STUDY_METRICS, out);
  fclose(in); fclose(out);
  printf("ok %%d cases, sums %%d, metrics %%d, counts %%d, rows %%d %%d %%d, nominal %%d %%d %%d %%d\n", (int)n_cases, EVL_STUDY_SUMS, EVL_STUDY_METRICS, EVL_STUDY_COUNTS, EVL_REW_GOAL,
         EVL_REW_AGENTS, EVL_REW_LANE, evl_nominal_from_cbf(0, 0), evl_nominal_from_cbf(1, 0), evl_nominal_from_cbf(0, 1), evl_nominal_from_cbf(1, 1));
  printf("consts %%a %%a %%a %%a %%a\n", (double)EVL_DT, (double)EVL_A_NORM, (double)EVL_J_NORM, (double)EVL_W_COMF, (double)EVL_EPS);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("eval_study_header")
    cs = dict(cases(), fp32=sc.fp32_case())  # (the many-frame case of the fp32-accumulator defect rides along)
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs.values():
            f.write(struct.pack("<3i", c["N"], c["B"], c["F"]))
            for k in ("applied", "nominal", "reward_info", "timer0", "timer1"):
                f.write(np.ascontiguousarray(c[k]).tobytes())
    stdout = host_program.build_and_run(tmp, "eval_study_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(cs)} cases, sums 7, metrics 6, counts 4, rows 1 7 8, nominal 0 0 0 1" in stdout
    raw = open(tmp / "out.bin", "rb").read()
    res, at = {}, 0
    for name, c in cs.items():
        N, B, F = c["N"], c["B"], c["F"]
        got = {}
        for key, dt, shape in (("sums", np.float64, (7, B)), ("n_act", np.uint32, (B,)), ("carry", np.float32, (B, N, 2)), ("metrics", np.float32, (B, 6)), ("counts", np.uint32, (B, 4))):
            n = int(np.prod(shape))
            got[key] = np.frombuffer(raw, dt, n, at).reshape(shape)
            at += n * np.dtype(dt).itemsize
        got["frames"] = np.full(B, F, np.uint32)
        res[name] = got
    none = np.frombuffer(raw, np.float32, 6, at)
    assert at + 24 == len(raw)
    consts = [float.fromhex(v) for v in [ln for ln in stdout.splitlines() if ln.startswith("consts ")][0].split()[1:]]  # EVL_DT, _A_NORM, _J_NORM, _W_COMF, _EPS
    return cs, res, none, consts


def test_the_cases_cover_what_they_claim(header_results):
    cs = cases()
    assert [(c["N"], c["B"], c["F"]) for c in cs.values()] == sc.SHAPES
    assert sc.METRICS == capi.EVAL_STUDY_METRICS and sc.REW_ROWS == capi.EVL_REW_ROWS and len(sc.SUMS) == len(capi.EVAL_STUDY_SUM_NAMES)
    big = cs["16x257x5"]
    ref = sc.reference64(big)
    assert np.array_equal(header_results[1]["16x257x5"]["n_act"], ref["n_act"])  # the header decides the elements an ulp either side of the threshold as float64 does
    assert ref["n_act"].min() > 0 and ref["n_inactive"].min() > 0 and len(set(ref["n_act"].tolist())) > 1
    assert (ref["tries"] == 0).any() and (ref["tries"] > 0).any() and (ref["success"] <= ref["tries"]).all()
    d = np.abs(big["applied"][1:, ..., 0].astype(np.float64) - big["nominal"][1:, ..., 0].astype(np.float64))
    assert ((d > 0) & (d <= sc.EPS)).any() and ((d > sc.EPS) & (d < 1.2 * sc.EPS)).any()  # either side of the threshold, within an ulp or two
    nz = np.abs(big["applied"])[big["applied"] != 0]
    assert nz.min() >= 2.0 ** -10 and (big["applied"] == 0).any() and np.abs(big["applied"][0]).max() > 0  # frame 0 holds stale values
    ri = big["reward_info"]
    assert not np.allclose(ri[:, 11], ri[:, 1] + ri[:, 7] + ri[:, 8]) and big["replaced"].any()
    eq = sc.make_case(6, 3, 5, seed=1, equal=True)
    assert np.array_equal(eq["applied"], eq["nominal"])


@pytest.mark.parametrize("name", NAMES)
def test_header_equals_the_twin_bit_for_bit_and_holds_the_bars(header_results, name):
    cs, res = header_results[:2]
    case, got = cs[name], res[name]
    bars = sc.check(got, case)
    print(name, bars, sc.figures(got, case))
    assert all(bars.values()), bars


def test_no_frame_and_no_try(header_results):
    none = header_results[2]
    assert none[1] == 0.0 and np.isnan(none[[0, 2, 3, 4, 5]]).all()  # the event reward of no frame is an empty sum; a mean enters everything else


@pytest.mark.parametrize("defect", sc.DEFECTS)
def test_every_planted_defect_misses_a_bar_of_its_own(header_results, defect):
    """the sound twin and the header hold every bar in every case; the defective twin misses the bar the defect is about in at least one case, and there the header
    does not compute what the defective twin computes"""
    cs, res = header_results[:2]
    own = {"jerk_from_v": "comfort_reward", "parameters_dt": "comfort_reward", "initial_frame_not_divided": "cbf_activation_rate", "activation_per_env": "counts",
           "normalised_by_nominal": "cbf_activation_degree", "eps_per_element": "cbf_activation_degree", "carry_cleared_at_replacement": "comfort_reward",
           "rew_total": "event_reward", "fp32_accumulators": None}[defect]
    missed = {}
    for name in ("3x5x2", "3x5x3", "6x3x37", "33x2x4", "fp32"):
        ref = sc.reference64(cs[name])
        assert all(sc.check(sc.twin(cs[name]), cs[name], ref=ref).values())
        assert all(sc.check(res[name], cs[name], ref=ref).values())
        bad = sc.twin(cs[name], defect=defect)
        bars = sc.check(bad, cs[name], ref=ref)
        missed[name] = [k for k, v in bars.items() if not v and k != "equal_twin"]
        if missed[name]:
            assert not (sc.same_bits(res[name]["metrics"], bad["metrics"]) and sc.same_bits(res[name]["counts"], bad["counts"])), name
    print(defect, missed)
    if own is None:
        assert missed["fp32"], defect
    else:
        assert any(own in m for m in missed.values()), (defect, missed)
    if defect == "jerk_from_v":
        assert not missed["3x5x2"] and "comfort_reward" in missed["3x5x3"]  # with two frames a_prev is zero: the jerk IS a / dt; the third frame tells


@pytest.mark.parametrize("name", ["3x5x3", "6x3x37", "33x2x4"])
def test_the_reference_formulas_in_fp32_torch_hold_the_looser_bar(header_results, name):
    """... and the header's metrics lie within the two bars' sum of what the reference's own formulas give"""
    case, hdr = header_results[0][name], header_results[1][name]["metrics"].astype(np.float64)
    M = case["F"] * case["N"]
    ref = sc.reference64(case, chain=sc.fp32_sum_chain(M))
    got = sc.torch_reference(case)
    for k, key in enumerate(sc.METRICS[:4]):
        err = np.abs(got[:, k] - ref[key])
        print(name, key, float(err.max()), float(ref["bar_" + key].min()))
        assert (err <= ref["bar_" + key]).all(), key
    assert sc.same_bits(got[:, 4].astype(np.float32), ref["cbf_activation_rate"])
    tight = sc.reference64(case)
    assert (tight["bar_total_reward"] < ref["bar_total_reward"]).all()  # the looser bar is the looser one
    for k, key in enumerate(sc.METRICS[:4]):
        assert (np.abs(hdr[:, k] - got[:, k]) <= ref["bar_" + key] + tight["bar_" + key]).all(), key
    assert sc.same_bits(hdr[:, 4].astype(np.float32), got[:, 4].astype(np.float32))


def test_torch_scalar_semantics_the_header_relies_on(header_results):
    """The header's constants, as its own program prints them, are the nearest fp32 of the reference's Python scalars, and torch applies those scalars as the header
    applies its constants: ``x / 0.1`` on an fp32 tensor is the IEEE fp32 division by fl32(0.1); ``|x| / 3.0`` and ``/ 20.0`` the ones by 3.0f and 20.0f; ``.pow(2)`` is x * x; ``-0.2 * x`` the
    product with fl32(-0.2); ``x + 1e-9`` the sum with fl32(1e-9); ``x > 1e-9`` decides for every fp32 x as ``x > fl32(1e-9)`` does (fl32(1e-9) < 1e-9 is the
    nearest fp32, so no fp32 lies in between, and at fl32(1e-9) itself both are false)."""
    f32 = np.float32
    dt, a_norm, j_norm, w_comf, eps = (f32(v) for v in header_results[3])
    assert [float(v) for v in (dt, a_norm, j_norm, w_comf, eps)] == header_results[3] == [sc.DT, sc.A_NORM, sc.J_NORM, sc.W_COMF, sc.EPS]
    assert (dt, a_norm, j_norm, w_comf, eps) == (f32(0.1), f32(3.0), f32(20.0), f32(0.2), f32(1e-9))
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(100000, generator=g) * torch.exp2(torch.randint(-12, 8, (100000,), generator=g).float())).float()
    xn = x.numpy()
    assert sc.same_bits((x / 0.1).numpy(), xn / dt)
    assert sc.same_bits((x.abs() / 3.0).numpy(), np.abs(xn) / a_norm) and sc.same_bits((x.abs() / 20.0).numpy(), np.abs(xn) / j_norm)
    assert sc.same_bits(x.pow(2).numpy(), xn * xn)
    assert sc.same_bits((-0.2 * x).numpy(), -w_comf * xn)
    small = (x * 1e-9).float()
    assert sc.same_bits((small.abs() + 1e-9).numpy(), np.abs(small.numpy()) + eps)
    around = np.array([np.nextafter(eps, f32(0)), eps, np.nextafter(eps, f32(1))], f32)  # below, at, above the threshold
    assert (torch.from_numpy(around) > 1e-9).tolist() == [False, False, True] == (around > eps).tolist()
    probe = np.concatenate([np.abs(small.numpy()), around])
    assert sc.same_bits((torch.from_numpy(probe) > 1e-9).numpy(), probe > eps) and (probe > eps).any() and not (probe > eps).all()
    # 100 * float32 item in Python double, rounded to fp32, is the fp32 product: 100 has 5 significant bits, the double product is exact
    y = x[:1000]
    assert all(f32(100 * float(v)) == f32(100.0) * f32(v) for v in y.numpy())


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_and_constants_match_the_header(tmp_path):
    if shutil.which("cc") is None:
        pytest.fail("no host C compiler: the header's layout cannot be checked")
    structs = {"sigmaenv_eval_args_t": capi.EvalArgs, "sigmaenv_eval_src_t": capi.EvalSrc, "sigmaenv_eval_study_src_t": capi.EvalStudySrc}
    consts = ["STUDY_SUMS", "STUDY_N_ACT", "STUDY_CARRY", "STUDY_TIMER0"]
    body = ""
    for cname, mirror in structs.items():
        body += f'  printf("{cname} %zu\\n", sizeof({cname}));\n'
        body += "".join(f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));\n' for f in mirror._fields_)
    body += "".join(f'  printf("{c} %d\\n", SIGMAENV_EVAL_{c});\n' for c in consts)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n' + body + '  printf("abi %d\\n", SIGMAENV_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == ctypes.sizeof(mirror)
        for f in mirror._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(mirror, f[0]).offset, (cname, f[0])
    assert ctypes.sizeof(capi.EvalArgs) == 32 and capi.EvalArgs.study.offset == 8  # the switch took the first reserved word: size and the two older fields as they were
    assert ctypes.sizeof(capi.EvalSrc) == 48 and ctypes.sizeof(capi.EvalStudySrc) == 48
    for c in consts:
        assert int(got[c]) == getattr(capi, "EVAL_" + c)
    assert int(got["abi"]) == capi.ABI_VERSION == 5  # new entry points and a reserved word only
    hdr = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_eval.h")).read()
    assert f"#define EVL_STUDY_SUMS {len(capi.EVAL_STUDY_SUM_NAMES)}\n" in hdr and f"#define EVL_STUDY_METRICS {len(capi.EVAL_STUDY_METRICS)} " in hdr
    assert f"#define EVL_STUDY_COUNTS {len(capi.EVAL_STUDY_COUNTS)} " in hdr
    assert capi.EVAL_STUDY_METRICS == sc.METRICS and tuple("sum_" + s for s in sc.SUMS) == capi.EVAL_STUDY_SUM_NAMES
    assert capi.EVL_REW_ROWS == sc.REW_ROWS == tuple(capi.REWARD_INFO_FIELDS.index(n) for n in ("rew_reach_goal", "rew_collide_other_agents", "rew_collide_lane"))
    assert capi.REWARD_INFO_FIELDS[sc.REW_TOTAL] == "rew_total"


ENTRY_POINTS = ("eval_accumulate_study", "eval_study_finish")


def test_the_entry_points_are_bound_and_hashed_into_the_build_id():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ENTRY_POINTS:
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f" sigmaenv_{name}(" in header, name
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_eval.h" in src and "sigmaenv_eval.inc" in src and "../../include/sigmaenv.h" in src
    assert os.path.exists(capi.DEFAULT_LIB), "the library is not built: the build() of the repository's entry module comes first"
    lib = ctypes.CDLL(capi.DEFAULT_LIB)
    assert all(hasattr(lib, "sigmaenv_" + name) for name in ENTRY_POINTS)


def test_the_nominal_rule_asked_of_parameters():
    """``capi.nominal_from_cbf`` is the header's ``evl_nominal_from_cbf`` (whose four values the header program prints) asked of a ``Parameters``"""
    from sigmarl_amd.params import Parameters

    for tr, te, qp in [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]:
        p = Parameters(is_using_cbf_training=tr, is_using_cbf_testing=te, is_solve_qp=qp)
        assert capi.nominal_from_cbf(p) == ((tr or te) and qp)


# ---- refusals before any device call -------------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call():
    import types

    from sigmarl_amd import evaluate as E
    from sigmarl_amd.params import Parameters

    assert E.eval_study_src() is None
    s = E.eval_study_src(initial=True)
    assert (s.applied, s.nominal, s.reward_info, s.timer, s.initial) == (None, None, None, None, 1) and not any(s.reserved)
    s = E.eval_study_src(applied_ptr=4096, timer_ptr=8192)
    assert (s.applied, s.nominal, s.reward_info, s.timer, s.initial) == (4096, None, None, 8192, 0)
    for bad in (dict(applied_ptr=4098), dict(nominal_ptr=4097), dict(reward_info_ptr=4099), dict(timer_ptr=2), dict(applied_ptr=0)):
        with pytest.raises(ValueError, match="evaluation"):
            E.eval_study_src(**bad)
    env = types.SimpleNamespace(B=4, N=16, parameters=Parameters(max_steps=1))
    with pytest.raises(ValueError, match="at least one frame"):
        E.evaluate(env, None, study=True)
    with pytest.raises(ValueError, match="2\\^24"):
        E.evaluate(env, None, n_steps=(1 << 24) // 16, study=True)


# ---- the summary -----------------------------------------------------------------------------------------------------------------------------
def test_study_summary_per_env_and_pooled():
    from sigmarl_amd import evaluate as E

    case = sc.make_case(6, 5, 9, seed=11)
    tw, ref = sc.twin(case), sc.reference64(case)
    acc = {"sums": tw["sums"], "n_act": tw["n_act"]}
    acc.update({name: tw["sums"][k] for k, name in enumerate(capi.EVAL_STUDY_SUM_NAMES)})
    result = {"study": {"metrics": torch.from_numpy(tw["metrics"]), "counts": torch.from_numpy(tw["counts"].astype(np.int32)), "frames": 9}, "study_accumulators": acc, "n_agents": 6}
    s = E.study_summary(result)
    for k, name in enumerate(capi.EVAL_STUDY_METRICS):
        assert sc.same_bits(s["per_env"][name].numpy(), tw["metrics"][:, k])
    ok = ~np.isnan(tw["metrics"][:, 5])
    assert (~ok).any() and s["mean"]["task_success_rate"] == pytest.approx(float(tw["metrics"][ok, 5].astype(np.float64).mean()))
    assert s["mean"]["total_reward"] == pytest.approx(float(tw["metrics"][:, 0].astype(np.float64).mean()))
    assert s["median"]["event_reward"] == float(torch.from_numpy(tw["metrics"][:, 1].copy()).median())
    # pooled: ONE reference run of the 5 envs (a batch of 5 in out_td): the reference's lines in float64 on all elements
    M = 5 * 9 * 6
    S = ref["sums"].sum(axis=1)
    pooled = s["pooled"]
    assert pooled["event_reward"] == pytest.approx(S[0], rel=1e-6) and pooled["comfort_reward"] == pytest.approx(-sc.W_COMF * (S[1] + S[2]) / M, rel=1e-5)
    assert pooled["total_reward"] == pytest.approx(S[0] - sc.W_COMF * (S[1] + S[2]) / M, rel=1e-5)
    assert pooled["cbf_activation_degree"] == pytest.approx(50 * (S[3] / (S[5] + M * 1e-9) + S[4] / (S[6] + M * 1e-9)), rel=1e-5)
    assert pooled["cbf_activation_rate"] == pytest.approx(100 * int(ref["n_act"].sum()) / M)
    assert pooled["num_task_tries"] == int(ref["tries"].sum()) and pooled["task_success_rate"] == pytest.approx(100.0 * int(ref["success"].sum()) / int(ref["tries"].sum()))
    none = dict(result, study=dict(result["study"], counts=torch.zeros(5, 4, dtype=torch.int32)))
    assert E.study_summary(none)["pooled"]["task_success_rate"] is None
