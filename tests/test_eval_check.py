"""The evaluation metrics' arithmetic and host parts (no GPU): sigmarl_amd/csrc/sigmaenv_eval.h compiled ALONE into a stand-alone program (tests/host_program.py: with
AddressSanitizer + UBSan where the compiler has them; a program with its own main, nothing is loaded into Python under a sanitizer) against tests/eval_check.py --
accumulators, metrics and trace equal the float32 twin bit for bit and hold the derived bars at (N, B, F) = (1,1,1), (3,5,2), (6,3,37), (16,257,5), (33,2,3), (64,3,4);
every planted defect of the twin misses a bar; the ctypes mirrors against the header as the host C compiler lays it out; the bound entry points and the build id's
source list; the refusals that happen before any device call; summarize / remove_max_min / composite_score against sigmarl/evaluation_base.py:670-809 written out."""
import ctypes
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import eval_check as vc
import host_program
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["%dx%dx%d" % s for s in vc.SHAPES]


def cases():
    return {name: vc.make_case(*shape, seed=100 + k) for k, (name, shape) in enumerate(zip(NAMES, vc.SHAPES))}


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
    std::vector<float> state(F * B * N * 8), dref(F * B * N), trace(F * B * N * EVL_TRACE_COLS), metrics(B * 4);
    std::vector<uint8_t> ca(F * B * N * N), cf(F * B * N * 4);
    rd(in, state.data(), 4 * state.size());
    rd(in, dref.data(), 4 * dref.size());
    rd(in, ca.data(), ca.size());
    rd(in, cf.data(), cf.size());
    std::vector<evl_acc_t> acc(B);
    for (size_t b = 0; b < B; ++b) acc[b] = evl_acc_t{0.0, 0.0, 0u, 0u, 0u};
    for (size_t f = 0; f < F; ++f)
      for (size_t b = 0; b < B; ++b) {
        const size_t a = (f * B + b) * N;
        evl_frame(state.data() + a * 8, dref.data() + a, ca.data() + a * N, cf.data() + a * 4, (int)N, &acc[b], trace.data() + a * EVL_TRACE_COLS);
      }
    for (size_t b = 0; b < B; ++b) {
      evl_finish(acc[b].sum_speed, acc[b].sum_dref, acc[b].n_aa, acc[b].n_al, acc[b].frames, (int)N, metrics.data() + b * 4);
      fwrite(&acc[b].sum_speed, 8, 1, out); fwrite(&acc[b].sum_dref, 8, 1, out);
      fwrite(&acc[b].n_aa, 4, 1, out); fwrite(&acc[b].n_al, 4, 1, out); fwrite(&acc[b].frames, 4, 1, out);
    }
    fwrite(metrics.data(), 4, metrics.size(), out);
    fwrite(trace.data(), 4, trace.size(), out);
  }
  float nan4[4];
  evl_finish(0.0, 0.0, 0u, 0u, 0u, 3, nan4);  // F = 0
  fwrite(nan4, 4, 4, out);
  fclose(in); fclose(out);
  printf("ok %%d cases, max terms %%d, trace cols %%d, groups %%d %%d %%d %%d %%d, full %%d %%d\n", (int)n_cases, (int)EVL_MAX_TERMS, (int)EVL_TRACE_COLS, evl_group(1), evl_group(3),
         evl_group(16), evl_group(33), evl_group(64), evl_full((1u << 20) - 2u, 16), evl_full((1u << 20) - 1u, 16));
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("eval_header")
    cs = cases()
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs.values():
            f.write(struct.pack("<3i", c["N"], c["B"], c["F"]))
            for k in ("state", "dist_ref", "col_agents", "col_flags"):
                f.write(np.ascontiguousarray(c[k]).tobytes())
    stdout = host_program.build_and_run(tmp, "eval_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(cs)} cases, max terms {vc.MAX_TERMS}, trace cols 8, groups 1 4 16 64 64, full 0 1" in stdout
    raw = open(tmp / "out.bin", "rb").read()
    res, at = {}, 0
    rec = np.dtype([("sum_speed", "<f8"), ("sum_dref", "<f8"), ("n_aa", "<u4"), ("n_al", "<u4"), ("frames", "<u4")])
    assert rec.itemsize == 28
    for name, c in cs.items():
        N, B, F = c["N"], c["B"], c["F"]
        a = np.frombuffer(raw, rec, B, at)
        at += 28 * B
        got = {k: np.ascontiguousarray(a[k]) for k in rec.names}
        got["metrics"] = np.frombuffer(raw, np.float32, B * 4, at).reshape(B, 4)
        at += 16 * B
        got["trace"] = np.frombuffer(raw, np.float32, F * B * N * 8, at).reshape(F, B, N, 8)
        at += 32 * F * B * N
        res[name] = got
    nan4 = np.frombuffer(raw, np.float32, 4, at)
    assert at + 16 == len(raw)
    return cs, res, nan4


def test_the_cases_cover_what_they_claim():
    cs = cases()
    assert [(c["N"], c["B"], c["F"]) for c in cs.values()] == vc.SHAPES
    for c in cs.values():
        N = c["N"]
        ca, cf = c["col_agents"], c["col_flags"]
        if N >= 2:
            only = np.zeros((N, N), bool)
            only[N - 1, N - 2] = only[N - 2, N - 1] = True
            assert not ca[..., ~only].any()
        else:
            assert not ca.any()
        assert not cf[..., : N - 1, 0].any()                          # only the last agent's lanelet byte
        assert not (cf[..., 1:4].any(axis=-1) & (cf[..., 0] != 0)).any()  # the other bytes only where it is clear
    big = cs["16x257x5"]
    v = np.abs(big["state"][..., 5:7])
    assert (v == 0).any() and v[v > 0].min() < 2.0 ** -19 and v.max() > 2.0 and big["col_agents"].any() and big["col_flags"][..., 0].any() and big["col_flags"][..., 1:4].any()
    ref = vc.reference64(big)
    assert len(set(ref["n_aa"].tolist())) > 1 and len(set(ref["n_al"].tolist())) > 1  # the counts differ between envs
    assert (big["state"][..., 3] <= 0).all()  # the signed speed is not the norm


@pytest.mark.parametrize("name", NAMES)
def test_header_equals_the_twin_bit_for_bit_and_holds_the_bars(header_results, name):
    cs, res, _ = header_results
    case, got = cs[name], res[name]
    tw = vc.twin(case)
    bars = vc.check(got, case, tw=tw)
    print(name, bars, vc.figures(got, case))
    assert all(bars.values()), bars
    assert vc.same_bits(got["trace"], tw["trace"])
    assert (got["frames"] == case["F"]).all()


def test_no_frame_gives_nan(header_results):
    assert np.isnan(header_results[2]).all()


@pytest.mark.parametrize("defect", vc.DEFECTS)
def test_every_planted_defect_misses_a_bar(defect):
    """the sound twin holds every bar in every case; the defective twin misses one in at least one case"""
    cs = dict(cases(), fp32=vc.fp32_case())
    missed = {}
    for name in ("3x5x2", "6x3x37", "33x2x3", "fp32"):
        assert all(vc.check(vc.twin(cs[name]), cs[name]).values())
        bars = vc.check(vc.twin(cs[name], defect=defect), cs[name])
        if not all(bars.values()):
            missed[name] = [k for k, v in bars.items() if not v and k != "equal_twin"]
    print(defect, missed)
    assert any(missed.values()), defect  # a bar of its own: differing from the twin alone does not count
    if defect == "fp32_accumulators":
        assert "m0" in missed["fp32"]
    if defect == "padding_garbage":
        assert "16x257x5" not in missed and (missed.get("3x5x2") or missed.get("6x3x37") or missed.get("33x2x3"))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_and_constants_match_the_header(tmp_path):
    if shutil.which("cc") is None:
        pytest.fail("no host C compiler: the header's layout cannot be checked")
    structs = {"sigmaenv_eval_args_t": capi.EvalArgs, "sigmaenv_eval_src_t": capi.EvalSrc}
    consts = ["SUM_SPEED", "SUM_DREF", "N_AA", "N_AL", "FRAMES", "TRACE", "FRAMES_HOST"]
    src = tmp_path / "layout.c"
    body = ""
    for cname, mirror in structs.items():
        body += f'  printf("{cname} %zu\\n", sizeof({cname}));\n'
        body += "".join(f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));\n' for f in mirror._fields_)
    body += "".join(f'  printf("{c} %d\\n", SIGMAENV_EVAL_{c});\n' for c in consts)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigmaenv.h"\nint main(void) {\n' + body + '  printf("abi %d\\n", SIGMAENV_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == ctypes.sizeof(mirror)
        for f in mirror._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(mirror, f[0]).offset, (cname, f[0])
    for c in consts:
        assert int(got[c]) == getattr(capi, "EVAL_" + c)
    assert int(got["abi"]) == capi.ABI_VERSION == 5  # new entry points only: no existing structure changed
    hdr = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_eval.h")).read()
    assert "#define EVL_MAX_TERMS (1 << 24)" in hdr and f"#define EVL_TRACE_COLS {capi.EVL_TRACE_COLS} " in hdr
    assert capi.EVL_MAX_TERMS == vc.MAX_TERMS == 1 << 24 and len(capi.EVAL_TRACE_FIELDS) == capi.EVL_TRACE_COLS == 8
    assert len(capi.EVAL_METRICS) == 4 and len(capi.EVAL_COUNTS) == 3


ENTRY_POINTS = ("eval_create", "eval_destroy", "eval_reset", "eval_accumulate", "eval_finish", "eval_attach", "eval_get")


def test_the_entry_points_are_bound_and_hashed_into_the_build_id():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ENTRY_POINTS:
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f" sigmaenv_{name}(" in header, name
    assert "are NOT affected by an attachment" in header
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_eval.h" in src and "sigmaenv_eval.inc" in src
    hip = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv.hip")).read()
    assert '#include "sigmaenv_eval.h"' in hip and '#include "sigmaenv_eval.inc"' in hip
    if os.path.exists(capi.DEFAULT_LIB):
        lib = ctypes.CDLL(capi.DEFAULT_LIB)
        assert all(hasattr(lib, "sigmaenv_" + name) for name in ENTRY_POINTS)


# ---- refusals before any device call -------------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call():
    from sigmarl_amd import evaluate as E
    from sigmarl_amd.params import Parameters

    env = types.SimpleNamespace(B=4, N=16, parameters=Parameters(max_steps=1))
    assert E.eval_src(env, 0) is None
    s = E.eval_src(env, 5, state_ptr=4096, col_flags_ptr=8192)
    assert (s.state, s.dist_ref, s.col_agents, s.col_flags) == (4096, None, None, 8192) and not any(s.reserved)
    for bad in (dict(state_ptr=4098), dict(dist_ref_ptr=4097), dict(col_agents_ptr=4099), dict(col_flags_ptr=2), dict(state_ptr=0)):
        with pytest.raises(ValueError, match="evaluation"):
            E.eval_src(env, 0, **bad)
    limit = (1 << 24) // 16  # (frames + 1) * N >= 2^24 is refused
    assert E.eval_src(env, limit - 2) is None
    with pytest.raises(ValueError, match="2\\^24"):
        E.eval_src(env, limit - 1)
    with pytest.raises(ValueError, match="at least one frame"):
        E.evaluate(env, None)           # params.max_steps - 1 = 0 frames
    with pytest.raises(ValueError, match="2\\^24"):
        E.evaluate(env, None, n_steps=limit)
    assert [E.group_lanes(n) for n in (1, 2, 3, 16, 33, 64)] == [1, 2, 4, 16, 64, 64] == [vc.group(n) for n in (1, 2, 3, 16, 33, 64)]


def test_evaluation_parameters_makes_the_changes_that_reach_the_env():
    from sigmarl_amd import evaluate as E
    from sigmarl_amd.params import Parameters

    p = Parameters(is_prb=True, is_challenging_initial_state_buffer=True, n_agents=4, max_steps=128, num_vmas_envs=32)
    q = E.evaluation_parameters(p, n_agents=6, simulation_steps=1200, num_envs=32)
    assert (q.is_testing_mode, q.n_agents, q.max_steps, q.num_vmas_envs, q.is_prb, q.is_challenging_initial_state_buffer) == (True, 6, 1200, 32, False, False)
    assert (p.is_testing_mode, p.n_agents, p.max_steps, p.is_prb) == (False, 4, 128, True)  # the input is left as it is
    r = E.evaluation_parameters(p)
    assert (r.is_testing_mode, r.n_agents, r.max_steps, r.num_vmas_envs) == (True, 4, 128, 32)


# ---- the summary against the reference's lines written out ------------------------------------------------------------------------------------
def reference_remove_max_min(tensor):
    """sigmarl/evaluation_base.py:771-809 written out: the first maximum and the first minimum of every row become +-inf (columns 0 and 1 where they are the same
    entry), then everything that is not +-inf is kept"""
    tensor = tensor.clone()
    max_idx = torch.max(tensor, dim=1, keepdim=True).indices
    min_idx = torch.min(tensor, dim=1, keepdim=True).indices
    for r in range(tensor.shape[0]):
        if max_idx[r, 0] == min_idx[r, 0]:
            tensor[r, 0], tensor[r, 1] = float("inf"), float("-inf")
        else:
            tensor[r, max_idx[r, 0]], tensor[r, min_idx[r, 0]] = float("inf"), float("-inf")
    return tensor[(tensor != float("inf")) & (tensor != float("-inf"))].view(tensor.size(0), -1)


def reference_summary(speed, cr_aa, cr_al, dref, agent_width, max_speed, remove=True, relative=True):
    """sigmarl/evaluation_base.py:670-738 written out on [n_models, B] tensors"""
    if remove:
        cr_aa, cr_al, dref, speed = (reference_remove_max_min(x) for x in (cr_aa, cr_al, dref, speed))
    if relative:
        dref = dref / agent_width * 100
        speed = speed / max_speed * 100
    cr_aa, cr_al = cr_aa * 100, cr_al * 100
    cr_sum = cr_aa + cr_al
    out = dict(CR_AA_avg=cr_aa.mean(dim=-1), CR_AL_avg=cr_al.mean(dim=-1), CR_total_avg=cr_sum.mean(dim=-1), CD_avg=dref.mean(dim=-1), AS_avg=speed.mean(dim=-1))
    w1, w2, w3 = 1 / out["CR_total_avg"].mean(), 1 / out["CD_avg"].mean(), 1 / out["AS_avg"].mean()
    out["composite_score"] = -w1 * out["CR_total_avg"] - w2 * out["CD_avg"] + w3 * out["AS_avg"]
    out.update(CR_AA_median=cr_aa.median(dim=-1).values, CR_AL_median=cr_al.median(dim=-1).values, CR_total_median=cr_sum.median(dim=-1).values,
               CD_median=dref.median(dim=-1).values, AS_median=speed.median(dim=-1).values,
               average_speed=speed, collision_rate_with_agents=cr_aa, collision_rate_with_lanelets=cr_al, distance_ref_average=dref, collision_rate_sum=cr_sum)
    return out


ROWS = {
    "unique": torch.tensor([[0.3, 0.1, 0.7, 0.2, 0.5, 0.4], [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]]),
    "ties": torch.tensor([[0.5, 0.1, 0.5, 0.1, 0.3, 0.2], [0.0, 0.0, 0.0, 1.0, 1.0, 0.5], [2.0, 1.0, 1.0, 1.0, 1.0, 2.0]]),
    "all_equal": torch.tensor([[0.25, 0.25, 0.25, 0.25, 0.25], [0.0, 0.0, 0.0, 0.0, 0.0]]),
}


@pytest.mark.parametrize("kind", list(ROWS))
def test_remove_max_min_equals_the_reference_lines(kind):
    from sigmarl_amd import evaluate as E

    t = ROWS[kind]
    keep = t.clone()
    got, want = E.remove_max_min(t), reference_remove_max_min(t)
    assert torch.equal(t, keep)  # the input is left as it is
    assert got.shape == (t.shape[0], t.shape[1] - 2) and torch.equal(got, want)
    if kind == "all_equal":
        assert torch.equal(got, t[:, 2:])  # columns 0 and 1 went
    if kind == "ties":
        assert got[0].tolist() == pytest.approx([0.5, 0.1, 0.3, 0.2])  # only the FIRST maximum and the first minimum went


@pytest.mark.parametrize("remove,relative", [(True, True), (False, True), (True, False)])
def test_summarize_and_composite_score_equal_the_reference_lines(remove, relative):
    from sigmarl_amd import evaluate as E

    g = torch.Generator().manual_seed(3)
    n_models, B = 3, 9
    speed, dref = torch.rand(n_models, B, generator=g), torch.rand(n_models, B, generator=g) * 0.05
    cr_aa = torch.randint(0, 4, (n_models, B), generator=g).float() / 20  # ties, and an all-equal row
    cr_al = torch.randint(0, 6, (n_models, B), generator=g).float() / 20
    cr_aa[1] = 0.0
    want = reference_summary(speed, cr_aa, cr_al, dref, 0.107, 1.0, remove, relative)
    summaries = []
    for k in range(n_models):
        metrics = torch.stack([speed[k], cr_aa[k], cr_al[k], dref[k]], dim=1)  # [B, 4] in capi.EVAL_METRICS order
        s = E.summarize(metrics, 0.107, 1.0, is_remove_max_min=remove, is_relative_values=relative)
        s2 = E.summarize({n: metrics[:, j] for j, n in enumerate(capi.EVAL_METRICS)}, 0.107, 1.0, is_remove_max_min=remove, is_relative_values=relative)
        for key, v in s.items():
            assert torch.equal(v, want[key][k]), (key, k)
            assert torch.equal(v, s2[key])
        summaries.append(s)
    assert torch.equal(E.composite_score(summaries), want["composite_score"])
