"""Communication noise on the host (no GPU): sigmarl_amd/csrc/sigmaenv_dist.h compiled ALONE into a stand-alone program (tests/host_program.py) against
tests/comm_noise_check.py -- comm_noise_seen and comm_noise_std equal the float32 twin bit for bit (also when the compiler is told to contract and has an fma),
whole rows composed as the gather kernel composes them pass the criterion in the device's place, the new stream overlaps no other DRAW_* range; the planted
defects of the host model each miss a check; and the table of ``check_rollout_wrapper`` / ``params.communication_noise``."""
import struct
import subprocess

import numpy as np
import pytest

import comm_noise_check as cn
import host_program
import policy_head_check as ph
from sigmarl_amd import capi
from sigmarl_amd.params import Parameters, check_rollout_wrapper, communication_noise

f32 = np.float32
SEED, COUNTER, ENV_BASE, B, N = 0x1234567890ABCDEF, 2 ** 32 + 77, 4096, 257, 16
LEVEL = 0.1

PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_dist.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
#define ROW(name) printf("table " #name " %%u\n", (unsigned)(name))
  ROW(AUTO_RESET_MAX_TRIES); ROW(DRAW_RESET_TRY); ROW(DRAW_RESET_SPEED); ROW(DRAW_AGENT_TRY); ROW(DRAW_AGENT_SPEED); ROW(DRAW_SCENARIO); ROW(DRAW_ACTOR);
  ROW(DRAW_PRIORITY); ROW(DRAW_SHUFFLE); ROW(DRAW_ENTROPY); ROW(DRAW_PRIORITY_ENTROPY); ROW(DRAW_REPLAY); ROW(DRAW_COMM_NOISE); ROW(COMM_NOISE_MAX_COLUMNS);
  ROW(DRAW_OBS_NOISE);
  // the element: seen = v + std * z, and the position rule
  int32_t n = 0;
  rd(in, &n, 4);
  std::vector<float> v((size_t)n), sd((size_t)n), z((size_t)n), seen((size_t)n);
  rd(in, v.data(), 4 * (size_t)n); rd(in, sd.data(), 4 * (size_t)n); rd(in, z.data(), 4 * (size_t)n);
  for (int k = 0; k < n; ++k) seen[k] = comm_noise_seen(v[k], sd[k], z[k]);
  fwrite(seen.data(), 4, (size_t)n, out);
  float rule[4];
  for (int q = 0; q < 4; ++q) rule[q] = comm_noise_std(q, 3.0f, 5.0f);
  fwrite(rule, 4, 4, out);
  // whole rows as the gather kernel composes them: row r = (env, agent), column q
  int32_t R = 0, n_agents = 0, env_base = 0;
  uint64_t seed = 0, counter = 0;
  float s_v = 0, s_d = 0;
  rd(in, &R, 4); rd(in, &n_agents, 4); rd(in, &env_base, 4); rd(in, &seed, 8); rd(in, &counter, 8); rd(in, &s_v, 4); rd(in, &s_d, 4);
  std::vector<float> clean(4 * (size_t)R), row(4 * (size_t)R);
  rd(in, clean.data(), 16 * (size_t)R);
  for (int r = 0; r < R; ++r)
    for (int q = 0; q < 4; ++q) {
      const float zq = rng_normal_cos(seed, counter, (uint32_t)(env_base + r / n_agents), (uint32_t)(r %% n_agents), DRAW_COMM_NOISE + 2u * (uint32_t)q);
      row[4 * r + q] = comm_noise_seen(clean[4 * r + q], comm_noise_std(q, s_v, s_d), zq);
    }
  fwrite(row.data(), 4, 4 * (size_t)R, out);
  fclose(in); fclose(out);
  printf("ok %%d elements %%d rows\n", (int)n, (int)R);
  return 0;
}
"""


def element_inputs():
    """(v, std, z): random values, zeros of undecided neighbours, a zero std, signed zeros; most products are inexact, so a fused multiply-add would differ"""
    g = np.random.default_rng(4)
    n = 20000
    v = (g.standard_normal(n) * 0.7).astype(f32)
    std = np.abs(g.standard_normal(n) * 0.1).astype(f32)
    z = g.standard_normal(n).astype(f32)
    v[:2000] = 0.0
    std[2000:2500] = 0.0
    v[2500:2600] = -0.0
    return v, std, z


def row_inputs():
    g = np.random.default_rng(6)
    clean = (g.uniform(-1, 1, (B * N, 4)) * np.array([1.0, 0.6, 1.0, 0.6])).astype(f32)
    clean[g.random((B * N, 4)) < 0.4] = 0.0
    return clean


def _write_inputs(path):
    v, std, z = element_inputs()
    s = cn.column_stds(LEVEL)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", v.size) + v.tobytes() + std.tobytes() + z.tobytes())
        f.write(struct.pack("<iiiQQ", B * N, N, ENV_BASE, SEED, COUNTER) + s[0].tobytes() + s[2].tobytes() + row_inputs().tobytes())


def _read_outputs(path, stdout):
    raw = np.fromfile(path, f32)
    n = element_inputs()[0].size
    assert raw.size == n + 4 + 4 * B * N and f"ok {n} elements {B * N} rows" in stdout
    table = {p[1]: int(p[2]) for p in (line.split() for line in stdout.splitlines()) if len(p) == 3 and p[0] == "table"}
    return dict(seen=raw[:n], rule=raw[n:n + 4], rows=raw[n + 4:].reshape(B * N, 4), table=table)


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("comm_noise_header")
    _write_inputs(tmp / "in.bin")
    stdout = host_program.build_and_run(tmp, "comm_noise_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    return _read_outputs(tmp / "out.bin", stdout)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_element_and_the_position_rule_equal_the_twin_bit_for_bit(header):
    v, std, z = element_inputs()
    assert np.array_equal(bits(header["seen"]), bits(cn.seen32(v, std, z)))
    fused = (v.astype(np.float64) + std.astype(np.float64) * z.astype(np.float64)).astype(f32)  # (the product is exact in float64: one rounding, as an fma)
    assert (bits(fused) != bits(header["seen"])).mean() > 0.05                                   # the inputs tell the two apart
    assert np.all(header["seen"][2000:2500] == v[2000:2500])                                     # a zero std: values that compare equal to the clean ones
    assert np.array_equal(header["rule"], np.array([3, 3, 5, 5], f32))                           # by position: [s_v, s_v, s_d, s_d]
    s = cn.column_stds(LEVEL)
    assert s[0] == s[1] == f32(capi.AGENTS["max_speed"] * LEVEL) and s[2] == s[3] == f32(capi.AGENTS["max_steering"] * LEVEL) and s[0] != s[2]
    assert (cn.MAX_SPEED, cn.MAX_STEERING) == (capi.AGENTS["max_speed"], capi.AGENTS["max_steering"])


def test_the_element_is_not_contracted_when_the_compiler_may(tmp_path):
    """The same program built with contraction allowed and, where this CPU has one, the fma instruction enabled: comm_noise_seen is still two roundings."""
    cxx = host_program.compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler")
    _write_inputs(tmp_path / "in.bin")
    src, exe = tmp_path / "fast.cpp", tmp_path / "fast"
    src.write_text(PROGRAM % dict(inp=str(tmp_path / "in.bin"), out=str(tmp_path / "out.bin")))
    with open("/proc/cpuinfo") as f:
        has_fma = any(line.startswith("flags") and " fma " in line + " " for line in f)
    subprocess.check_call([cxx, "-std=gnu++17", "-O2", "-ffp-contract=fast"] + (["-mfma"] if has_fma else []) + ["-I", host_program.CSRC, str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = _read_outputs(tmp_path / "out.bin", run.stdout)
    v, std, z = element_inputs()
    assert np.array_equal(bits(got["seen"]), bits(cn.seen32(v, std, z)))


def test_whole_rows_pass_the_criterion_in_the_devices_place(header):
    """rng_normal_cos + comm_noise_std + comm_noise_seen composed as sigmaenv_turn_gather_noise_kernel composes them, with the host's libm, against float64"""
    env, agent = ph.row_keys(B, N, ENV_BASE)
    clean, std = row_inputs(), cn.column_stds(LEVEL)
    z, z32, zmag = (cn.draws(SEED, COUNTER, env, agent, **kw) for kw in (dict(), dict(dtype=f32), dict(magnitude=True)))
    bound, c = cn.bar(clean, std, z, z32, zmag, SEED, COUNTER)
    want = clean.astype(np.float64) + std.astype(np.float64) * z
    err = np.abs(header["rows"].astype(np.float64) - want)
    print(dict(c=c, err_max=float(err.max()), ratio_max=float((err / bound).max())))
    assert np.isfinite(header["rows"]).all() and (err <= bound).all()
    assert np.abs(cn.seen32(clean, std, z32).astype(np.float64) - want).max() <= bound.max()       # the twin itself
    wrong = np.abs(cn.seen32(clean, std[[0, 2, 0, 2]], z32).astype(np.float64) - want)               # the stds by quantity miss the bar
    assert (wrong > bound)[:, 1:3].mean() > 0.9


def test_the_stream_overlaps_no_other(header):
    t = header["table"]
    assert t["DRAW_COMM_NOISE"] == cn.DRAW and t["COMM_NOISE_MAX_COLUMNS"] == cn.MAX_COLUMNS == 2 * capi.MAX_NEARING
    tries = 2 * t["AUTO_RESET_MAX_TRIES"]
    length = dict(DRAW_RESET_TRY=tries, DRAW_RESET_SPEED=1, DRAW_AGENT_TRY=tries, DRAW_AGENT_SPEED=1, DRAW_SCENARIO=1, DRAW_ACTOR=2, DRAW_PRIORITY=2, DRAW_SHUFFLE=1,
                  DRAW_ENTROPY=2, DRAW_PRIORITY_ENTROPY=2, DRAW_REPLAY=1, DRAW_COMM_NOISE=2 * t["COMM_NOISE_MAX_COLUMNS"])
    assert set(length) | {"DRAW_OBS_NOISE", "AUTO_RESET_MAX_TRIES", "COMM_NOISE_MAX_COLUMNS"} == set(t)
    spans = sorted((t[k], t[k] + n, k) for k, n in length.items())
    for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
        assert a1 <= b0, (ka, kb)
    assert spans[-1][1] <= t["DRAW_OBS_NOISE"]                                                     # the open-ended stream stays the highest
    assert t["DRAW_REPLAY"] < t["DRAW_COMM_NOISE"] < t["DRAW_OBS_NOISE"]
    assert (t["DRAW_ACTOR"], t["DRAW_ACTOR"] + 1) == ph.ACTOR_DRAWS and capi.PRB_DRAW == t["DRAW_REPLAY"]


# ---- the host model and its planted defects -------------------------------------------------------------------------------------------------------
def _model(defect=None, level=LEVEL, **kw):
    case = cn.model_case(**kw)
    stds = cn.column_stds(level)
    rec = cn.model_step(case["obs"], case["nearing"], case["ranks"], stds, case["seed"], case["counter"], case["env_index_base"], defect)
    ref = cn.turn_rows(rec["actions"], case["nearing"], case["ranks"], stds, case["seed"], case["counter"], case["env_index_base"])
    r = cn.compare(rec["tentative"], rec["base_obs"], case["obs"], ref, what=str(defect))
    r["no_feedback"] = bool(np.array_equal(bits(rec["actions"]), bits(cn.model_policy(rec["base_obs"]))))  # the step's actions are the actor's on the recorded rows
    return r, rec, ref, case


def test_the_host_model_passes_every_check():
    r, rec, ref, case = _model()
    print(r)
    assert r["ok"] and r["no_feedback"] and r["rows"] == 33 * 5 and r["undecided"] > 100
    assert ref["undecided"][0, 0, 2:].all()                                                        # the index that is no agent: a zero that gets its draw
    assert (rec["base_obs"][..., -4:][ref["undecided"]] != 0).all()                                # pure noise, never a clean zero
    r0, rec0, _, _ = _model(level=0.0)
    assert r0["ok"] and np.array_equal(rec0["base_obs"][..., -4:], cn.turn_rows(rec0["actions"], case["nearing"], case["ranks"], cn.column_stds(0.0), 1, 1)["clean"])


DEFECT_CASES = [("stds_by_quantity", "values"), ("one_draw_for_all_columns", "values"), ("draw_keyed_by_env_only", "values"), ("counter_ignored", "values"),
                ("noise_written_back", "no_feedback"), ("undecided_left_clean", "values"), ("actor_draw_ids", "values"), ("clean_base_record", "tentative_is_base")]


@pytest.mark.parametrize("defect,misses", DEFECT_CASES)
def test_a_planted_defect_misses_its_check(defect, misses):
    r, _, _, _ = _model(defect)
    print(r)
    assert not r[misses], (defect, r)
    assert not (r["ok"] and r["no_feedback"])


def test_every_defect_is_planted():
    assert sorted(c[0] for c in DEFECT_CASES) == sorted(cn.DEFECTS)


def test_clean_base_record_also_misses_the_values():
    r, _, _, _ = _model("clean_base_record")
    assert not r["values"]


# ---- params ----------------------------------------------------------------------------------------------------------------------------------------
def test_params_communication_noise():
    assert communication_noise(Parameters()) is None
    assert communication_noise(Parameters(is_communication_noise=True)) == 0.1
    assert communication_noise(Parameters(is_communication_noise=True, communication_noise_level=0.3)) == 0.3
    assert communication_noise(Parameters(communication_noise_level=0.3)) is None


def test_check_rollout_wrapper_with_the_noise_of_the_call():
    p = Parameters(is_using_prioritized_marl=True, is_communication_noise=True)
    check_rollout_wrapper(p, "prioritized", communication_noise(p))                                # the parameters' noise, passed: accepted (K = 2)
    check_rollout_wrapper(p, "prioritized", 0.0)
    check_rollout_wrapper(Parameters(is_using_prioritized_marl=True), "prioritized", 0.2)          # a sweep at evaluation on a policy trained without
    check_rollout_wrapper(None, "prioritized", 0.2)
    with pytest.raises(NotImplementedError, match="would ignore"):
        check_rollout_wrapper(p, "prioritized")                                                    # asked for and not passed: refused, never ignored
    with pytest.raises(NotImplementedError, match="would ignore"):
        check_rollout_wrapper(p, "prioritized", None)
    for kw in (dict(n_agents=2), dict(n_nearing_agents_observed=3), dict(n_nearing_agents_observed=1)):  # K = 1, 3, 1
        with pytest.raises(NotImplementedError, match="raises in the reference as well"):
            check_rollout_wrapper(Parameters(is_using_prioritized_marl=True, **kw), "prioritized", 0.1)
    check_rollout_wrapper(Parameters(n_agents=3), "prioritized", 0.1)                              # K = min(2, N - 1) = 2
    for w in (None, "plain", "opponent"):
        with pytest.raises(ValueError, match="prioritized"):
            check_rollout_wrapper(p, w, 0.1)
        check_rollout_wrapper(p, w)
    with pytest.raises(ValueError):
        check_rollout_wrapper(p, "cbf", 0.1)


def test_the_binding_carries_the_noise_fields():
    names = [f[0] for f in capi.RolloutOpts._fields_]
    assert names[-3:] == ["comm_noise_std", "comm_noise_std_env", "base_obs_rec"] and "reserved" not in names
    assert capi.RolloutOpts.comm_noise_std.offset == 56 and capi.RolloutOpts.comm_noise_std_env.offset == 64 and capi.RolloutOpts.base_obs_rec.offset == 72
    assert "sigmaenv_comm_noise_stds" in capi.exported_symbols()
