"""The challenging initial-state buffer's index arithmetic and decisions on the host (no GPU): sigmarl_amd/csrc/sigmaenv_isb.h compiled ALONE into a stand-alone
program (tests/host_program.py: with AddressSanitizer + UBSan where the compiler has them) against the numpy twin tests/isb_check.py -- ring slots, record decisions,
ranks, the ring and bank slots of every surviving write, ptr, count, the use decisions, j, the settled envs, and the final rings and bank agree word for word over a
sweep of (B, capacity, n_steps_stored, recorders per step, probabilities); every defect planted in the twin fails a named check; the draw ids against the table; the
entry points are bound and hashed into the build id; check_supported accepts the flag and the three refusals raise."""
import ctypes
import os
import struct
import types

import numpy as np
import pytest

import host_program
import isb_check as ic
from sigmarl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234_5678_9ABC_DEF1

PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_isb.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
static void wr(FILE* f, const std::vector<int32_t>& v) { fwrite(v.data(), 4, v.size(), f); }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  rd(in, &n_cases, 4);
  for (int c = 0; c < n_cases; ++c) {
    int32_t d[6];  // B, capacity, S, steps, env_index_base, counter0
    float p[2];    // p_record, p_use
    uint64_t seed;
    rd(in, d, sizeof d); rd(in, p, sizeof p); rd(in, &seed, 8);
    const int B = d[0], cap = d[1], S = d[2], steps = d[3], base = d[4], counter0 = d[5];
    std::vector<uint8_t> col((size_t)steps * B), done(col.size()), req(col.size());
    std::vector<int32_t> tag_step(col.size()), tag_fresh(col.size());
    rd(in, col.data(), col.size()); rd(in, done.data(), col.size()); rd(in, req.data(), col.size());
    rd(in, tag_step.data(), 4 * col.size()); rd(in, tag_fresh.data(), 4 * col.size());
    std::vector<int32_t> bank(cap, 0), ring((size_t)B * S, 0), held(B, 0), head(B, 0), epi(B, 0), episodes(B, 0), rows(B, 0), pending(B, 0);
    int ptr = 0, count = 0;
    for (int b = 0; b < B; ++b) { int h = 0, n = 0; ring[(size_t)b * S + isb_push(&h, &n, S)] = rows[b]; head[b] = h; held[b] = n; epi[b] = episodes[b]; }  // sigmaenv_isb_reset
    for (int t = 0; t < steps; ++t) {
      const size_t o = (size_t)t * B;
      const uint64_t counter = (uint64_t)counter0 + t;
      std::vector<int32_t> pushed(B), rec(B), rank(B), src(B, -1), dst(B, -1), uses(B), jj(B, -1), settled(B);
      std::vector<uint8_t> recb(B);
      for (int b = 0; b < B; ++b) {  // record: push, the decision, pending
        rows[b] = tag_step[o + b];
        pushed[b] = isb_push(&head[b], &held[b], S);
        ring[(size_t)b * S + pushed[b]] = rows[b];
        recb[b] = (uint8_t)isb_records(col[o + b] != 0, isb_word(seed, counter, (uint32_t)(base + b), DRAW_ISB_RECORD), p[0]);
        rec[b] = recb[b];
        pending[b] = !done[o + b] && req[o + b];
      }
      const int R = isb_ranks(recb.data(), B, rank.data());
      for (int b = 0; b < B; ++b) {
        if (rank[b] < 0 || !isb_rank_kept(rank[b], R, cap)) continue;
        src[b] = isb_nth_latest(head[b], held[b], S, S);
        dst[b] = isb_bank_slot(ptr, rank[b], cap);
        bank[dst[b]] = ring[(size_t)b * S + src[b]];
      }
      ptr = isb_ptr_after(ptr, R, cap);
      count = isb_count_after(count, R, cap);
      for (int b = 0; b < B; ++b) {  // restart, then the resets on the tags
        uses[b] = isb_uses(done[o + b], count, isb_word(seed, counter, (uint32_t)(base + b), DRAW_ISB_USE), p[1]);
        if (uses[b]) { jj[b] = isb_index(isb_word(seed, counter, (uint32_t)(base + b), DRAW_ISB_INDEX), count); rows[b] = bank[jj[b]]; episodes[b] += 1; }
        else if (done[o + b]) { rows[b] = tag_fresh[o + b]; episodes[b] += 1; }
        else if (req[o + b]) rows[b] = tag_fresh[o + b];
      }
      for (int b = 0; b < B; ++b) {  // settle
        settled[b] = isb_settles(episodes[b], epi[b], pending[b]);
        if (!settled[b]) continue;
        head[b] = 0; held[b] = 0;
        ring[(size_t)b * S + isb_push(&head[b], &held[b], S)] = rows[b];
        epi[b] = episodes[b]; pending[b] = 0;
      }
      wr(out, pushed); wr(out, rec); wr(out, rank); wr(out, src); wr(out, dst);
      const int32_t w[2] = {ptr, count};
      fwrite(w, 4, 2, out);
      wr(out, uses); wr(out, jj); wr(out, settled); wr(out, rows);
    }
    wr(out, bank); wr(out, ring); wr(out, held); wr(out, head);
  }
  fclose(in); fclose(out);
  printf("ok %%d cases, chunk %%d, draws %%u %%u %%u\n", (int)n_cases, (int)ISB_CHUNK, (unsigned)DRAW_ISB_RECORD, (unsigned)DRAW_ISB_USE, (unsigned)DRAW_ISB_INDEX);
  return 0;
}
"""


def sweep():
    """(name, script, p_record, p_use, env_index_base, counter0): capacities 1, 3, 100; n_steps_stored 1, 3, 10; R = 0, 1, capacity, capacity + 1, 2 capacity + 1
    recorders in one step with ptr wrapping across steps; B = 1, 5, 70 and past a chunk of the record workgroup; probabilities 0, 1 and in between."""
    cs = []
    k = 0
    for B in (1, 5, 70):
        for cap in (1, 3):
            for S in (1, 3):
                rec = [0, 1, cap, cap + 1, 2 * cap + 1, 1, cap]
                for p_record, p_use in ((1.0, 1.0), (0.5, 0.5), (1.0, 0.2)):
                    cs.append((f"B{B}_c{cap}_s{S}_p{p_record}_{p_use}", ic.make_script(B, cap, S, 9, rec, 100 + k), p_record, p_use, 0, 3 * k))
                    k += 1
    cs.append(("defaults", ic.make_script(300, 100, 10, 14, [None], 7), 1.0, 0.2, 0, 0))
    cs.append(("never", ic.make_script(40, 3, 3, 6, [None], 8), 0.0, 0.0, 0, 5))
    cs.append(("sharded", ic.make_script(33, 3, 3, 6, [None], 9), 0.5, 0.5, 4096, (1 << 32) - 2))  # env_index_base, and a counter across 2^32
    cs.append(("past_a_chunk", ic.make_script(ic.CHUNK + 7, 3, 3, 3, [None], 10), 1.0, 0.5, 0, 1))
    return cs


KEYS = ("pushed", "records", "rank", "src", "dst", "ptr", "count", "uses", "j", "settled", "rows")


@pytest.fixture(scope="module")
def header_results(tmp_path_factory):
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("isb_header")
    cs = sweep()
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for _, sc, p_record, p_use, base, counter0 in cs:
            f.write(struct.pack("<6i", sc["B"], sc["capacity"], sc["S"], sc["steps"], base, counter0 - (1 << 32) if counter0 >= 1 << 31 else counter0))
            f.write(struct.pack("<2f", p_record, p_use))
            f.write(struct.pack("<Q", SEED))
            for k, dt in (("collided", np.uint8), ("done", np.uint8), ("request", np.uint8), ("tag_step", np.int32), ("tag_fresh", np.int32)):
                f.write(np.ascontiguousarray(sc[k], dt).tobytes())
    stdout = host_program.build_and_run(tmp, "isb_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {len(cs)} cases, chunk {ic.CHUNK}, draws {ic.DRAW_RECORD} {ic.DRAW_USE} {ic.DRAW_INDEX}" in stdout
    raw = np.fromfile(tmp / "out.bin", np.int32)
    res, at = {}, 0
    for name, sc, *_ in cs:
        B, steps, cap, S = sc["B"], sc["steps"], sc["capacity"], sc["S"]
        r = {k: [] for k in KEYS}
        for _ in range(steps):
            for k in KEYS:
                n = 1 if k in ("ptr", "count") else B
                r[k].append(raw[at] if n == 1 and k in ("ptr", "count") else raw[at: at + n])
                at += n
        r = {k: np.asarray(v, np.int32) for k, v in r.items()}
        for k, n, shape in (("bank", cap, (cap,)), ("ring", B * S, (B, S)), ("held", B, (B,)), ("head", B, (B,))):
            r[k] = raw[at: at + n].reshape(shape)
            at += n
        res[name] = r
    assert at == raw.size
    return res


def twin_of(case, defect=None):
    _, sc, p_record, p_use, base, counter0 = case
    return ic.run_script(sc, p_record, p_use, SEED, counter0, base, defect)


def test_the_header_agrees_with_the_twin_word_for_word(header_results):
    seen = dict(records=0, dropped=0, uses=0, settled=0, wrapped=0, slot0=0)
    for case in sweep():
        got, want = header_results[case[0]], twin_of(case)
        for k in KEYS + ("bank", "ring", "held", "head"):
            assert np.array_equal(got[k], want[k]), (case[0], k)
        seen["records"] += int(want["records"].sum())
        seen["dropped"] += int(((want["rank"] >= 0) & (want["dst"] < 0)).sum())
        seen["uses"] += int(want["uses"].sum())
        seen["settled"] += int(want["settled"].sum())
        seen["wrapped"] += int((np.diff(want["ptr"]) < 0).sum())
        seen["slot0"] += int(((want["src"] == 0) & (case[1]["S"] > 1)).sum())
    assert all(v > 0 for v in seen.values()), seen  # the sweep reaches every branch: recorders, overwritten ranks, restarts, settles, a wrapping ptr, a short ring


def differs(case, defect, keys):
    a, b = twin_of(case), twin_of(case, defect)
    return [k for k in keys if not np.array_equal(a[k], b[k])]


CASES = {c[0]: c for c in sweep()}


def test_planted_defect_ranks_in_descending_b():
    assert "rank" in differs(CASES["B70_c3_s3_p1.0_1.0"], "ranks_descending", ("rank", "dst", "bank"))


def test_planted_defect_the_first_capacity_recorders_kept():
    d = differs(CASES["B70_c3_s3_p1.0_1.0"], "keep_first", ("rank", "dst", "bank", "ptr", "count"))
    assert "dst" in d and "rank" not in d and "ptr" not in d and "count" not in d  # (the slots written: the final bank may agree again once later steps overwrite it)


def test_planted_defect_nth_latest_returns_the_newest():
    d = differs(CASES["B70_c3_s3_p1.0_1.0"], "nth_newest", ("src", "bank", "dst"))
    assert "src" in d and "bank" in d and "dst" not in d
    assert not differs(CASES["B70_c3_s1_p1.0_1.0"], "nth_newest", ("src", "bank"))  # (a ring of one entry: the oldest IS the newest)


def test_planted_defect_j_modulo_capacity():
    d = differs(CASES["B70_c3_s3_p1.0_1.0"], "index_mod_capacity", ("j", "uses"))  # (step 1 holds one entry of three: every finished env must draw j = 0)
    assert "j" in d and "uses" not in d


def test_planted_defect_use_decided_before_the_recordings_count():
    d = differs(CASES["B5_c3_s3_p1.0_1.0"], "use_before_count", ("uses", "j"))
    assert "uses" in d  # (the first recording and the first finished env fall into one step: an empty bank before, one entry after)


def test_planted_defect_settle_skips_pending_envs():
    d = differs(CASES["B70_c3_s3_p1.0_1.0"], "settle_skips_pending", ("settled", "held", "ring"))
    assert "settled" in d


def test_planted_defect_collision_state_pushed_after_the_read():
    d = differs(CASES["B70_c3_s1_p1.0_1.0"], "push_after_read", ("bank", "src"))
    assert "bank" in d and "src" not in d  # (n_steps_stored = 1: the entry must be the collision state itself, not the step before it)
    assert "bank" in differs(CASES["B70_c3_s3_p1.0_1.0"], "push_after_read", ("bank",))


def test_the_draw_ids_and_the_chunk_match_the_table():
    hdr = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_dist.h")).read()
    for name, v in (("DRAW_ISB_RECORD", ic.DRAW_RECORD), ("DRAW_ISB_USE", ic.DRAW_USE), ("DRAW_ISB_INDEX", ic.DRAW_INDEX)):
        assert f"#define {name} {v}u" in hdr
    assert (capi.ISB_DRAW_RECORD, capi.ISB_DRAW_USE, capi.ISB_DRAW_INDEX) == (ic.DRAW_RECORD, ic.DRAW_USE, ic.DRAW_INDEX)
    assert 5000 < ic.DRAW_RECORD < ic.DRAW_USE < ic.DRAW_INDEX < 7000  # between DRAW_SCENARIO and DRAW_ACTOR
    isb = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv_isb.h")).read()
    assert f"#define ISB_CHUNK {ic.CHUNK} " in isb and capi.ISB_CHUNK == ic.CHUNK
    assert "#include <hip" not in isb and isb.count("#include") == 2 and "<stdint.h>" in isb and '"sigmaenv_dist.h"' in isb  # plain C++: <stdint.h> and sigmaenv_dist.h
    pub = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    assert f"#define SIGMAENV_ISB_CHUNK {ic.CHUNK} " in pub
    for k, name in enumerate(("BANK_STATE", "BANK_PATH", "WORDS", "RING_STATE", "RING_PATH", "HELD", "HEAD", "PENDING")):
        assert f"#define SIGMAENV_ISB_{name} {k} " in pub and getattr(capi, "ISB_" + name) == k


ENTRY_POINTS = ("isb_create", "isb_destroy", "isb_reset", "isb_record", "isb_restart", "isb_settle", "isb_attach", "isb_get", "isb_set")


def test_the_entry_points_are_bound_and_hashed_into_the_build_id():
    header = open(os.path.join(ROOT, "include", "sigmaenv.h")).read()
    for name in ENTRY_POINTS:
        assert "sigmaenv_" + name in capi.exported_symbols() and name in capi._PRODUCT_ONLY and f" sigmaenv_{name}(" in header, name
    assert "never consult a bank" in header
    mk = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "Makefile")).read()
    src = [ln for ln in mk.splitlines() if ln.startswith("SRC = ")][0].split()
    assert "sigmaenv_isb.h" in src and "sigmaenv_isb.inc" in src
    hip = open(os.path.join(ROOT, "sigmarl_amd", "csrc", "sigmaenv.hip")).read()
    assert '#include "sigmaenv_isb.h"' in hip and '#include "sigmaenv_isb.inc"' in hip
    if os.path.exists(capi.DEFAULT_LIB):
        lib = ctypes.CDLL(capi.DEFAULT_LIB)
        assert all(hasattr(lib, "sigmaenv_" + name) for name in ENTRY_POINTS)


def test_check_supported_accepts_the_flag_and_the_three_refusals_raise():
    from sigmarl_amd import evaluate as E
    from sigmarl_amd import learn
    from sigmarl_amd.actor import Actor
    from sigmarl_amd.params import Parameters, check_initial_state_bank, check_supported
    from sigmarl_amd.scenario import ScenarioRoadTraffic

    p = Parameters(is_apply_mask=False, is_challenging_initial_state_buffer=True)
    check_supported(p)
    check_initial_state_bank(p, True)
    check_initial_state_bank(Parameters(is_apply_mask=False), False)
    check_initial_state_bank(None, False)
    with pytest.raises(NotImplementedError, match="InitialStateBank"):
        check_initial_state_bank(p, False)
    env = types.SimpleNamespace(B=4, N=4, K=2, D=32, parameters=p)  # (no bank attached: refused before any device call)
    with pytest.raises(NotImplementedError, match="InitialStateBank"):
        Actor.rollout(object.__new__(Actor), env, 4)
    with pytest.raises(NotImplementedError, match="InitialStateBank"):
        learn.collect(env, None, None, 4, gamma=0.99, lmbda=0.9)
    sc = ScenarioRoadTraffic.__new__(ScenarioRoadTraffic)
    sc.parameters = p
    with pytest.raises(NotImplementedError, match="InitialStateBank"):
        sc.make_world(4, "cpu")
    assert E.evaluation_parameters(p).is_challenging_initial_state_buffer is False  # evaluation keeps switching it off


def test_the_recording_run_on_the_oracle():
    """The seed of tests/test_gpu_isb.py's recording run, as it was picked: on the CPU, the oracle stepping and the twin deciding.  Seeds 1 .. 5 give (recorded,
    restarted) = (51, 88), (382, 404), (199, 237), (349, 374), (195, 230); seed 1 stays below the bank's capacity, so its count is the number of recordings."""
    recorded, restarted = ic.recording_run_on_the_oracle()
    assert (recorded, restarted) == (51, 88) and recorded < ic.RECORDING_RUN["capacity"] and recorded >= 8 and restarted >= 2
