"""The generator, its draw table and the TanhNormal head on the host (no GPU): sigmarl_amd/csrc/sigmaenv_dist.h compiled ALONE into a stand-alone program
(tests/host_program.py: with AddressSanitizer + UBSan where the compiler has them) against tests/policy_head_check.py -- rng_u32, the two uniforms and the bounded
draw equal the Python restatement bit for bit; the normal pair, the cosine-only normal and the whole head, composed as actor_distribution and the priority head
compose them, pass ``policy_head_check.compare`` in the device's place (the host's libm is not the device's: held by the criterion, not by bits; saturated rows
exactly); and the table the program prints equals every Python mirror of it.

Head rows: 257 x 16, random loc / raw ~ N(0, 1.5), and planted: rows 0 .. 63 loc = +-12 at raw = -40 (|x| >= 10: saturated), rows 64 .. 127 raw = -40 (the scale on
its floor), rows 128 .. 159 raw = +25 (softplus takes its v > 20 branch).  softplus >= 0, so of biased_softplus's two floors only the 0.01 one acts on finite input
(the scale is 0.01 to rounding); the 1e-4 one is the same fmaxf and is never reached."""
import struct

import numpy as np
import pytest

import host_program
import observation_check
import policy_head_check as ph
import ppo_head_check
import prb_check
from sigmarl_amd import capi

f32 = np.float32
SEED, COUNTERS = (0xABCD1234 << 32) | 77, (5, 2 ** 32 + 5)  # a seed with its high word set; the two counters draw the same words
ENVS, AGENTS = (0, 1, 100000, 2 ** 32 - 1), (0, 3)
MAX_TRIES = 64
# every id of the table, from the Python mirrors (test_the_table_equals_every_python_mirror holds the two equal): the try ranges, the single draws, 9000 + k
DRAW_IDS = np.concatenate([np.arange(2 * MAX_TRIES), [1000], 2000 + np.arange(2 * MAX_TRIES), [3000, 5000], ph.ACTOR_DRAWS, ph.PRIORITY_DRAWS, [ph.SHUFFLE_DRAW],
                           ppo_head_check.ENTROPY_DRAWS, [prb_check.DRAW], observation_check.NOISE_DRAW + np.arange(4096)]).astype(np.uint32)
WORDS = np.concatenate([np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF], np.uint32),
                        np.random.default_rng(3).integers(0, 2 ** 32, 65536, dtype=np.uint64).astype(np.uint32)])
BOUNDS = (1, 2, 3, 16, 65535)
B, N = 257, 16
HEAD_SEED, HEAD_COUNTER, ENV_BASE = 0x1234567890ABCDEF, 77, 4096
LOW, HIGH = np.array([-1.0, -0.6], f32), np.array([1.0, 0.6], f32)
TABLE = ("AUTO_RESET_MAX_TRIES", "DRAW_RESET_TRY", "DRAW_RESET_SPEED", "DRAW_AGENT_TRY", "DRAW_AGENT_SPEED", "DRAW_SCENARIO", "DRAW_ACTOR", "DRAW_PRIORITY",
         "DRAW_SHUFFLE", "DRAW_ENTROPY", "DRAW_REPLAY", "DRAW_OBS_NOISE")


def generator_keys():
    """(counter u64, env u32, agent u32, draw u32), the full cross"""
    c, e, a, d = np.meshgrid(np.array(COUNTERS, np.uint64), np.array(ENVS, np.uint32), np.array(AGENTS, np.uint32), DRAW_IDS, indexing="ij")
    return c.reshape(-1), e.reshape(-1), a.reshape(-1), d.reshape(-1)


def head_rows():
    g = np.random.default_rng(9)
    loc, raw = (g.standard_normal((B * N, 2)) * 1.5).astype(f32), (g.standard_normal((B * N, 2)) * 1.5).astype(f32)
    loc[:64] = np.where(g.random((64, 2)) < 0.5, -12.0, 12.0)
    raw[:128] = -40.0
    raw[128:160] = 25.0
    return loc, raw


PROGRAM = r"""
#define SIGMA_HD static inline
#include "sigmaenv_dist.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
template <class T> static void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }

int main() {
  FILE* in = fopen("%(inp)s", "rb");
  FILE* out = fopen("%(out)s", "wb");
  if (!in || !out) return 3;
#define ROW(name) printf("table " #name " %%u\n", (unsigned)(name))
  ROW(AUTO_RESET_MAX_TRIES); ROW(DRAW_RESET_TRY); ROW(DRAW_RESET_SPEED); ROW(DRAW_AGENT_TRY); ROW(DRAW_AGENT_SPEED); ROW(DRAW_SCENARIO); ROW(DRAW_ACTOR);
  ROW(DRAW_PRIORITY); ROW(DRAW_SHUFFLE); ROW(DRAW_ENTROPY); ROW(DRAW_REPLAY); ROW(DRAW_OBS_NOISE);
  // the generator
  int32_t K = 0;
  uint64_t seed = 0;
  rd(in, &K, 4); rd(in, &seed, 8);
  std::vector<uint64_t> counter((size_t)K);
  std::vector<uint32_t> env((size_t)K), agent((size_t)K), draw((size_t)K), word((size_t)K);
  rd(in, counter.data(), 8 * (size_t)K); rd(in, env.data(), 4 * (size_t)K); rd(in, agent.data(), 4 * (size_t)K); rd(in, draw.data(), 4 * (size_t)K);
  for (int k = 0; k < K; ++k) word[k] = rng_u32(seed, counter[k], env[k], agent[k], draw[k]);
  wr(out, word);
  // a word -> a number
  int32_t W = 0, NB = 0;
  rd(in, &W, 4); rd(in, &NB, 4);
  std::vector<uint32_t> w((size_t)W), bound((size_t)NB), below((size_t)W);
  std::vector<float> u((size_t)W), um((size_t)W);
  rd(in, w.data(), 4 * (size_t)W); rd(in, bound.data(), 4 * (size_t)NB);
  for (int k = 0; k < W; ++k) { u[k] = rng_uniform(w[k]); um[k] = rng_uniform_mid(w[k]); }
  wr(out, u); wr(out, um);
  for (int b = 0; b < NB; ++b) {
    for (int k = 0; k < W; ++k) below[k] = rng_below(w[k], bound[b]);
    wr(out, below);
  }
  // the head: two dimensions between bounds as actor_distribution composes it, then one dimension as the priority head does
  int32_t R = 0, n_agents = 0, env_base = 0;
  uint64_t hs = 0, hc = 0;
  float low[2], high[2];
  rd(in, &R, 4); rd(in, &n_agents, 4); rd(in, &env_base, 4); rd(in, &hs, 8); rd(in, &hc, 8); rd(in, low, 8); rd(in, high, 8);
  std::vector<float> loc(2 * (size_t)R), raw(2 * (size_t)R), action(2 * (size_t)R), scale(2 * (size_t)R), slope(2 * (size_t)R), lp((size_t)R), score((size_t)R), lp1((size_t)R);
  rd(in, loc.data(), 8 * (size_t)R); rd(in, raw.data(), 8 * (size_t)R);
  for (int r = 0; r < R; ++r) {
    const uint32_t e = (uint32_t)(env_base + r / n_agents), a = (uint32_t)(r %% n_agents);
    float z[2], ld[2];
    rng_normal_pair(hs, hc, e, a, DRAW_ACTOR, &z[0], &z[1]);
    for (int d = 0; d < 2; ++d) {
      const float sc = tn_scale(raw[2 * r + d]), x = loc[2 * r + d] + sc * z[d], h = 0.5f * (high[d] - low[d]);
      scale[2 * r + d] = sc;
      slope[2 * r + d] = tn_scale_slope(raw[2 * r + d], tn_raw_scale(raw[2 * r + d]));
      action[2 * r + d] = tn_affine(low[d], tn_squash(x), h);
      ld[d] = tn_log_density(z[d], logf(sc), x) - logf(h);
    }
    lp[r] = ld[0] + ld[1];
    const float sc = tn_scale(raw[2 * r]), z1 = rng_normal_cos(hs, hc, e, a, DRAW_PRIORITY), x = loc[2 * r] + sc * z1;
    score[r] = tn_squash(x);
    lp1[r] = tn_log_density(z1, logf(sc), x);
  }
  wr(out, action); wr(out, scale); wr(out, slope); wr(out, lp); wr(out, score); wr(out, lp1);
  fclose(in); fclose(out);
  printf("ok %%d keys %%d words %%d rows\n", (int)K, (int)W, (int)R);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """everything through the header compiled alone, once"""
    if host_program.compiler() is None:
        pytest.fail("no host C++ compiler: the header cannot be compiled alone")
    tmp = tmp_path_factory.mktemp("dist_header")
    c, e, a, d = generator_keys()
    loc, raw = head_rows()
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<iQ", c.size, SEED))
        for v in (c, e, a, d):
            f.write(np.ascontiguousarray(v).tobytes())
        f.write(struct.pack("<ii", WORDS.size, len(BOUNDS)))
        f.write(WORDS.tobytes())
        f.write(np.array(BOUNDS, np.uint32).tobytes())
        f.write(struct.pack("<iiiQQ", B * N, N, ENV_BASE, HEAD_SEED, HEAD_COUNTER))
        f.write(LOW.tobytes() + HIGH.tobytes() + loc.tobytes() + raw.tobytes())
    stdout = host_program.build_and_run(tmp, "dist_header", PROGRAM % dict(inp=str(tmp / "in.bin"), out=str(tmp / "out.bin")))
    assert f"ok {c.size} keys {WORDS.size} words {B * N} rows" in stdout
    rawout = np.fromfile(tmp / "out.bin", np.uint32)
    at, res = 0, {}

    def take(name, n, dtype=np.uint32, shape=None):
        nonlocal at
        res[name] = rawout[at:at + n].view(dtype).reshape(shape or (n,))
        at += n

    take("word", c.size)
    for k in ("uniform", "uniform_mid"):
        take(k, WORDS.size, f32)
    for n in BOUNDS:
        take(("below", n), WORDS.size)
    R = B * N
    for k in ("action", "scale", "slope"):
        take(k, 2 * R, f32, (R, 2))
    for k in ("log_prob", "score", "log_prob_1d"):
        take(k, R, f32)
    assert at == rawout.size
    res["table"] = {p[1]: int(p[2]) for p in (line.split() for line in stdout.splitlines()) if len(p) == 3 and p[0] == "table"}
    return res


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_rng_u32_equals_the_python_generator_on_every_id_of_the_table(header):
    c, e, a, d = generator_keys()
    got = header["word"]
    assert np.array_equal(got, ph.rng_u32(SEED, c, e, a, d))
    per = got.reshape(len(COUNTERS), -1)
    assert np.array_equal(per[0], per[1])                                                      # counter 5 and 2^32 + 5: the low word only
    assert not np.array_equal(per[0], ph.rng_u32(SEED & 0xFFFFFFFF, c, e, a, d).reshape(len(COUNTERS), -1)[0])  # the seed's high word enters


def test_the_uniforms_and_the_bounded_draw_equal_numpy_bit_for_bit(header):
    k = WORDS >> np.uint32(8)
    half_open = k.astype(f32) * f32(1.0 / 16777216.0)
    assert np.array_equal(bits(header["uniform"]), bits(half_open))
    assert np.array_equal(bits(header["uniform_mid"]), bits(ph.uniform(WORDS)))
    assert header["uniform_mid"][WORDS == 0xFFFFFFFF][0] == f32(1.0) and header["uniform_mid"].max() == f32(1.0) and header["uniform_mid"].min() == f32(2.0 ** -25)
    assert header["uniform"].max() < f32(1.0) and header["uniform"][WORDS == 0xFFFFFFFF][0] == f32(1.0 - 2.0 ** -24) and header["uniform"].min() == 0.0
    for n in BOUNDS:
        want = [(int(w) * n) >> 32 for w in WORDS.tolist()]
        assert np.array_equal(header[("below", n)], np.array(want, np.uint32)), n
        assert header[("below", n)].max() == n - 1


def _draws(draw_ids):
    env, agent = ph.row_keys(B, N, ENV_BASE)
    z = [np.stack(ph.normals(HEAD_SEED, HEAD_COUNTER, env, agent, draw_ids, **kw), -1) for kw in (dict(), dict(dtype=np.float32), dict(magnitude=True))]
    return z  # float64, the float32 twin's, the magnitudes


def test_the_head_between_bounds_passes_the_criterion_in_the_devices_place(header):
    """rng_normal_pair + the head in two dimensions, as actor_distribution composes them; compared at the header's own float32 scale, as the actor's cases are"""
    loc, raw = head_rows()
    z, z32, zmag = _draws(ph.ACTOR_DRAWS)
    r, ref = ph.compare(header["action"], header["log_prob"], loc, header["scale"], z, LOW, HIGH, z32=z32, zmag=zmag, what="header, between bounds")
    print(r)
    assert r["rows"] == B * N >= ph.FULL_ROWS and r["ok"], r
    assert r["saturated"] >= 128 and r["saturated_wrong"] == 0                                 # rows 0 .. 63, both dimensions, held with ==
    sc = ph.compare_scale(header["scale"], raw.astype(np.float64), 0.0)
    print(sc)
    assert sc["ok"], sc
    assert np.all(header["scale"][:128] == f32(0.01)) and np.all(header["scale"][128:160] == (f32(25.0) + f32(ph.BIAS)) + f32(0.01))  # the floor; the v > 20 branch
    n = ph.regime_counts(ref["x"], header["scale"], z)
    print(n)
    assert min(n["tanh_is_one"], n["shortcut_jacobian"], n["shortcut_scale"], n["scale_floor"], n["inside"]) > 0


def test_the_one_dimensional_head_passes_the_criterion_in_the_devices_place(header):
    """rng_normal_cos + the head without the affine map, as sigmaenv_priority_head_kernel composes them; the reference forms scale_of(raw) in float64"""
    loc, raw = head_rows()
    z, z32, zmag = (v[:, :1] for v in _draws(ph.PRIORITY_DRAWS))
    r, ref = ph.compare(header["score"][:, None], header["log_prob_1d"], loc[:, :1], None, z, None, None, z32=z32, zmag=zmag, raw=raw[:, :1], what="header, 1-D")
    print(r)
    assert r["rows"] == B * N and r["ok"], r
    assert r["saturated"] >= 64 and r["saturated_wrong"] == 0


def test_the_scale_slope_is_the_sigmoid(header):
    """d scale / d raw = 1 / (1 + exp(-w)), w = raw + bias, against float64.  d ln slope / d w = 1 - slope <= 1, so the float32 rounding of w moves the slope by at
    most |w| 2^-24 relative and the float32 bias's own rounding by under 2^-24; expf (under 1 ulp in a libm), the sum and the correctly rounded quotient add
    2^-23 + 2^-24 + 2^-24: in all under (|w| / 2 + 2.5) 2^-23."""
    _, raw = head_rows()
    w = raw.astype(np.float64) + ph.BIAS
    want = 1.0 / (1.0 + np.exp(-w))
    assert np.all(np.abs(header["slope"] - want) <= (np.abs(w) / 2 + 2.5) * 2.0 ** -23 * want)
    assert header["slope"][:128].max() < 1e-16 and header["slope"][128:160].min() == f32(1.0)


def test_the_table_equals_every_python_mirror(header):
    t = header["table"]
    assert set(t) == set(TABLE)
    assert (t["DRAW_ACTOR"], t["DRAW_ACTOR"] + 1) == ph.ACTOR_DRAWS and (t["DRAW_PRIORITY"], t["DRAW_PRIORITY"] + 1) == ph.PRIORITY_DRAWS
    assert t["DRAW_SHUFFLE"] == ph.SHUFFLE_DRAW and (t["DRAW_ENTROPY"], t["DRAW_ENTROPY"] + 1) == ppo_head_check.ENTROPY_DRAWS
    assert t["DRAW_REPLAY"] == prb_check.DRAW == capi.PRB_DRAW and t["DRAW_OBS_NOISE"] == observation_check.NOISE_DRAW
    # no id changes: the values the oracle's twin and the recorded golden runs were made with
    assert [t[k] for k in TABLE] == [64, 0, 1000, 2000, 3000, 5000, 7000, 7100, 7200, 7300, 7400, 9000]
    assert t["AUTO_RESET_MAX_TRIES"] == MAX_TRIES
    ids = DRAW_IDS.tolist()
    assert len(set(ids)) == len(ids) and max(ids[:-4096]) < t["DRAW_OBS_NOISE"]               # the streams are disjoint, the open-ended one the highest
