"""The restart of a finished env from registers (auto_reset_tile's accept loop, place_from_start_table's row head) at every lane layout of the sampler.

A finished env's 64 lanes hold TR = 64 / N precomputed tries per agent; the accept loop keeps the feasibility of all of them in one wavefront-uniform word, lane i
notes the LANE whose try agent i accepted and fetches (path, point) from it after the loop; an agent without a feasible try among its first TR evaluates tries
TR .. 63 on all lanes against the accepted positions of the agents before it, read from the lanes' registers.  A reset before the last step of a T-step launch
loads only the head of the start table's row.  Every case here forces one tile shape (asserted with ``launch_shape()``) and drives

  (a) the stand-alone ``auto_reset`` (the workgroup kernel; every env at once, and again after separate ``step`` launches later),
  (b) one ``step_autoreset_n`` chunk of 8 steps against 8 single ``step_autoreset`` launches on a second handle: every buffer and the record byte for byte, and
      both against the C oracle (test_gpu_parity._compare_all: integers bit-exact),
  (c) in testing mode on an entry / exit map, the per-agent requests (``while (rq)``).

What keeps a case from showing nothing is asserted on the ORACLE's buffers, and therefore without a GPU too (test_case_meets_its_conditions_on_the_oracle): an env
restarted before the last step of the chunk and another in its last step; a 4 x 4 tile had finished and unfinished envs in one step; and in the 32-agent case on
on_ramp_1 (injected start) some agent accepted a try beyond its first TR and some agent had no feasible try at all -- found by replaying the sampler's draws
(policy_head_check.rng_u32, held to the oracle's path rows) and seen on the oracle's state as a pair closer than the minimum start distance right after a restart.
The seeds were picked on the oracle alone."""
from collections import namedtuple

import numpy as np
import pytest

import oracle_binding as ob
import policy_head_check as phc
import test_gpu_parity as tp
import test_gpu_tiles as tt
from sigmarl_amd import capi
from sigmarl_amd.maps import injected_start, load_map
from sigmarl_amd.params import Parameters, make_config

gpu = pytest.mark.gpu

T_CHUNK = 8
MAX_TRIES = 64
Case = namedtuple("Case", "name scen N G B fixed testing injected seed")

CASES = [
    Case("fixed_16x1", "cpm_entire", 16, 1, 7, True, False, False, 1),                 # TR = 4
    Case("fixed_32x1_on_ramp_injected", "on_ramp_1", 32, 1, 5, True, False, True, 2),  # TR = 2: tries beyond TR, agents without a feasible try
    Case("fixed_4x4", "cpm_entire", 4, 4, 39, True, False, False, 3),                  # TR = 16: tiles with finished and unfinished envs
    Case("generic_3x5", "cpm_entire", 3, 5, 23, False, False, False, 4),               # TR = 21: lane 63 idle
    Case("21x3", "cpm_entire", 21, 3, 8, False, False, False, 5),                      # TR = 3
    Case("1x16_single_agent", "cpm_entire", 1, 16, 37, False, False, False, 6),        # TR = 64: every lane a try of the one agent
    Case("fixed_8x2_on_ramp_testing", "on_ramp_1", 8, 2, 21, True, True, False, 14),   # TR = 8: per-agent requests at three steps of the chunk
]


def _config(c):
    kw = dict(n_agents=c.N, scenario_type=c.scen, is_use_mtv_distance=False, rew_method="distance", dt=0.05, is_apply_mask=False, is_obs_noise=False, max_steps=5,
              is_testing_mode=c.testing)
    mp = load_map(c.scen)
    start = None
    if c.injected:
        idx, st = injected_start(mp, c.N)
        kw.update(predefined_ref_path_idx=idx, init_state=st)
        start = (idx, st)
    return make_config(Parameters(**kw), mp, c.B), mp, start


def _min_d_sq(cfg):
    """(sqrtf((float)(length^2 + width^2)) * 1.5f)^2, the operations of derive_config."""
    min_d = np.sqrt(np.float32(float(cfg.length) * float(cfg.length) + float(cfg.width) * float(cfg.width))) * np.float32(1.5)
    return np.float32(min_d * min_d)


def replay_restart(cfg, mp, pf, pc, seed, counter, b):
    """The full-env sampler of env b, restated from its specification (sigmaenv_dist.h's draw table; first feasible try, else try 63): per agent
    (try, feasible, path, point), and the accepted positions."""
    N, testing = cfg.n_agents, bool(cfg.is_testing_mode)
    env = cfg.env_index_base + b
    min_d_sq = _min_d_sq(cfg)
    X, Y, out = np.zeros(N, np.float32), np.zeros(N, np.float32), []
    t_all = np.arange(MAX_TRIES)
    for i in range(N):
        k_path = phc.rng_u32(seed, counter, env, i, 2 * t_all).astype(np.uint64)
        k_pt = phc.rng_u32(seed, counter, env, i, 2 * t_all + 1).astype(np.uint64)
        for t in range(MAX_TRIES):
            path = pf + int((k_path[t] * np.uint64(pc)) >> np.uint64(32))
            half = int(mp.n_center[path]) // 2
            end = min(3 + (t + 1) * (t + 2) // 2, half) if testing else half
            end = max(end, 4)
            pt = 3 + int((k_pt[t] * np.uint64(end - 3)) >> np.uint64(32))
            px, py = np.float32(mp.center[path, pt, 0]), np.float32(mp.center[path, pt, 1])
            dx, dy = px - X[:i], py - Y[:i]
            d2 = dx * dx + dy * dy
            ok = bool(np.all(d2 >= min_d_sq))
            if ok:
                break
        X[i], Y[i] = px, py
        out.append((t, ok, path, pt))
    return out, X, Y


class _Run:
    """One case: the oracle and the HIP handles (the chunk's handle first, the single launches' second; none without a GPU)."""

    def __init__(self, c, devs):
        self.c, self.devs = c, devs
        self.cfg, self.mp, self.start = _config(c)
        self.ora = ob.OracleEnv(self.cfg, self.mp)
        self.B, self.N, self.G, self.D = c.B, c.N, c.G, self.ora.D
        self.W = self.N * (self.D + 1) + 1
        self.pf, self.pc = int(self.mp.list_first[0]), int(self.mp.list_count[0])
        self.min_d_sq = _min_d_sq(self.cfg)

    def actions(self, rng, t):
        B, N = self.B, self.N
        if t % 3 == 1:
            act = np.stack([rng.uniform(0.1, 0.4, (B, N)), rng.uniform(-0.03, 0.03, (B, N))], axis=-1)
        else:
            act = np.stack([rng.uniform(-0.5, 1.6, (B, N)), rng.uniform(-0.9, 0.9, (B, N))], axis=-1)
        return act.astype(np.float32)

    def check(self, tag):
        tag = f"{self.c.name}: {tag}"
        for d in self.devs:
            try:
                tp._compare_all(d, self.ora, tag)
            except AssertionError as e:
                raise AssertionError(f"{e}; {tt._locate_oracle_mismatch(d, self.ora, self.N, self.G)}") from None
        if len(self.devs) == 2:
            for which in tt.ALL_BUFS:
                tt._assert_same_bits(tag, f"buffer {which}", self.devs[0].get(which), self.devs[1].get(which), self.N, self.G, which)

    def ora_step(self, act, counter, stats):
        """One oracle step and its resets; the conditions are read between the two."""
        B, N, G = self.B, self.N, self.G
        self.ora.step(act)
        done = self.ora.get(capi.BUF_DONE).astype(bool)
        req = self.ora.get(capi.BUF_COL_FLAGS)[..., 3].astype(bool) & ~done[:, None]
        rec = (self.ora.get(capi.BUF_OBS).copy(), self.ora.get(capi.BUF_REWARD).copy(), done)
        stats["done"].append(int(done.sum()))
        stats["req"].append(int(req.sum()))
        stats["mixed"] += sum(int(0 < done[k:k + G].sum() < len(done[k:k + G])) for k in range(0, B, G))
        self.ora.auto_reset(self.c.seed, counter, self.pf, self.pc)
        if self.c.injected:  # which try every agent of a restarted env accepted
            path, st = self.ora.get(capi.BUF_PATH), self.ora.get(capi.BUF_STATE)
            for b in np.flatnonzero(done):
                tries, X, Y = replay_restart(self.cfg, self.mp, self.pf, self.pc, self.c.seed, counter, int(b))
                assert [(p, q) for _, _, p, q in tries] == [(int(path[b, i, 0]), int(path[b, i, 3])) for i in range(N)], "the replay of the sampler left the oracle"
                assert np.array_equal(X, st[b, :, 0]) and np.array_equal(Y, st[b, :, 1])
                tr = MAX_TRIES // N
                stats["beyond_tr"] += sum(1 for t, ok, _, _ in tries if ok and t >= tr)
                stats["infeasible"] += sum(1 for _, ok, _, _ in tries if not ok)
                dx, dy = X[:, None] - X[None, :], Y[:, None] - Y[None, :]
                d2 = dx * dx + dy * dy
                stats["close_pairs"] += int(((d2 < self.min_d_sq) & ~np.eye(N, dtype=bool)).sum()) // 2
        return rec

    def run(self):
        c, B, N = self.c, self.B, self.N
        torch = None
        if self.devs:
            import torch
        # ---- the start: the stand-alone auto_reset of every env, or the injected start ----------------------------------------------------------------------------
        if self.start:
            idx, st = self.start
            ids = np.zeros((B, N, 4), np.int32)
            ids[..., 0] = np.asarray([self.mp.global_path(0, q) for q in idx], np.int32)[None, :]
            ids[..., 2] = np.asarray(idx, np.int32)[None, :]
            st8 = np.zeros((B, N, 8), np.float32)
            st8[..., 0:3] = np.asarray(st, np.float32)[None, :, :]
            ei, ai = np.repeat(np.arange(B, dtype=np.int32), N), np.tile(np.arange(N, dtype=np.int32), B)
            for e in self.devs + [self.ora]:
                e.reset(ei, ai, ids.reshape(-1, 4), st8.reshape(-1, 8), 1)
                e.observe()
            self.check("injected start")
        else:
            for d in self.devs:
                d.env.buffer(capi.BUF_DONE).fill_(1)
                d.auto_reset(c.seed, 0, self.pf, self.pc)
            self.ora.get(capi.BUF_DONE, copy=False)[:] = 1
            self.ora.auto_reset(c.seed, 0, self.pf, self.pc)
            self.check("stand-alone auto_reset of every env")
        rng = np.random.default_rng(9000 + c.seed)
        # ---- one chunk of 8 steps against 8 single launches ----------------------------------------------------------------------------------------------------------
        acts = np.stack([self.actions(rng, k) for k in range(T_CHUNK)])
        chunk = dict(done=[], req=[], mixed=0, beyond_tr=0, infeasible=0, close_pairs=0)
        recs = [self.ora_step(acts[k], 1 + k, chunk) for k in range(T_CHUNK)]
        if self.devs:
            one, many = self.devs
            ta = torch.as_tensor(acts).cuda()
            rec_one = torch.full((T_CHUNK, B, self.W), float("nan"), device="cuda")
            rec_many = torch.full((T_CHUNK, B, self.W), float("nan"), device="cuda")
            one.env.step_autoreset_n(ta, rec_one, seed=c.seed, counter0=1, path_first=self.pf, path_count=self.pc)
            for k in range(T_CHUNK):
                many.env.set_slab(rec_many[k])
                many.env.step_autoreset(ta[k], c.seed, 1 + k, self.pf, self.pc)
            many.env.set_slab(None)
            for d in self.devs:
                d.env.sync()
            h_one, h_many = rec_one.cpu().numpy(), rec_many.cpu().numpy()
            tt._assert_same_bits(f"{c.name}: chunk", "rollout record", h_one.reshape(T_CHUNK * B, -1), h_many.reshape(T_CHUNK * B, -1), 1, self.G)
            for k in range(T_CHUNK):
                row = h_one[k]
                assert np.abs(row[:, :N * self.D].reshape(B, N, self.D).astype(np.float64) - recs[k][0]).max() <= tp.FTOL, f"{c.name}: record observation, step {k}"
                assert np.abs(row[:, N * self.D:N * self.D + N].astype(np.float64) - recs[k][1]).max() <= tp.FTOL, f"{c.name}: record reward, step {k}"
                assert np.array_equal(row[:, -1] != 0, recs[k][2]), f"{c.name}: record done flags, step {k}"
        self.check(f"after the chunk of {T_CHUNK} steps")
        # ---- separate launches: step, then the stand-alone auto_reset, on the state the chunk left --------------------------------------------------------------
        tail = dict(done=[], req=[], mixed=0, beyond_tr=0, infeasible=0, close_pairs=0)
        for k in range(4):
            act = self.actions(rng, T_CHUNK + k)
            for d in self.devs:
                d.step(act)
            for d in self.devs:
                d.auto_reset(c.seed, 100 + k, self.pf, self.pc)
            self.ora_step(act, 100 + k, tail)
            self.check(f"step + stand-alone auto_reset {k}")
        self.ora.close()
        # ---- the conditions, on the oracle's buffers --------------------------------------------------------------------------------------------------------------
        assert sum(chunk["done"][:T_CHUNK - 1]) > 0, f"{c.name}: no env restarted before the last step of the chunk"
        assert chunk["done"][T_CHUNK - 1] > 0, f"{c.name}: no env restarted in the last step of the chunk"
        assert sum(tail["done"]) + sum(tail["req"]) > 0, f"{c.name}: the stand-alone auto_reset after the chunk had nothing to do"
        if c.G > 1 and not c.testing:  # (in testing mode a collision re-places the agent and the env goes on: its envs finish together, by the step count)
            assert chunk["mixed"] > 0, f"{c.name}: no step of the chunk with a tile in which some envs finished and others did not"
        if c.testing:
            assert self.cfg.has_entry_exit and sum(chunk["req"][:T_CHUNK - 1]) > 0, f"{c.name}: no per-agent request inside the chunk"
        if c.injected:
            assert chunk["beyond_tr"] > 0, f"{c.name}: no agent accepted a try beyond its first {MAX_TRIES // N}"
            assert chunk["infeasible"] > 0 and chunk["close_pairs"] > 0, f"{c.name}: no agent without a feasible try (a pair closer than the minimum start distance)"
        return chunk, tail


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_meets_its_conditions_on_the_oracle(c):
    """No GPU: the case's workload on the oracle alone (the GPU test asserts the same on the same run)."""
    assert c.B <= 48 and (c.G == 1 or c.B % c.G != 0)  # a ragged last tile
    chunk, tail = _Run(c, []).run()
    print(f"{c.name}: finished envs per chunk step {chunk['done']}, requests {chunk['req']}, mixed tiles {chunk['mixed']}, tries beyond TR {chunk['beyond_tr']}, "
          f"agents without a feasible try {chunk['infeasible']}, close pairs {chunk['close_pairs']}; after the chunk: finished {tail['done']}, requests {tail['req']}")


def test_the_cases_cover_the_lane_layouts():
    assert sorted({MAX_TRIES // c.N for c in CASES}) == [2, 3, 4, 8, 16, 21, 64]  # tries per agent held by the lanes
    assert any(MAX_TRIES // c.N * c.N < 64 for c in CASES)  # lanes beyond N * TR idle (3 x 21 = 63)
    assert any(c.injected and c.N == 32 for c in CASES) and any(c.testing for c in CASES)
    assert all(c.G * c.N <= 64 for c in CASES) and len({c.name for c in CASES}) == len(CASES)


@gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_restart_from_registers_chunk_against_single_launches_and_oracle(c, monkeypatch):
    cfg, mp, _ = _config(c)
    devs = [tt._handle(monkeypatch, cfg, mp, c.G, {}) for _ in range(2)]
    try:
        for d in devs:
            ls = d.env.launch_shape()
            tiles = (c.B + c.G - 1) // c.G
            assert (ls["wave_G"], ls["wave_wpb"], ls["wave_grid"]) == (c.G, 1, tiles), ls
            assert ls["wave_spec"] == (c.N * 256 + c.G if c.fixed else 0), ls
            assert ls["instantiation"] == ((True, True, c.N, c.G, False, False) if c.fixed else (True, 2 * c.G * c.N <= 64, 0, 0, False, False)), ls
            assert ls["G"] == c.G, ls
        _Run(c, devs).run()
    finally:
        for d in devs:
            d.close()
