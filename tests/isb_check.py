"""The yardstick of the challenging initial-state buffer (sigmarl_amd/csrc/sigmaenv_isb.h; the contract: include/sigmaenv.h, sigmaenv_isb_*) -- no GPU and no pytest
here: a plain numpy twin like prb_check.py, imported by the tests (tests/test_isb_check.py holds the header compiled alone to it bit for bit; tests/test_gpu_isb.py
holds the kernels to it as words).

The twin is written env by env, in the order the specification states the steps -- one Python loop per rule, no vector tricks that would restate the kernels' scan.
``Twin(defect=...)`` plants one of ``DEFECTS``; every one of them must fail a named check of tests/test_isb_check.py."""
import numpy as np

from policy_head_check import rng_u32

DRAW_RECORD, DRAW_USE, DRAW_INDEX = 5100, 5101, 5102  # sigmaenv_dist.h: DRAW_ISB_RECORD, DRAW_ISB_USE, DRAW_ISB_INDEX
CHUNK = 1024  # ISB_CHUNK: envs per chunk of the record workgroup

DEFECTS = ("ranks_descending", "keep_first", "nth_newest", "index_mod_capacity", "use_before_count", "settle_skips_pending", "push_after_read")


def uniform(k):
    """sigmaenv_dist.h rng_uniform: (k >> 8) * 2^-24, exact in float32, never 1"""
    return (np.asarray(k, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def below(k, n):
    """sigmaenv_dist.h rng_below: the high word of k * n"""
    return int((int(k) * int(n)) >> 32)


def words(seed, counter, base, B, draw):
    """the word of every env b = 0 .. B - 1 under the key (seed, counter, base + b, agent 0, draw)"""
    return rng_u32(seed, counter, (np.arange(B, dtype=np.uint64) + np.uint64(base)).astype(np.uint32), 0, draw).reshape(B)


class Twin:
    """The bank of ``B`` envs of ``N`` agents: ``bank_state [capacity, N, 8]`` float32, ``bank_path [capacity, N, 4]`` int32, ``ptr``, ``count``; per env a ring
    ``ring_state [B, S, N, 8]`` / ``ring_path [B, S, N, 4]`` with ``held`` / ``head``; the episode copy ``epi`` and ``pending``."""

    def __init__(self, B, N, capacity, n_steps_stored, p_record=1.0, p_use=0.2, env_index_base=0, defect=None):
        assert defect is None or defect in DEFECTS
        self.B, self.N, self.capacity, self.S, self.base, self.defect = int(B), int(N), int(capacity), int(n_steps_stored), int(env_index_base), defect
        self.p_record, self.p_use = np.float32(p_record), np.float32(p_use)
        self.bank_state = np.zeros((self.capacity, self.N, 8), np.float32)
        self.bank_path = np.zeros((self.capacity, self.N, 4), np.int32)
        self.ptr = self.count = self.count_before = 0
        self.ring_state = np.zeros((self.B, self.S, self.N, 8), np.float32)
        self.ring_path = np.zeros((self.B, self.S, self.N, 4), np.int32)
        self.held, self.head, self.epi = (np.zeros(self.B, np.int32) for _ in range(3))
        self.pending = np.zeros(self.B, np.uint8)

    # ---- the ring of one env
    def push(self, b, state, path):
        slot = int(self.head[b])
        self.ring_state[b, slot], self.ring_path[b, slot] = state[b], path[b]
        self.head[b] = (slot + 1) % self.S
        self.held[b] = min(int(self.held[b]) + 1, self.S)
        return slot

    def nth_latest(self, b, n):
        if self.defect == "nth_newest":
            n = 1
        return int((int(self.head[b]) - n) % self.S) if int(self.held[b]) >= n else 0

    def reset(self, state, path, timer):
        self.ptr = self.count = self.count_before = 0  # (the bank's rows are left, as on the device: nothing at or above count is ever read)
        self.held[:], self.head[:], self.pending[:] = 0, 0, 0
        for b in range(self.B):
            self.push(b, state, path)
            self.epi[b] = timer[b, 3]

    # ---- record
    def record(self, state, path, col_agents, col_flags, done, seed, counter):
        """Returns what the step decided: ``pushed`` (ring slot per env), ``collided``, ``records``, ``rank`` (-1: no recorder), ``src`` / ``dst`` (ring / bank slot of a
        recorder whose write survives, else -1)."""
        B = self.B
        pushed = np.full(B, -1, np.int32)
        src = np.full(B, -1, np.int32)
        if self.defect == "push_after_read":
            for b in range(B):
                src[b] = self.nth_latest(b, self.S)
            snap_state, snap_path = self.ring_state.copy(), self.ring_path.copy()
        for b in range(B):
            pushed[b] = self.push(b, state, path)
        collided = np.array([bool(np.any(col_agents[b] != 0)) for b in range(B)])
        one_minus = np.float32(1.0) - self.p_record
        u = uniform(words(seed, counter, self.base, B, DRAW_RECORD))
        records = np.array([bool(collided[b]) and bool(u[b] > one_minus) for b in range(B)])
        order = [b for b in range(B) if records[b]]
        if self.defect == "ranks_descending":
            order = order[::-1]
        R = len(order)
        rank = np.full(B, -1, np.int32)
        dst = np.full(B, -1, np.int32)
        for k, b in enumerate(order):
            rank[b] = k
            kept = k < self.capacity if self.defect == "keep_first" else k >= R - self.capacity
            if not kept:
                src[b] = -1
                continue
            if self.defect == "push_after_read":
                s = int(src[b])
                row_s, row_p = snap_state[b, s], snap_path[b, s]
            else:
                s = self.nth_latest(b, self.S)
                row_s, row_p = self.ring_state[b, s], self.ring_path[b, s]
            src[b], dst[b] = s, (self.ptr + k) % self.capacity
            self.bank_state[dst[b]], self.bank_path[dst[b]] = row_s, row_p
        for b in range(B):
            if not records[b]:
                src[b] = -1
        self.count_before = self.count
        self.ptr = (self.ptr + R) % self.capacity
        self.count = min(self.count + R, self.capacity)
        for b in range(B):
            self.pending[b] = int(not done[b] and bool(np.any(col_flags[b, :, 3] != 0)))
        return dict(pushed=pushed, collided=collided, records=records, rank=rank, src=src, dst=dst, R=R)

    # ---- restart: the decisions (the reset itself is sigmaenv_reset's: the oracle's twin)
    def restart(self, done, seed, counter):
        """``uses [B]`` bool and ``j [B]`` (-1 where the env does not restart from the bank)"""
        count = self.count_before if self.defect == "use_before_count" else self.count
        uses, j = np.zeros(self.B, bool), np.full(self.B, -1, np.int32)
        u, w = uniform(words(seed, counter, self.base, self.B, DRAW_USE)), words(seed, counter, self.base, self.B, DRAW_INDEX)
        for b in range(self.B):
            uses[b] = bool(done[b]) and count >= 1 and bool(u[b] < self.p_use)
            if uses[b]:
                j[b] = below(w[b], self.capacity if self.defect == "index_mod_capacity" else count)
        return uses, j

    # ---- settle
    def settle(self, state, path, timer):
        settled = np.zeros(self.B, bool)
        for b in range(self.B):
            pend = bool(self.pending[b]) and self.defect != "settle_skips_pending"
            if int(timer[b, 3]) != int(self.epi[b]) or pend:
                settled[b] = True
                self.held[b] = self.head[b] = 0
                self.push(b, state, path)
                self.epi[b] = timer[b, 3]
                self.pending[b] = 0
        return settled


# ---- a scripted run on tagged rows: what tests/test_isb_check.py feeds the header's program and the twin alike -------------------------------------------------------
def tag_rows(tags):
    """rows whose every word is the env's tag: ``state [B, 1, 8]`` float32 (the tag's value), ``path [B, 1, 4]`` int32"""
    tags = np.asarray(tags, np.int32)
    return np.repeat(tags.astype(np.float32)[:, None, None], 8, axis=2), np.repeat(tags[:, None, None], 4, axis=2)


def make_script(B, capacity, S, steps, recorders, seed, p_done=0.3, p_request=0.2):
    """``steps`` frames: ``collided``, ``done``, ``request`` u8 ``[steps, B]``; ``tag_step`` / ``tag_fresh`` int32 ``[steps, B]`` (the rows a step leaves / a reset places).
    ``recorders[t]``: how many envs collide at step t (the lowest-numbered ones of a random permutation), or None for a coin per env."""
    rng = np.random.default_rng(seed)
    col = np.zeros((steps, B), np.uint8)
    for t in range(steps):
        r = recorders[t % len(recorders)]
        if r is None:
            col[t] = rng.random(B) < 0.5
        else:
            col[t, rng.permutation(B)[: min(r, B)]] = 1
    done = (rng.random((steps, B)) < p_done).astype(np.uint8)
    done |= col & (rng.random((steps, B)) < 0.7).astype(np.uint8)  # (a collision usually ends the env; not always: testing mode re-places one agent)
    request = (rng.random((steps, B)) < p_request).astype(np.uint8)
    tag_step = (1 + np.arange(steps * B, dtype=np.int32).reshape(steps, B)) * 2
    tag_fresh = tag_step + 1
    return dict(B=B, capacity=capacity, S=S, steps=steps, collided=col, done=done, request=request, tag_step=tag_step, tag_fresh=tag_fresh)


def run_script(sc, p_record, p_use, seed, counter0=0, env_index_base=0, defect=None):
    """The script through the twin: per step record -> restart decisions -> (the resets, on the tags) -> settle.  Returns the per-step decisions and the final state, all
    int32 arrays, under the names the header's program prints them."""
    B, steps = sc["B"], sc["steps"]
    tw = Twin(B, 1, sc["capacity"], sc["S"], p_record, p_use, env_index_base, defect)
    rows = np.zeros(B, np.int32)
    timer = np.zeros((B, 4), np.int32)
    tw.reset(*tag_rows(rows), timer)
    keys = ("pushed", "records", "rank", "src", "dst", "ptr", "count", "uses", "j", "settled", "rows")
    out = {k: [] for k in keys}
    for t in range(steps):
        rows = sc["tag_step"][t].copy()
        col_agents = sc["collided"][t][:, None, None]
        col_flags = np.zeros((B, 1, 4), np.uint8)
        col_flags[:, 0, 3] = sc["request"][t]
        done = sc["done"][t]
        st, pa = tag_rows(rows)
        r = tw.record(st, pa, col_agents, col_flags, done, seed, counter0 + t)
        uses, j = tw.restart(done, seed, counter0 + t)
        for b in range(B):
            if uses[b]:
                rows[b] = tw.bank_path[min(int(j[b]), tw.capacity - 1), 0, 0]
                timer[b, 3] += 1
            elif done[b]:
                rows[b] = sc["tag_fresh"][t, b]
                timer[b, 3] += 1
            elif sc["request"][t, b]:
                rows[b] = sc["tag_fresh"][t, b]
        settled = tw.settle(*tag_rows(rows), timer)
        for k in ("pushed", "rank", "src", "dst"):
            out[k].append(r[k])
        out["records"].append(r["records"].astype(np.int32))
        out["ptr"].append(np.int32(tw.ptr)); out["count"].append(np.int32(tw.count))
        out["uses"].append(uses.astype(np.int32)); out["j"].append(j); out["settled"].append(settled.astype(np.int32)); out["rows"].append(rows.copy())
    res = {k: np.asarray(v, np.int32) for k, v in out.items()}
    res.update(bank=tw.bank_path[:, 0, 0].copy(), ring=tw.ring_path[:, :, 0, 0].copy(), held=tw.held.copy(), head=tw.head.copy())
    return res


# ---- the run that really records (tests/test_gpu_isb.py; the seed was picked with the oracle: tests/test_isb_check.py::test_the_recording_run_on_the_oracle) -----------
RECORDING_RUN = dict(N=4, B=64, T=64, capacity=100, n_steps_stored=10, p_use=0.5, seed=1)


def recording_run_on_the_oracle(r=RECORDING_RUN):
    """CPM, full speed straight ahead: the oracle steps, the twin records and decides, the oracle restarts (``reset(full_env=1)``) and re-places.  Returns
    ``(recorded, restarted)``."""
    import oracle_binding as ob
    from sigmarl_amd import capi
    from sigmarl_amd.maps import load_map
    from sigmarl_amd.params import Parameters, make_config

    N, B, seed = r["N"], r["B"], r["seed"]
    p = Parameters(n_agents=N, scenario_type="cpm_entire", is_use_mtv_distance=False, is_apply_mask=False, is_obs_noise=False)
    mp = load_map("cpm_entire")
    ora = ob.OracleEnv(make_config(p, mp, B), mp)
    first, count = mp.list_first[0], mp.list_count[0]
    ora.get(capi.BUF_DONE, copy=False)[:] = 1
    ora.auto_reset(seed, 0, first, count)
    tw = Twin(B, N, r["capacity"], r["n_steps_stored"], 1.0, r["p_use"])
    g = lambda w: ora.get(w)  # noqa: E731
    tw.reset(g(capi.BUF_STATE), g(capi.BUF_PATH), g(capi.BUF_TIMER))
    act = np.zeros((B, N, 2), np.float32)
    act[..., 0] = capi.AGENTS["max_speed"]
    recorded = restarted = 0
    for t in range(r["T"]):
        ora.step(act)
        done = g(capi.BUF_DONE)
        recorded += tw.record(g(capi.BUF_STATE), g(capi.BUF_PATH), g(capi.BUF_COL_AGENTS), g(capi.BUF_COL_FLAGS), done, seed, 1 + t)["R"]
        uses, j = tw.restart(done, seed, 1 + t)
        if uses.any():
            idx = np.nonzero(uses)[0]
            ora.reset(np.repeat(idx, N).astype(np.int32), np.tile(np.arange(N, dtype=np.int32), len(idx)), tw.bank_path[j[idx]].reshape(-1, 4),
                      tw.bank_state[j[idx]].reshape(-1, 8), True)
        restarted += int(uses.sum())
        ora.auto_reset(seed, 1 + t, first, count)
        tw.settle(g(capi.BUF_STATE), g(capi.BUF_PATH), g(capi.BUF_TIMER))
    ora.close()
    return recorded, restarted
