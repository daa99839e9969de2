"""The yardstick of the prioritized replay buffer (sigmarl_amd/csrc/sigmaenv_prb.h; the contract: include/sigmaenv.h, sigmaenv_prb_*) -- no GPU and no pytest here:
  * a float64 reference of every formula: priority, the lower-bound scan over the prefix sums, weight, x_m, the minibatch normalisation;
  * a float32 twin of the header in numpy: the levels (sum and min), total / q_min, the descent, x_m, the normalisation -- the SAME operations in the SAME order, so
    the header compiled alone (tests/test_prb_check.py) and the kernels fed the device's own leaves (tests/test_gpu_prb.py) must equal it bit for bit.  The two
    powers (priority, weight) are the only operations it cannot reproduce to the bit (another libm): they are held to float64 within a bar in ulp;
  * the generator's draw 7400 (policy_head_check.rng_u32 / uniform);
  * the admissibility test of a sampled index against float64 prefix sums of the STORED float32 leaves;
  * planted defects of the twin, each of which must miss a bar.
"""
import numpy as np

import policy_head_check as ph

FAN, DRAW = 256, 7400  # DRAW: sigmaenv_dist.h DRAW_REPLAY
ALPHA, BETA, EPS, TD_GAMMA = 0.7, 0.6, 1e-8, 0.9
f32, f64 = np.float32, np.float64
U = 2.0 ** -24  # the unit roundoff of float32
POW_CAP_ULP = 16.0  # the cap the bar of the two powers may never exceed: the eps-dropped defect moves a priority by about 60 ulp at td = 1e-3
POW_HOST_ULP = 3.0  # numpy's float32 power on the host: glibc documents powf within 1 ulp; the rounded input (td + eps, q / q_min: half an ulp times the exponent
#                     <= 1) and the final comparison in float64 add less than one more: 3 with room
DEFECTS = ("upper_bound", "no_clamp", "r_not_reduced", "minmax_whole_buffer", "nd_dropped", "eps_dropped", "div_n_dropped", "weight_plus_beta")


def level_sizes(capacity):
    n = [int(capacity)]
    while n[-1] > FAN:
        n.append((n[-1] + FAN - 1) // FAN)
    return n


def cnt(length, k):
    c = int(length)
    for _ in range(k):
        c = (c + FAN - 1) // FAN
    return c


def uniforms(seed, counter, M):
    """u_m of the slots 0 .. M - 1: draw 7400 keyed (seed, counter, env = m, agent = 0)"""
    return ph.uniform(ph.rng_u32(seed, counter, np.arange(M, dtype=np.uint32), np.uint32(0), DRAW)).astype(f32)


def ulp_of(a, b):
    """|a - b| in units of the float32 spacing at |b| (b: the float64 reference)"""
    b = np.asarray(b, f64)
    return np.abs(np.asarray(a, f64) - b) / np.spacing(np.abs(b).astype(f32)).astype(f64)


# ---- the float32 twin of the header -----------------------------------------------------------------------------------------------------------------------------------
def node_prefix(e):
    """prb_node_prefix on e [.., 256] float32 -> S [.., 256]"""
    e = np.ascontiguousarray(e, f32).reshape(e.shape[:-1] + (64, 4))
    c0 = e[..., 0]
    c1 = c0 + e[..., 1]
    c2 = c1 + e[..., 2]
    c3 = c2 + e[..., 3]
    I = c3.copy()
    for d in (1, 2, 4, 8, 16, 32):
        J = I.copy()
        J[..., d:] = I[..., d:] + I[..., :-d]
        I = J
    E = np.zeros_like(I)
    E[..., 1:] = I[..., :-1]
    return np.stack([E + c0, E + c1, E + c2, I], axis=-1).reshape(e.shape[:-2] + (FAN,))


def _min(a, b):
    return np.where(b < a, b, a)


def node_min(e):
    """prb_node_min on e [.., 256] float32"""
    e = np.ascontiguousarray(e, f32).reshape(e.shape[:-1] + (64, 4))
    with np.errstate(invalid="ignore"):
        m = _min(_min(_min(e[..., 0], e[..., 1]), e[..., 2]), e[..., 3])
        lanes = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            m = _min(m, m[..., lanes ^ s])
    return m[..., 0]


def _nodes(level, valid, n_nodes, fill):
    a = np.full((n_nodes * FAN,), fill, f32)
    v = min(int(valid), level.size)
    a[:v] = level[:v]
    return a.reshape(n_nodes, FAN)


def build(leaves, length, capacity=None):
    """the levels from the leaves: {"sum": [leaves, level 1, ..], "min": [..], "total", "q_min", "n": level sizes}"""
    leaves = np.ascontiguousarray(leaves, f32)
    n = level_sizes(leaves.size if capacity is None else capacity)
    sums, mins = [leaves], [leaves]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(n)):
            valid, nodes = (length if k == 0 else n[k]), (n[k + 1] if k + 1 < len(n) else 1)
            s = node_prefix(_nodes(sums[k], valid, nodes, 0.0))[:, FAN - 1]
            m = node_min(_nodes(mins[k], valid, nodes, np.inf))
            sums.append(s.astype(f32))
            mins.append(m.astype(f32))
    return {"sum": sums[:-1], "min": mins[:-1], "total": sums[-1][0], "q_min": mins[-1][0], "n": n}


def descend(sums, length, mass, defect=None):
    """prb_descend for the masses [M] -> index [M] (int64)"""
    mass = np.asarray(mass, f32)
    M = mass.size
    r, node = mass.copy(), np.zeros(M, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(sums) - 1, -1, -1):
            c = cnt(length, k)
            p = node[:, None] * FAN + np.arange(FAN)[None, :]
            lvl = sums[k]
            e = np.where(p < c, lvl[np.minimum(p, lvl.size - 1)], f32(0.0)).astype(f32)
            S = node_prefix(e)
            last = np.minimum(FAN - 1, c - 1 - node * FAN)
            hit = r[:, None] < S
            j = np.where(hit.any(axis=1), hit.argmax(axis=1), FAN - 1 if defect == "no_clamp" else last)
            if defect == "upper_bound" and k == 0:
                j = j + 1
            if defect != "no_clamp":
                j = np.minimum(j, last)
            prev = np.where(j > 0, S[np.arange(M), np.clip(j - 1, 0, FAN - 1)], f32(0.0)).astype(f32)
            if defect != "r_not_reduced":
                r = (r - prev).astype(f32)
            node = node * FAN + j
    return node


def sample(lv, length, seed, counter, M, u=None, defect=None):
    """(index, mass, u): the twin's sample of M slots from the levels ``lv`` (``u``: forced uniforms instead of the generator's)"""
    u = uniforms(seed, counter, M) if u is None else np.asarray(u, f32)
    mass = (u * f32(lv["total"])).astype(f32)
    return descend(lv["sum"], length, mass, defect), mass, u


def twin_x(reward, done, v, vn, td_gamma=TD_GAMMA, defect=None):
    """prb_x per slot: reward [M, N], done / v / vn [M], float32"""
    reward, done, v, vn = (np.asarray(t, f32) for t in (reward, done, v, vn))
    nd = (f32(1.0) - done).astype(f32)
    boot = (f32(td_gamma) * vn).astype(f32)
    if defect != "nd_dropped":
        boot = (boot * nd).astype(f32)
    x = np.zeros(v.shape, f32)
    for i in range(reward.shape[1]):
        x = (x + np.abs(((reward[:, i] + boot).astype(f32) - v).astype(f32))).astype(f32)
    return x if defect == "div_n_dropped" else (x / f32(reward.shape[1])).astype(f32)


def twin_norm(x, mn, mx):
    """prb_norm"""
    x = np.asarray(x, f32)
    rng = np.maximum(f32(mx) - f32(mn), f32(1e-3)).astype(f32)
    y = (((x - f32(mn)).astype(f32) / rng).astype(f32) * f32(10.0)).astype(f32)
    return np.minimum(np.maximum(y, f32(1e-3)), f32(10.0)).astype(f32)


def twin_priority(td, eps=EPS, alpha=ALPHA, defect=None):
    td = np.asarray(td, f32)
    base = td if defect == "eps_dropped" else (td + f32(eps)).astype(f32)
    return np.power(base, f32(alpha)).astype(f32)


def twin_weight(q, q_min, beta=BETA, defect=None):
    e = f32(beta) if defect == "weight_plus_beta" else -f32(beta)
    return np.power((np.asarray(q, f32) / f32(q_min)).astype(f32), e).astype(f32)


def twin_refresh(case, defect=None):
    """(x [M], td [M]) of the valid slots' formulas on a refresh case (``make_refresh_case``); invalid slots hold NaN"""
    idx, length = case["index"], case["len"]
    ok = (idx >= 0) & (idx < length)
    f = np.where(ok, idx, 0)
    x = twin_x(case["reward"][f], case["done"][f], case["v"], case["vn"], case["td_gamma"], defect)
    if defect == "minmax_whole_buffer":  # over every frame of the buffer, with the critic's values of the frames' first slots (frames never sampled: value 0)
        vf, vnf = np.zeros(length, f32), np.zeros(length, f32)
        vf[f[ok][::-1]], vnf[f[ok][::-1]] = case["v"][ok][::-1], case["vn"][ok][::-1]
        pool = twin_x(case["reward"][:length], case["done"][:length], vf, vnf, case["td_gamma"])
    else:
        pool = x[ok]
    td = twin_norm(x, pool.min(), pool.max())
    x, td = x.copy(), td.copy()
    x[~ok], td[~ok] = np.nan, np.nan
    return x, td


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------------------------------------
def ref_priority(td, eps=EPS, alpha=ALPHA):
    return np.power(np.asarray(td, f32).astype(f64) + float(f32(eps)), float(f32(alpha)))


def ref_weight(q, q_min, beta=BETA):
    return np.power(np.asarray(q, f32).astype(f64) / float(q_min), -float(f32(beta)))


def ref_x(reward, done, v, vn, td_gamma=TD_GAMMA):
    reward, done, v, vn = (np.asarray(t, f32).astype(f64) for t in (reward, done, v, vn))
    return np.abs(reward + (float(f32(td_gamma)) * vn * (1.0 - done))[:, None] - v[:, None]).sum(axis=1) / reward.shape[1]


def ref_norm(x, mn, mx):
    return np.clip((x - mn) / max(mx - mn, float(f32(1e-3))) * 10.0, float(f32(1e-3)), 10.0)


def ref_refresh(case):
    idx, length = case["index"], case["len"]
    ok = (idx >= 0) & (idx < length)
    f = np.where(ok, idx, 0)
    x = ref_x(case["reward"][f], case["done"][f], case["v"], case["vn"], case["td_gamma"])
    td = ref_norm(x, x[ok].min(), x[ok].max())
    x[~ok], td[~ok] = np.nan, np.nan
    return x, td


def x_bound(case):
    """|x32 - x64| per slot.  prb_x: fl(td_gamma v') and its product with nd (2 roundings of a term of size |g v'|), per agent the sum r + boot, the difference with
    v and the addition into the chain (3 roundings of terms of size <= |r| + |g v'| + |v|, and the chain's value is at most N times that), the division: first
    order, per slot, with s = max_i |r_i| + |g v'| + |v|:  ((2 + 3) + N + 1) u s  -- the chain's N additions each round a value <= N s, averaged by / N."""
    idx = np.clip(case["index"], 0, case["len"] - 1)
    s = np.abs(case["reward"][idx]).max(axis=1).astype(f64) + np.abs(case["td_gamma"] * case["vn"].astype(f64)) + np.abs(case["v"].astype(f64))
    return (6 + case["reward"].shape[1]) * U * s + 1e-45


def td_bound(case, x64):
    """|td32 - td64| per slot: td = clamp(10 (x - min) / range): the errors of x, min and max enter through 10 / range times (|dx| + |dmin|) + td / range (|dmax| +
    |dmin|) <= (10 / range) 4 max|dx|; the subtraction, the division and the product round three times more (3 u td, td <= 10)."""
    ok = ~np.isnan(x64)
    rng = max(x64[ok].max() - x64[ok].min(), 1e-3)
    return 10.0 / rng * 4.0 * x_bound(case)[ok].max() + 3 * U * 10.0 + np.zeros(x64.shape)


# ---- admissibility of a sampled index ---------------------------------------------------------------------------------------------------------------------------------
def rounding_count(n_levels):
    """The roundings between the exact prefix sums of the stored leaves and what the descent compares, for L levels (the summation order the header states):
      a prefix S_j inside a node: the lane chain (<= 3 additions), the scan (6) and E + c_i (1): depth 10;
      an entry of level k is a node sum of level k - 1 (depth 9: chain 3 + scan 6), k levels deep: 9 k -- so a prefix of level k has depth 10 + 9 k; for sums of
        non-negative terms a depth d costs a relative error of d u: at most d u total;
      the bracket S_{j-1} <= r < S_j holds at every level with r = r' - S'_{j'-1}: L - 1 subtractions, one rounding each, of values <= total;
      mass = fl(u total): 1.
    d(L) = 1 + (L - 1) + sum_{k < L} (10 + 9 k) roundings of at most u total <= ulp(total) each, i.e. 2 d(L) times ulp(total) / 2.  (L = 3: d = 60.)"""
    L = int(n_levels)
    return 2 * (1 + (L - 1) + sum(10 + 9 * k for k in range(L)))


def admissible(leaves, length, index, u, total, n_levels):
    """per slot: index in [0, len) and C[f - 1] - tol <= mass <= C[f] + tol (the upper side open at len - 1), C the float64 prefix sums of the stored float32 leaves,
    mass = u total in float64, tol = rounding_count(L) ulp(total) / 2"""
    index = np.asarray(index, np.int64)
    inside = (index >= 0) & (index < length)
    C = np.cumsum(np.asarray(leaves, f32)[:length].astype(f64))
    f = np.clip(index, 0, length - 1)
    mass = np.asarray(u, f32).astype(f64) * float(total)
    tol = rounding_count(n_levels) * float(np.spacing(f32(total))) / 2.0
    lo = np.where(f > 0, C[np.maximum(f - 1, 0)], 0.0)
    return inside & (lo - tol <= mass) & ((mass <= C[f] + tol) | (f == length - 1))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------------------
LEAF_SETS = ("random", "all_equal", "one_huge", "chunk_edge", "nan_leaf")


def make_td(kind, length, seed=0):
    """TD errors in [1e-3, 10] (what sigmaenv_gae writes) whose priorities (td + eps)^alpha give the adversarial leaf sets"""
    rng = np.random.default_rng(seed)
    td = rng.uniform(1e-3, 10.0, length).astype(f32)
    if kind == "all_equal":
        td[:] = 1.0
    elif kind == "one_huge":  # one leaf 10^4 times the rest: a td ratio of 10^(4 / alpha)
        td[:] = 1e-3
        td[length // 2] = 1e-3 * 10.0 ** (4.0 / ALPHA)
    elif kind == "chunk_edge":  # the mass in the last leaf of a chunk and the first of the next
        td[:] = 1e-3
        if length > FAN:
            td[FAN - 1], td[FAN] = 10.0, 10.0
        else:
            td[length - 1] = 10.0
    elif kind == "nan_leaf":
        td[length // 3] = np.nan
    return td


def make_refresh_case(F, N, M, seed, dup=False, equal=False, out_of_range=False, done_all=False):
    rng = np.random.default_rng(seed)
    case = {"len": F, "td_gamma": f32(TD_GAMMA), "reward": rng.normal(0, 1, (F, N)).astype(f32), "done": (rng.uniform(size=F) < 0.25).astype(f32),
            "index": rng.integers(0, F, M).astype(np.int32), "v": rng.normal(0, 1, M).astype(f32), "vn": rng.normal(0, 1, M).astype(f32)}
    if done_all:
        case["done"][:] = 1.0
    if dup:  # many duplicates of one frame: the same frame has the same values
        case["index"][M // 4:] = case["index"][0]
    if equal:  # every x_m equal: zero rewards and values
        case["reward"][:], case["v"][:], case["vn"][:] = 0.0, 0.5, 0.0
    same = {}
    for m, f in enumerate(case["index"]):  # (one frame, one critic value: duplicates compute the same bits)
        m0 = same.setdefault(int(f), m)
        case["v"][m], case["vn"][m] = case["v"][m0], case["vn"][m0]
    if out_of_range and M > 1:
        case["index"][M // 2] = F + 3
        if M > 2:
            case["index"][1] = -1
    return case
