"""The bf16 actor kernel (sigmaenv_actor_kernel in sigmarl_amd/csrc/sigmaenv_actor.inc) held BIT FOR BIT to a float64 restatement: a plain helper module like
network_check.py / policy_head_check.py (numpy, torch only for the module object; tests/test_bf16_actor_check.py runs it on the host, tests/test_gpu_bf16_actor_exact.py
on the device).

Why a construction.  On a dense network the kernel can only be held to its restatement within a tolerance: the summation order inside v_mfma_f32_16x16x32_bf16 is
not known, and an activation rounded to bf16 is discontinuous in its argument.  Both obstacles are removed by construction, and what remains has ONE possible result.

The network (``make_net``): D -> 256 -> 256 -> 256 -> 4 in torch.nn.Linear layout, every number dyadic and bf16-exact.  Layer 1 dense, weights k / 8 with k = -8 .. 8;
layers 2 and 3 with 16 non-zero weights per output feature, from {+-1/2, +-1}, at random positions (an input feature feeds about 16 outputs); layer 4 with four
disjoint supports of 64 features (together all 256), weights +-1/8; biases multiples of 1/8 in [-1/2, 1/2].  The inputs (``make_input``): x = xh + d, xh a bf16-exact
multiple of 2^-10 with |xh| < 2, |d| < 0.45 bf16 ulp of xh (the kernel's own input rounding has something to round), and ``TIES`` columns per row EXACTLY on a bf16
rounding midpoint, a mantissa of either parity below them (ties-to-even is pinned both ways).  The spread of xh keeps the pre-activations at a standard deviation of
about 1.5 at every width: smaller ones have finely spaced bf16 neighbours, and fewer rows can be certified.

``reference``  bf16 round-to-nearest-even of the inputs and of tanh (the float64 tanh is rounded DIRECTLY to bf16, never through fp32: no double rounding), exact sums,
(loc, raw) out.

``certify``  the verdict per row, from the reference alone.  A row is certified when every feature of every layer passes both certificates:

  exactness, per (row, layer, output feature).  q: the smallest integer such that the bias and every product w_k x_k are multiples of 2^-q (bf16 x bf16 is exact in
      fp32); M = |b| + sum |w_k x_k|.  Required: M < 2^(ACC_BITS - q), ACC_BITS = 24 - SPARE_BITS = 22.  Then every partial sum in every order and grouping is a
      multiple of 2^-q below 2^22 2^-q: an fp32 number with SPARE_BITS = 2 bits to spare.  The spare bits are for a matrix pipe that aligns its addends to the
      largest and truncates instead of rounding each sum: it may then keep two bits fewer than an fp32 adder and still drop nothing.
  activation, per hidden activation a (known exactly).  The device computes fast_tanh(a) = 1 - 2 rcp(1 + exp2(fl(a * C32))), C32 = fl(2 / ln 2).  ``fast_tanh_error``
      bounds its absolute error against tanh(a) by carrying an interval through these operations, each widened by its rounding: the product's (2^-24 relative), exp2 and
      rcp by ``HW_ULPS`` = 1 ulp each (2^-23 relative), the sum 1 + e (2^-24), the final subtraction (2^-24 of the result; 2 rcp is exact, and the build forbids
      contraction); the gap between C32 and 2 / ln 2 is inside because the interval is compared with the real tanh.  Every step is monotone, so the ends of the interval
      are its worst cases: no first-order approximation.  At worst E = 7.13 * 2^-24 = 4.3e-7 (at a = -1.53), at most 4 * 2^-24 for a > 0.
      Certified: the distance of tanh(a) to the nearest bf16 rounding midpoint exceeds ``MARGIN`` * E(a), MARGIN = 2: once for
      the bound, once more so that a hardware function which is a little worse than assumed shows up as failing rows with ratios near 1 rather than passing by luck.
      The midpoints are those between the bf16 number tanh(a) rounds to and its two neighbours, so below a power of two the finer spacing is taken.  a = 0 gives
      exp2(0) = 1, rcp(2) = 1/2 and 1 - 1 = 0 exactly and is always certified.

ASSUMPTION: v_exp_f32 and v_rcp_f32 are within one ulp, exact at exp2(0) and rcp(2) (sigmaenv_mlp32s.inc makes the same assumption for its tanh).  It is not measured
here.  For |a| below about 2^-9 the error of fast_tanh is no longer far below the bf16 spacing of tanh(a) (2^-17 there, E about 3 * 2^-24): such activations are
hardly ever certified, and the rows that hold one are left out.  ``MIN_SHARE`` = 0.75 caps what may be left out: at least three quarters of a pool of 1120 rows must be
certified at every width (host test); a construction that misses it is changed, not the cap.

``compare``  the device's loc_scale rows against the reference: loc with ==  on the words, the scale through policy_head_check.compare_scale with a raw bound of 0 (raw
is exact on a certified row; what remains is the fp32 softplus of actor_distribution).  A failure names rows, outputs and each failing row's smallest certificate ratio:
a structural defect fails rows of any ratio, an assumption on fast_tanh that is too tight only rows whose ratio is near 1.
"""
from __future__ import annotations

import functools

import numpy as np

import network_check as nc
import policy_head_check as ph

H = 256
SPARE_BITS = 2                 # bits of an fp32 significand the exactness certificate leaves unused (an aligning, truncating adder)
ACC_BITS = 24 - SPARE_BITS
HW_ULPS = 1.0                  # assumed error of v_exp_f32 and v_rcp_f32, in ulps
MARGIN = 2.0                   # times E(a): see the module docstring
MIN_SHARE = 0.75               # least certified share of a pool of POOL_ROWS rows
POOL_ROWS = 1120
TIES = 2                       # columns per row exactly on a bf16 midpoint
U = 2.0 ** -24                 # unit roundoff of fp32
C32 = float(np.float32(2.8853900817779268))  # the kernel's constant, as fp32 holds it
F64_SLOP = 2.0 ** -50          # numpy's float64 tanh / exp2 and the few float64 operations of the interval, generously


# ---- roundings ------------------------------------------------------------------------------------------------------------------------------
def bf16_from_f64(v):
    """float64 -> nearest bf16 (ties to even) as float64, in one rounding.  (bf16 subnormals, below 2^-126, are not handled: tanh of a dyadic a of this module is either
    0 or far above.)"""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(np.abs(v))                      # |v| = m 2^e, m in [1/2, 1)
    return np.copysign(np.ldexp(np.rint(m * 256.0), e - 8), v)  # 8 significant bits; rint rounds half to even


def midpoint_distance(t):
    """The distance of t (float64) to the nearer of the two rounding midpoints around the bf16 number it rounds to; inf for t = 0."""
    t = np.abs(np.asarray(t, np.float64))
    r = bf16_from_f64(t)
    m, e = np.frexp(r)
    up = np.ldexp(1.0, e - 8)                        # spacing above r
    dn = np.where(m == 0.5, 0.5 * up, up)            # below a power of two the spacing is half
    d = np.minimum(r + 0.5 * up - t, t - (r - 0.5 * dn))
    return np.where(t == 0.0, np.inf, d)


def fast_tanh_error(a, hw_ulps=HW_ULPS):
    """E(a): a bound on |fast_tanh(a) - tanh(a)| for the fp32 number a, as the interval of the module docstring."""
    a = np.asarray(a, np.float64)
    h = hw_ulps * 2.0 * U
    with np.errstate(over="ignore", under="ignore"):
        p = a * C32                                  # exact in float64 (24 x 24 bits)
        dp = np.abs(p) * U
        e_lo, e_hi = np.exp2(p - dp) * (1.0 - h), np.exp2(p + dp) * (1.0 + h)
        s_lo, s_hi = (1.0 + e_lo) * (1.0 - U), (1.0 + e_hi) * (1.0 + U)
        r_lo, r_hi = (1.0 - h) / s_hi, (1.0 + h) / s_lo
        t_lo, t_hi = 1.0 - 2.0 * r_hi, 1.0 - 2.0 * r_lo
    t = np.tanh(a)
    return np.maximum(t_hi - t, t - t_lo) + U * np.maximum(np.abs(t_lo), np.abs(t_hi)) + F64_SLOP


def _q(v, bits=24):
    """The smallest q with v 2^q an integer, for numbers of at most ``bits`` significant bits; a large negative number for 0."""
    m, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    i = np.ldexp(m, bits).astype(np.int64)
    tz = np.round(np.log2(np.maximum(i & -i, 1))).astype(np.int64)
    return np.where(i == 0, -10000, bits - e - tz)


# ---- the construction -------------------------------------------------------------------------------------------------------------------------
def make_net(D, seed):
    """The network of the module docstring as a torch.nn.Sequential (CPU, float32)"""
    import torch
    g = np.random.default_rng([seed, D, 1])
    L, T = torch.nn.Linear, torch.nn.Tanh
    net = torch.nn.Sequential(L(D, H), T(), L(H, H), T(), L(H, H), T(), L(H, 4))
    w = [g.integers(-8, 9, (H, D)) / 8.0]
    for _ in range(2):
        m = np.zeros((H, H))
        for f in range(H):
            m[f, g.choice(H, 16, replace=False)] = g.choice([-1.0, -0.5, 0.5, 1.0], 16)
        w.append(m)
    m, perm = np.zeros((4, H)), g.permutation(H)
    for o in range(4):
        m[o, perm[64 * o:64 * o + 64]] = g.choice([-0.125, 0.125], 64)
    w.append(m)
    with torch.no_grad():
        for lin, wl in zip([x for x in net if isinstance(x, L)], w):
            b = g.integers(-4, 5, wl.shape[0]) / 8.0
            b[-1] = b[-1] if b[-1] else 0.375       # the last feature's bias is never zero: a kernel that drops it is seen
            lin.weight.copy_(torch.from_numpy(wl))
            lin.bias.copy_(torch.from_numpy(b))
    return net


def make_input(rows, D, seed):
    """(x [rows, D] float32, ties [rows, TIES] the tie columns of every row)"""
    g = np.random.default_rng([seed, D, 2])
    spread = min(0.9, 1.5 / np.sqrt(0.375 * D))      # 0.375: the variance of a layer-1 weight
    xh = nc.bf16(np.clip(np.rint(g.normal(0.0, spread, (rows, D)) * 1024.0), -2032, 2032) / 1024.0).astype(np.float64)
    m, e = np.frexp(np.abs(xh))
    ulp = np.ldexp(1.0, e - 8)
    d = g.uniform(-0.45, 0.45, xh.shape) * ulp * np.sign(xh)
    d = np.where((m == 0.5) & (d * xh < 0), 0.5 * d, d)  # towards zero from a power of two the spacing is half
    x = xh + np.where(xh == 0.0, 0.0, d)
    ties = np.stack([g.permutation(D)[:TIES] for _ in range(rows)])
    r = np.arange(rows)[:, None]
    big = np.abs(xh[r, ties]) >= 0.125                  # (there the neighbour is still a multiple of 2^-10)
    x[r, ties] = np.where(big, xh[r, ties] + 0.5 * ulp[r, ties] * np.sign(xh[r, ties]), x[r, ties])
    x32 = x.astype(np.float32)
    off = np.ones(x.shape, bool)
    off[r, ties] = ~big
    assert (nc.bf16(x32)[off] == xh[off]).all() and (x32[r, ties][big] == x[r, ties][big]).all()
    return x32, ties


def layers(net):
    """[(W [F, K], b [F])] in float64, the weights as the pack kernel rounds them (bf16, round to nearest even)"""
    import torch
    return [(nc.bf16(m.weight.detach().cpu().numpy()).astype(np.float64), m.bias.detach().cpu().numpy().astype(np.float64))
            for m in net.modules() if isinstance(m, torch.nn.Linear)]


# ---- reference and certificates ---------------------------------------------------------------------------------------------------------------
def reference(net, x):
    """dict(out [rows, 4] = (loc0, loc1, raw0, raw1), h: the bf16 inputs of the four layers, a: the pre-activations of the three hidden layers), all float64"""
    h, hs, pre = nc.bf16(x).astype(np.float64), [], []
    for k, (w, b) in enumerate(layers(net)):
        hs.append(h)
        a = h @ w.T + b + 0.0                         # (+ 0.0: a sum of zero is +0, as an accumulator that starts at the bias gives it)
        if k == 3:
            return dict(out=a, h=hs, a=pre)
        pre.append(a)
        h = bf16_from_f64(np.tanh(a))


def certify(net, x, ref=None, chunk=32):
    """dict(ok [rows] bool, ratio [rows]: the smallest distance / (MARGIN E) over the row's 768 activations, slack [rows]: the smallest 2^(ACC_BITS - q) / M over the
    row's 772 sums); ok = both above 1"""
    ref = ref or reference(net, x)
    rows = ref["out"].shape[0]
    ratio, slack = np.full(rows, np.inf), np.full(rows, np.inf)
    for (w, b), h in zip(layers(net), ref["h"]):
        M = np.abs(h) @ np.abs(w).T + np.abs(b)
        qw, qh, qb = np.where(w != 0, _q(w), -10000), _q(h), _q(b)
        q = np.empty(M.shape, np.int64)
        for r0 in range(0, rows, chunk):              # q of a product of two odd multiples of powers of two: the sum of theirs
            q[r0:r0 + chunk] = (qh[r0:r0 + chunk, None, :] + qw[None]).max(-1)
        q = np.maximum(q, qb[None])
        with np.errstate(divide="ignore"):
            slack = np.minimum(slack, (np.ldexp(1.0, ACC_BITS - np.maximum(q, -1000)) / M).min(-1))
    for a in ref["a"]:
        ratio = np.minimum(ratio, (midpoint_distance(np.tanh(a)) / (MARGIN * fast_tanh_error(a))).min(-1))
    return dict(ok=(ratio > 1.0) & (slack > 1.0), ratio=ratio, slack=slack)


class Case:
    """A pool of rows of one width: the network, the inputs, their reference and certificate -- computed once, shared, never changed"""

    def __init__(self, D, seed, rows):
        self.D, self.seed = D, seed
        self.net = make_net(D, seed)
        self.x, self.ties = make_input(rows, D, seed)
        self.ref = reference(self.net, self.x)
        self.cert = certify(self.net, self.x, self.ref)
        self.certified = np.flatnonzero(self.cert["ok"])
        for v in (self.x, self.ref["out"], self.cert["ok"], self.cert["ratio"], self.certified):
            v.setflags(write=False)

    @property
    def share(self):
        return self.certified.size / self.x.shape[0]


SEEDS = {8: 1, 16: 1, 24: 1, 32: 1}


@functools.lru_cache(maxsize=None)
def case(D, rows=POOL_ROWS):
    return Case(D, SEEDS[D], rows)


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------------
def compare(loc_scale_dev, c: Case, rows, what=""):
    """The device's loc_scale [len(rows), 4] of the pool rows ``rows`` (all certified) against the reference.  dict(ok, message, bad: the failing pool rows, ...)."""
    rows = np.asarray(rows)
    assert c.cert["ok"][rows].all(), "compare takes certified rows only"
    got = np.ascontiguousarray(np.asarray(loc_scale_dev, np.float32).reshape(rows.size, 4))
    out = c.ref["out"][rows]
    want = out.astype(np.float32)
    assert (want.astype(np.float64) == out).all()      # (a certified row's outputs are fp32 numbers)
    bad = got[:, :2].view(np.uint32) != np.ascontiguousarray(want[:, :2]).view(np.uint32)  # [n, 2]; a NaN differs, -0 differs from +0
    sc = ph.compare_scale(got[:, 2:], out[:, 2:], 0.0)
    bad_scale = np.zeros_like(bad)
    if not sc["ok"]:
        for i in range(rows.size):
            for j in range(2):
                bad_scale[i, j] = not ph.compare_scale(got[i:i + 1, 2 + j], out[i:i + 1, 2 + j], 0.0)["ok"]
    allbad = np.concatenate([bad, bad_scale], 1)
    failing = np.flatnonzero(allbad.any(1))
    r = dict(what=what, rows=int(rows.size), ok=failing.size == 0, bad=rows[failing], loc_wrong=int(bad.sum()), scale_wrong=int(bad_scale.sum()),
             scale_ratio_max=sc["ratio_max"], wrong_per_output=allbad.sum(0).tolist(), message="")
    if failing.size:
        names = ("loc0", "loc1", "scale0", "scale1")
        some = [f"row {i} (pool row {rows[i]}, certificate ratio {c.cert['ratio'][rows[i]]:.2f}, slack {c.cert['slack'][rows[i]]:.3g}): " +
                ", ".join(f"{names[j]} {got[i, j]!r} != {(want[i, j] if j < 2 else ph.scale_of(out[i, j])):.9g}" for j in np.flatnonzero(allbad[i]))
                for i in failing[:12]]
        ratios = c.cert["ratio"][rows[failing]]
        r["message"] = (f"{what}: D = {c.D}, {failing.size} of {rows.size} certified rows differ from the float64 restatement; wrong per output "
                        f"{dict(zip(names, r['wrong_per_output']))}; certificate ratios of the failing rows: min {ratios.min():.2f}, median {np.median(ratios):.2f}, "
                        f"max {ratios.max():.2f} (all near 1: the assumption on fast_tanh; any: structural).  " + "; ".join(some))
    return r
