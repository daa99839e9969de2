"""The observation row against real arithmetic: a float64 restatement of the row from the exported fp32 buffers, and a per-element bound that is a count of
roundings.  numpy only; a helper module like network_check.py / policy_head_check.py (tests/test_observation_check.py runs it on the host, tests/test_gpu_observation.py
on the device's buffers).

Why.  Every buffer a row is assembled from -- BUF_STATE (x, y, psi, speed, steering, vx, vy), BUF_VERTICES, BUF_SHORT_TERM, BUF_DIST_REF / _LEFT / _RIGHT,
BUF_DIST_AGENTS, BUF_NEARING, BUF_CLOSEST, BUF_PATH, BUF_TIMER -- is held to the C oracle to the bit; BUF_OBS alone is held to a flat 1e-5 (about 80 ulp of its O(1)
values), because the kernels deliberately differ from the oracle on every column (rotation form of the ego transform, reciprocal normalisers).  The row is a pure
function of those fp32 numbers, so it can be held to that function evaluated in float64 instead.

``row64``  the row in float64.  The LAYOUT is restated from oracle/sigmaenv_oracle.c::agent_observation (``assemble`` below, the only statement of it in the tests); the
VALUES are real arithmetic on the fp32 inputs widened exactly: cos / sin of the fp32 psi in float64, exact differences, hypot, division by the normaliser formed as the
code forms it ((float)((double)length * 10.0), max_speed, (float)((double)lane_width * 3.0), (float)(2 pi), world_x_dim, world_y_dim), the angle wrap with the float32
constants TWO_PI32, PI32 widened.  No oracle function is called for a value.  The discrete decisions are taken from the exported buffers and exact fp32 comparisons
(observed neighbours: BUF_NEARING; masked: dist >= distance_mask_agents; boundary-point indices: BUF_PATH, BUF_CLOSEST, the map's point counts and the caller's
``fresh`` flags), so they are the same on both sides.
NOT covered: the lanelet-relation mask of the bird view (bird view + is_apply_mask on a map with a lanelet neighbour table).  Its only effect is a 1.0 / 0.0 pattern,
which the existing 1e-5 comparison against the oracle already pins; ``assemble`` raises NotImplementedError for such a configuration.

``bound``  the per-element bound, same shape.  u = 2^-24 is the unit roundoff (one rounding to nearest: relative error <= u; a correctly rounded cos / sin / atan2 the
same); every first-order constant is multiplied by 1.01 for the second-order terms.  "val" is the float64 value of the element, n its normaliser.

  form="kernel" -- what observe_tile_default / observe_tile_variant (sigmarl_amd/csrc/sigmaenv.hip) compute.  No FMA contraction (-ffp-contract=off); an FMA would only
  remove roundings.

  scaled scalar  x * r, r = fl(1 / n) (distances, bird-view positions / vertices / velocities, length * r_da; the full observation divides, x / n: one rounding):
      r = (1 / n)(1 + e1), fl(x r) = x r (1 + e2):  2 u |val|.  The minimum over the five boundary distances is a selection: exact.
  own speed  norm2(vx, vy) * r_v, norm2 = sqrtf(fmaf(vy, vy, fl(vx vx))): the radicand is a sum of non-negative terms with two roundings, 2 u relative, halved by the
      root: u; the root's rounding u; the normalisation 2 u:  4 u |val|.
  ego-frame point  ((dx c + dy s) r_pos, (dy c - dx s) r_pos), dx = fl(tx - px), c = fl(cos psi), s = fl(sin psi) (the stored pair is the correctly rounded cos / sin
      of the stored psi: cr_sincos / cr_cos / cr_sin of the value written to BUF_STATE).  Per product: the difference's rounding u, the factor's half ulp u, the
      product's rounding u -> 3 u |term|; both terms: 3 u M with M = (|dx c| + |dy s|) / n (second component: (|dy c| + |dx s|) / n).  The sum's rounding u |val| and
      the normalisation 2 u |val|:  3 u M + 3 u |val|  (<= 6 u M, since |val| <= M).
  relative velocity  ((va cr) r_v, (va sr) r_v), va = norm2(vx_j, vy_j) (2 u, as above), cr = fl(fl(cj ci) + fl(sj si)): per product two half ulps and a rounding,
      3 u |term| -> 3 u S, S = |cj ci| + |sj si|; the sum u |cr|.  Then va's 2 u, the product u, the normalisation 2 u on |val| = (va / n) |cr|:
      (va / n)(3 u S + 6 u |cr|).  sr = fl(fl(sj ci) - fl(cj si)) the same with S = |sj ci| + |cj si| and |sr|.
  angle  wrap(a) * r_rot (own / neighbours' steering, bird-view rotation; relative rotation: a = fl(psi_j - psi_i)), wrap: m = fmodf(a, TWO_PI32) is exact; a negative m
      gets + TWO_PI32, ONE rounded addition, error u |m + TWO_PI32|; the following "- TWO_PI32 if > PI32" has its operand in [TWO_PI32 / 2, TWO_PI32]: exact
      (Sterbenz), as is the first addition when m <= -PI32.  So of the at most two additions of 2 pi at most one rounds.  The normalisation 2 u |val|:
      u |m + TWO_PI32| / n_rot (only for m < 0) + 2 u |val|;  the relative rotation adds |fl(psi_j - psi_i) - (psi_j - psi_i)| / n_rot for its rounded difference (the
      float64 row takes the exact difference; the rounding error of one IEEE subtraction of known operands, <= u |psi_j - psi_i|, is computed rather than bounded).
      Angles are compared MODULO 1: a value next to the wrap may land on either side (the rounded addition or difference decides "> PI32" the other way); then the
      two sides differ by TWO_PI32 * r_rot = 1 + at most 2 u (reciprocal and product), and 2 u is added where the comparison wrapped.
  exact  masked columns (1.0 / 0.0), opponent placeholders (0), the full observation's zeroed distance block, and every value whose bound is zero (coincident agents:
      dx = dy = 0; zero speed; zero steering): compared with ==.
  sensor noise (obs_noise_level > 0; steps and resets only, salt 0): element k of agent i of env b gets level * draw, draw = (rng_u32(seed, counter, env_index_base + b,
      i, 9000 + k) >> 8) * 2^-24 (exact in fp32), counter = episodes_reset * 65537 + timer.step as obs_noise (sigmaenv_device.h) forms it.  The row adds it in float64;
      the bound adds the product's rounding u |level draw| and the sum's u |val + level draw|.
  underflow floor: a product whose result is below the smallest normal number loses up to 2^-150 absolutely.  Scaled scalar / angle: one such product.  Ego point:
      two products seen through 1 / n, and the normalisation: 2 * 2^-150 / n + 2^-150.  norm2: fl(vx vx) and the fma can each lose 2^-150 of the RADICAND, which the
      root turns into at most sqrt(2 * 2^-150) = 2^-74.5 of va: speed 2^-74.5 / n + 2^-150; relative velocity the same plus the two products of cr through va / n, the
      product va cr through 1 / n and the normalisation.  A floor is only added where the value is not exactly zero by construction (see "exact").

  form="reference" -- the oracle's own formulation (the reference's), held on the host only; it needs a wider, differently shaped bound and the kernel is NOT held to it.
  ego-frame point  ab = norm2(dx, dy), rr = fl(fl(atan2(dy, dx)) - psi), (fl(cos rr) ab / n, fl(sin rr) ab / n).  The angle carries: the rounded dx, dy (they turn the
      direction by at most 2 u |dx dy| / (dx^2 + dy^2) <= u), the correctly rounded atan2 u |theta| (|theta| <= pi), the rounded difference u |theta - psi|:
      delta = u (1 + |theta| + |theta - psi|), seen through the OTHER component (d/d rr of ab cos rr is -ab sin rr).  The magnitude: dx, dy u, norm2 2 u, cos / sin u, product
      u, division u: 6 u |val|.  Bound: delta |other| + 6 u |val|, floor 2^-74.5 / n + 2 * 2^-150.
  relative velocity  va cos(wrap(fl(psi_j - psi_i))) / n: the angle carries u |a| for the difference, the one rounded addition of the wrap u * 2 pi, and k |TWO_PI32 - 2 pi|,
      k = floor(|a| / 2 pi) + 1, because the wrap removes multiples of the float32 2 pi where the float64 row takes the real cos / sin of the difference; seen through the other
      component.  The magnitude: va 2 u, cos u, product u, division u: 5 u |val|.
  everything else divides where the kernel multiplies by the reciprocal: one rounding less, the kernel's bound holds.

``compare``  the worst error / bound per column class and ``ok`` (every ratio <= 1, and error == 0 wherever the bound is 0).  No element is left out.
"""
from __future__ import annotations

import numpy as np

from policy_head_check import rng_u32
from sigmarl_amd import capi

U = 2.0 ** -24
NOISE_DRAW = 9000  # sigmaenv_dist.h DRAW_OBS_NOISE: element k of a row draws NOISE_DRAW + k
C1 = 1.01
TINY = 2.0 ** -150
ROOT_TINY = 2.0 ** -74.5
TWO_PI32 = float(np.float32(6.283185307179586))
PI32 = float(np.float32(3.141592653589793))
TWO_PI_GAP = abs(TWO_PI32 - 2.0 * np.pi)

EXACT, SCALED, SPEED, EGO, RELVEL, ANGLE = range(6)
CLASSES = ("exact", "scaled", "speed", "ego", "relvel", "angle")

INPUT_BUFS = (capi.BUF_STATE, capi.BUF_PREV_POS, capi.BUF_VERTICES, capi.BUF_SHORT_TERM, capi.BUF_DIST_REF, capi.BUF_DIST_LEFT, capi.BUF_DIST_RIGHT,
              capi.BUF_DIST_AGENTS, capi.BUF_NEARING, capi.BUF_CLOSEST, capi.BUF_PATH, capi.BUF_TIMER)


def read_bufs(env, fresh=None):
    """The input buffers of the row (and BUF_OBS itself) of an env with ``get(which)`` -- OracleEnv, NumpyAdapter.  ``fresh`` [B, N] bool: agents (re)placed and not
    stepped since (the boundary-point rows index differently then; not an exported buffer: the caller knows it, see FreshTracker)."""
    b = {w: env.get(w) for w in INPUT_BUFS + (capi.BUF_OBS,)}
    if fresh is not None:
        b["fresh"] = np.array(fresh, bool)
    return b


class FreshTracker:
    """Which agents are fresh, from the calls made: a step clears every flag; auto_reset re-places every agent of a done env and, in an unfinished env, the agents with
    a reset request (BUF_COL_FLAGS[..., 3]) -- call ``before_auto_reset`` with the env BEFORE the reset."""

    def __init__(self, B, N):
        self.fresh = np.zeros((B, N), bool)

    def step(self):
        self.fresh[:] = False

    def before_auto_reset(self, env):
        done = env.get(capi.BUF_DONE).astype(bool)
        req = env.get(capi.BUF_COL_FLAGS)[..., 3].astype(bool)
        self.fresh |= done[:, None] | req


def normalisers(cfg):
    """The normalisers as the code forms them, widened to float64"""
    f32 = np.float32
    return dict(pos=float(f32(float(f32(cfg.length)) * 10.0)), v=float(f32(cfg.max_speed)), dl=float(f32(float(f32(cfg.lane_width)) * 3.0)),
                rot=float(f32(2.0 * 3.141592653589793)), da=float(f32(float(f32(cfg.length)) * 10.0)), wx=float(f32(cfg.world_x_dim)), wy=float(f32(cfg.world_y_dim)))


# ---- the arithmetic: float64 values with their bounds --------------------------------------------------------------------------------------------------------------
class Real64:
    """Every method returns columns ``(value, bound, class)`` (float64 [B, N] arrays and a class id) for fp32 inputs; ``form`` chooses the bound."""

    def __init__(self, cfg, form="kernel"):
        assert form in ("kernel", "reference")
        self.form = form
        self.n = normalisers(cfg)

    @staticmethod
    def w(x):
        x = np.asarray(x)
        assert x.dtype == np.float32, x.dtype  # inputs are the fp32 words of the buffers, widened exactly
        return x.astype(np.float64)

    def const(self, value, like):
        return np.full(like.shape, float(value)), np.zeros(like.shape), EXACT

    def scaled(self, x, which):
        n = self.n[which]
        val = self.w(x) / n
        return val, np.where(val != 0, 2 * U * C1 * np.abs(val) + TINY, 0.0), SCALED

    def scaled_const(self, x, which, like):
        return self.scaled(np.full(like.shape, np.float32(x), np.float32), which)

    def speed(self, vx, vy):
        n = self.n["v"]
        val = np.hypot(self.w(vx), self.w(vy)) / n
        return val, np.where(val != 0, 4 * U * C1 * val + ROOT_TINY / n + TINY, 0.0), SPEED

    def ego(self, tx, ty, px, py, psi):
        n = self.n["pos"]
        dx, dy, p = self.w(tx) - self.w(px), self.w(ty) - self.w(py), self.w(psi)
        c, s = np.cos(p), np.sin(p)
        vx, vy = (dx * c + dy * s) / n, (dy * c - dx * s) / n
        mx, my = (np.abs(dx * c) + np.abs(dy * s)) / n, (np.abs(dy * c) + np.abs(dx * s)) / n
        if self.form == "kernel":
            floor = 2 * TINY / n + TINY
            bx = np.where(mx != 0, (3 * mx + 3 * np.abs(vx)) * U * C1 + floor, 0.0)
            by = np.where(my != 0, (3 * my + 3 * np.abs(vy)) * U * C1 + floor, 0.0)
        else:
            theta = np.arctan2(dy, dx)
            delta = U * (1.0 + np.abs(theta) + np.abs(theta - p))
            floor = ROOT_TINY / n + 2 * TINY
            some = (dx != 0) | (dy != 0)
            bx = np.where(some, (delta * np.abs(vy) + 6 * U * np.abs(vx)) * C1 + floor, 0.0)
            by = np.where(some, (delta * np.abs(vx) + 6 * U * np.abs(vy)) * C1 + floor, 0.0)
        return (vx, bx, EGO), (vy, by, EGO)

    def relvel(self, vx, vy, psi_j, psi_i):
        n = self.n["v"]
        va = np.hypot(self.w(vx), self.w(vy)) / n
        pj, pi = self.w(psi_j), self.w(psi_i)
        a = pj - pi
        cr, sr = np.cos(a), np.sin(a)
        if self.form == "kernel":
            cj, sj, ci, si = np.cos(pj), np.sin(pj), np.cos(pi), np.sin(pi)
            floor = ROOT_TINY / n + va * 2 * TINY + TINY / n + TINY
            bc = va * (3 * (np.abs(cj * ci) + np.abs(sj * si)) + 6 * np.abs(cr)) * U * C1 + floor
            bs = va * (3 * (np.abs(sj * ci) + np.abs(cj * si)) + 6 * np.abs(sr)) * U * C1 + floor
        else:
            delta = U * np.abs(a) + U * TWO_PI32 + (np.floor(np.abs(a) / (2 * np.pi)) + 1.0) * TWO_PI_GAP
            floor = ROOT_TINY / n + 2 * TINY
            bc = va * (delta * np.abs(sr) + 5 * U * np.abs(cr)) * C1 + floor
            bs = va * (delta * np.abs(cr) + 5 * U * np.abs(sr)) * C1 + floor
        return (va * cr, np.where(va != 0, bc, 0.0), RELVEL), (va * sr, np.where(va != 0, bs, 0.0), RELVEL)

    def _wrap(self, a, extra):
        n = self.n["rot"]
        m = np.fmod(a, TWO_PI32)
        neg = m < 0
        m = np.where(neg, m + TWO_PI32, m)
        err = np.where(neg, U * np.abs(m), 0.0) + extra
        m = np.where(m > PI32, m - TWO_PI32, m)
        val = m / n
        return val, np.where((val != 0) | (err != 0), (err / n + 2 * U * np.abs(val)) * C1 + TINY, 0.0), ANGLE

    def angle(self, a):
        return self._wrap(self.w(a), 0.0)

    def relangle(self, psi_j, psi_i):
        a = self.w(psi_j) - self.w(psi_i)
        return self._wrap(a, np.abs((np.asarray(psi_j) - np.asarray(psi_i)).astype(np.float64) - a))


# ---- the layout: oracle/sigmaenv_oracle.c::agent_observation ----------------------------------------------------------------------------------------------------------
def _gather(x, j):
    """x [B, N, ...] at agent j [B, N] of the same env"""
    return x[np.arange(x.shape[0])[:, None], j]


def boundary_point_ids(cfg, mp, bufs):
    """[B, N, 2, 5] indices into the padded boundary polylines (left, right) of the agent's path: k + closest + shift (1 for a fresh agent, else -2), the loop rule
    with the centre line's point count, a negative index from the end of the padded table"""
    path = bufs[capi.BUF_PATH][..., 0].astype(np.int64)
    cp = bufs[capi.BUF_CLOSEST][..., 1:3].astype(np.int64)
    if "fresh" not in bufs:
        raise ValueError("the boundary-point rows need bufs['fresh'] (see read_bufs)")
    shift = np.where(bufs["fresh"], 1, -2)
    n = mp.n_center[path].astype(np.int64)[..., None, None]
    loop = mp.is_loop[path].astype(bool)[..., None, None]
    idx = np.arange(5)[None, None, None, :] + cp[..., None] + shift[..., None, None]
    idx = np.where(loop & (idx >= n - 1), (idx + 1) % n, idx)
    return np.where(idx < 0, idx + mp.stride, idx), path


def assemble(cfg, mp, bufs, ar):
    """The columns of the row [B, N, D] in order, each a ``(value, bound, class)`` of ``ar``'s arithmetic (Real64 above; the float32 twin of the host test)."""
    F, N, K = int(cfg.obs_flags), int(cfg.n_agents), int(cfg.n_nearing)
    NS = int(getattr(cfg, "n_points_short_term", 0) or capi.N_SHORT_TERM)
    bird, full = bool(F & capi.OBS_BIRD_VIEW), bool(F & capi.OBS_FULL)
    mask_on = bool(cfg.is_apply_mask)
    if bird and not full and mask_on and mp.lanelet_tables() is not None:
        raise NotImplementedError("the lanelet-relation mask of the bird view is out of this module's scope (module docstring)")
    st = bufs[capi.BUF_STATE]
    vert, short = bufs[capi.BUF_VERTICES], bufs[capi.BUF_SHORT_TERM]
    dist = bufs[capi.BUF_DIST_AGENTS]
    px, py, psi = st[..., 0], st[..., 1], st[..., 2]
    like = px
    cols = []

    def point(tx, ty):
        if bird:
            return [ar.scaled(tx, "wx"), ar.scaled(ty, "wy")]
        return list(ar.ego(tx, ty, px, py, psi))

    def masked_cols(cs, mk, value):
        if mk is None:
            return cs
        out = []
        for v, b, c in cs:
            cv, cb, _ = ar.const(value, like)
            out.append((np.where(mk, cv, v), np.where(mk, cb, b), np.where(mk, EXACT, c)))
        return out

    # [own]
    if bird:
        cols += [ar.scaled(px, "wx"), ar.scaled(py, "wy"), ar.angle(psi), ar.scaled(st[..., 5], "v"), ar.scaled(st[..., 6], "v")]
    else:
        cols.append(ar.speed(st[..., 5], st[..., 6]))
    if F & capi.OBS_STEERING:
        cols.append(ar.angle(st[..., 4]))
    for k in range(NS):
        cols += point(short[..., k, 0], short[..., k, 1])
    if not (F & capi.OBS_NO_DIST_CENTER):
        cols.append(ar.scaled(bufs[capi.BUF_DIST_REF], "dl"))
    if F & capi.OBS_BOUNDARY_POINTS:
        idx, path = boundary_point_ids(cfg, mp, bufs)
        for side, poly in enumerate((mp.left, mp.right)):
            for k in range(5):
                pt = poly[path, idx[..., side, k]]
                cols += point(np.ascontiguousarray(pt[..., 0]), np.ascontiguousarray(pt[..., 1]))
    else:
        cols.append(ar.scaled(bufs[capi.BUF_DIST_LEFT].min(axis=-1), "dl"))
        cols.append(ar.scaled(bufs[capi.BUF_DIST_RIGHT].min(axis=-1), "dl"))
    # [others]
    if full:
        cols += _full_others(cfg, bufs, ar, NS)
    else:
        near = bufs[capi.BUF_NEARING].astype(np.int64)
        for k in range(K):
            j = near[..., k]
            sj = _gather(st, j)
            dj = np.take_along_axis(dist, j[..., None], axis=-1)[..., 0]
            mk = (dj >= np.float32(cfg.distance_mask_agents)) if mask_on else None
            if not (F & capi.OBS_NO_VERTICES):
                vj = _gather(vert, j)
                for q in range(4):
                    cols += masked_cols(point(vj[..., q, 0], vj[..., q, 1]), mk, 1.0)
            else:
                cols += masked_cols(point(sj[..., 0], sj[..., 1]), mk, 1.0)
                cols += masked_cols([ar.angle(sj[..., 2]) if bird else ar.relangle(sj[..., 2], psi)], mk, 0.0)
                cols += [ar.scaled_const(cfg.length, "da", like), ar.scaled_const(cfg.width, "da", like)]
            if bird:
                cols += masked_cols([ar.scaled(sj[..., 5], "v"), ar.scaled(sj[..., 6], "v")], mk, 0.0)
            else:
                cols += masked_cols(list(ar.relvel(sj[..., 5], sj[..., 6], sj[..., 2], psi)), mk, 0.0)
            if F & capi.OBS_STEERING:
                cols += masked_cols([ar.angle(sj[..., 4])], mk, 0.0)
            if not (F & capi.OBS_NO_DIST_AGENTS):
                cols += masked_cols([ar.scaled(dj, "dl")], mk, 1.0)
            if F & capi.OBS_REF_OTHERS:
                shj = _gather(short, j)
                for q in range(NS):
                    cols += masked_cols(point(shj[..., q, 0], shj[..., q, 1]), mk, 1.0)
    if F & capi.OBS_OPPONENT_PAD:
        cols += [ar.const(0.0, like) for _ in range(2 * K)]
    return cols


def _full_others(cfg, bufs, ar, NS):
    """The full observation (bird view): every feature holds ALL agents in index order, its flat per-env array [N * w] is cut into K equal chunks, and the row takes
    chunk 0 of every feature, then chunk 1, ...; the same for every observing agent.  The distance block is zero."""
    F, N, K = int(cfg.obs_flags), int(cfg.n_agents), int(cfg.n_nearing)
    st = bufs[capi.BUF_STATE]
    B = st.shape[0]
    feats = []  # per feature: list of w columns [B, N] (agent j's q-th value)
    if not (F & capi.OBS_NO_VERTICES):
        v = bufs[capi.BUF_VERTICES]
        feats.append([ar.scaled(v[..., q // 2, q % 2], "wy" if q & 1 else "wx") for q in range(8)])
    else:
        feats.append([ar.scaled(st[..., 0], "wx"), ar.scaled(st[..., 1], "wy")])
        feats.append([ar.angle(st[..., 2])])
        feats.append([ar.scaled_const(cfg.length, "da", st[..., 0])])
        feats.append([ar.scaled_const(cfg.width, "da", st[..., 0])])
    feats.append([ar.scaled(st[..., 5], "v"), ar.scaled(st[..., 6], "v")])
    if F & capi.OBS_STEERING:
        feats.append([ar.angle(st[..., 4])])
    if not (F & capi.OBS_NO_DIST_AGENTS):
        feats.append([ar.const(0.0, st[..., 0]) for _ in range(N)])
    if F & capi.OBS_REF_OTHERS:
        sh = bufs[capi.BUF_SHORT_TERM]
        feats.append([ar.scaled(sh[..., q // 2, q % 2], "wy" if q & 1 else "wx") for q in range(2 * NS)])
    chunks = []
    for f in feats:
        w = len(f)
        assert (N * w) % K == 0, "the reference's reshape refuses this shape"
        parts = []
        for part in range(3):  # value, bound, class
            a = np.stack([np.broadcast_to(np.asarray(c[part]), (B, N)) for c in f], axis=-1)   # [B, N, w]
            parts.append(a.reshape(B, K, N * w // K))
        chunks.append(parts)
    flat = [np.concatenate([c[part] for c in chunks], axis=-1).reshape(B, -1) for part in range(3)]   # [B, W_oth]
    return [tuple(np.broadcast_to(flat[part][:, None, q], (B, N)) for part in range(3)) for q in range(flat[0].shape[1])]


def noise_draws(cfg, bufs, D):
    """level * draw [B, N, D] in float64 and the draw's magnitude, or None with the noise off"""
    level = np.float32(cfg.obs_noise_level)
    if not level > 0:
        return None
    tim = bufs[capi.BUF_TIMER].astype(np.int64)
    B, N = bufs[capi.BUF_STATE].shape[:2]
    seed = (int(cfg.obs_noise_seed_hi) << 32) | int(cfg.obs_noise_seed_lo)
    counter = ((tim[:, 3] & 0xFFFFFFFF) * 65537 + (tim[:, 0] & 0xFFFFFFFF)).astype(np.uint64)
    env = (int(cfg.env_index_base) + np.arange(B)).astype(np.uint32)
    h = rng_u32(seed, counter[:, None, None], env[:, None, None], np.arange(N, dtype=np.uint32)[None, :, None], (NOISE_DRAW + np.arange(D)).astype(np.uint32)[None, None, :])
    draw = (np.asarray(h, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return float(level) * draw


def _stack(cols, shape):
    val = np.stack([np.broadcast_to(np.asarray(c[0], np.float64), shape) for c in cols], axis=-1)
    bnd = np.stack([np.broadcast_to(np.asarray(c[1], np.float64), shape) for c in cols], axis=-1)
    cls = np.stack([np.broadcast_to(np.asarray(c[2], np.int8), shape) for c in cols], axis=-1)
    return val, bnd, cls


def _row_bound_class(cfg, mp, bufs, form):
    cols = assemble(cfg, mp, bufs, Real64(cfg, form))
    val, bnd, cls = _stack(cols, bufs[capi.BUF_STATE].shape[:2])
    nz = noise_draws(cfg, bufs, val.shape[-1])
    if nz is not None:
        bnd = bnd + (U * np.abs(nz) + U * np.abs(val + nz)) * C1 + np.where(nz != 0, TINY, 0.0)
        val = val + nz
    return val, bnd, cls


def row64(cfg, mp, bufs):
    """The observation rows [B, N, D] in float64"""
    return _row_bound_class(cfg, mp, bufs, "kernel")[0]


def bound(cfg, mp, bufs, form="kernel"):
    """The per-element bound [B, N, D] (module docstring)"""
    return _row_bound_class(cfg, mp, bufs, form)[1]


def compare(got, cfg, mp, bufs, form="kernel"):
    """``got`` (fp32 [B, N, D]) against row64 within bound: dict(ok, worst = {class: error / bound}, count = {class: elements}, excluded = 0, where = the worst
    element's (class, index, got, want, bound)).  An element whose bound is 0 must be equal; the angle class is compared modulo 1."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    want, bnd, cls = _row_bound_class(cfg, mp, bufs, form)
    assert got.shape == want.shape, (got.shape, want.shape)
    g = got.astype(np.float64)
    err = np.abs(g - want)
    circ = np.minimum(np.abs(g - want - 1.0), np.abs(g - want + 1.0))
    wrapped = (cls == ANGLE) & (circ < err)
    err = np.where(wrapped, circ, err)
    bnd = np.where(wrapped, bnd + 2 * U * C1, bnd)
    finite = np.isfinite(g) & np.isfinite(want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(finite, ratio, np.inf)
    worst, count = {}, {}
    for c, name in enumerate(CLASSES):
        m = cls == c
        count[name] = int(m.sum())
        worst[name] = float(ratio[m].max()) if count[name] else 0.0
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert sum(count.values()) == got.size  # no element is left out
    return dict(ok=bool((ratio <= 1.0).all()), worst=worst, count=count, excluded=0,
                where=(CLASSES[int(cls[k])], tuple(int(x) for x in k), float(g[k]), float(want[k]), float(bnd[k])))


def report(res):
    return "  ".join(f"{name} {res['worst'][name]:.3f} ({res['count'][name]})" for name in CLASSES if res["count"][name]) + f"  worst at {res['where']}"


# ---- injected edge states (reset + observe), shared by the host and the GPU tests --------------------------------------------------------------------------------------
EDGE_ENVS = ("coincident", "outside", "large_psi", "near_pi", "zero_speed", "at_mask")


def injected_edge_states(cfg, mp, path=3):
    """(env_idx, agent_idx, path_ids [n, 4], state8 [n, 8]) for len(EDGE_ENVS) envs of 6 agents standing on centre-line points of ``path``, one edge per env:
    coincident agents (dx = dy = 0: exact zeros); an agent at (9, -3), outside the world; |psi| around 100 rad, one of them against psi = 0 (the difference is exact,
    only the wrap's own roundings remain); psi_j - psi_i within 1e-6 of +-pi on both sides (the circular comparison); zero speed; a neighbour whose centre distance is
    EXACTLY distance_mask_agents (x_i = d, x_j = 2 d, same y: fl(2 d - d) = d and sqrtf(d * d) = d), and one an ulp nearer."""
    B, N = len(EDGE_ENVS), 6
    assert cfg.n_envs == B and cfg.n_agents == N
    c = mp.center[path]
    st = np.zeros((B, N, 8), np.float32)
    ids = np.zeros((B, N, 4), np.int32)
    ids[..., 0] = path
    ids[..., 2] = path
    for i in range(N):
        k = 5 + 9 * i
        st[:, i, 0:2] = c[k]
        st[:, i, 2] = mp.yaw[path][k]
    st[..., 3] = 0.4
    st[..., 4] = np.float32([0.0, 0.1, -0.2, 0.0, 0.3, -0.05])
    e = EDGE_ENVS.index
    st[e("coincident"), 2, 0:3] = st[e("coincident"), 3, 0:3]
    st[e("outside"), 4, 0:2] = np.float32([9.0, -3.0])
    st[e("large_psi"), :, 2] = np.float32([0.0, 100.0, -100.0, 99.5, -101.25, 3.0])
    pi32 = np.float32(np.pi)
    st[e("near_pi"), :, 2] = np.float32([0.3, 0.3, 0.3, 0.3, 0.3, 0.3]) + np.float32([0.0, 1.0, -1.0, 1.0, -1.0, 0.0]) * pi32 + np.float32([0.0, 5e-7, 5e-7, -5e-7, -5e-7, 0.0])
    st[e("near_pi"), 1:5, 0:2] = st[e("near_pi"), 0, 0:2] + np.float32([[0.3, 0.0], [0.0, 0.3], [-0.3, 0.0], [0.0, -0.3]])   # the four are the nearest of agent 0
    st[e("zero_speed"), :, 3] = 0.0
    d = np.float32(cfg.distance_mask_agents)
    y = st[e("at_mask"), 0, 1]
    st[e("at_mask"), 0, 0:2] = (d, y)
    st[e("at_mask"), 1, 0:2] = (np.float32(2.0) * d, y)
    st[e("at_mask"), 2, 0:2] = (d - np.nextafter(d, np.float32(0.0)), y)   # x_2 = ulp(d): x_0 - x_2 is the float below d, exactly
    st[..., 5] = st[..., 3] * np.cos(st[..., 2].astype(np.float64)).astype(np.float32)
    st[..., 6] = st[..., 3] * np.sin(st[..., 2].astype(np.float64)).astype(np.float32)
    return np.repeat(np.arange(B), N), np.tile(np.arange(N), B), ids.reshape(-1, 4), st.reshape(-1, 8)
