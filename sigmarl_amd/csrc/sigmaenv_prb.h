// sigmaenv_prb.h -- the arithmetic of the prioritized replay buffer on the device, stated ONCE: the sum / min hierarchy over the stored priorities, the descent that
// turns a mass into a leaf index, and the element formulas of the TD-error refresh -- torchrl's TensorDictPrioritizedReplayBuffer(alpha, beta, priority_key =
// "td_error") as sigmarl/mappo_cavs.py:321-332 builds it, sample() as :397-407 calls it and _update_priorities_after_training (:431-456) with compute_td_error
// (sigmarl/helper_training.py:1029-1068).  torchrl is third-party and absent: restated from its published behaviour.  The kernels of sigmaenv_prb.inc run these
// functions on the device; a host program runs them on the host (tests/test_prb_check.py holds them bit for bit to the float32 twin of tests/prb_check.py and,
// within derived bounds, to float64).
//
// Plain C++: no HIP include and, of the library, only sigmaenv_dist.h (the generator's draw table and uniforms, plain C++ as well).  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.  Every operator below is ONE IEEE fp32 operation in the order written (-ffp-contract=off; `/` is the
// correctly rounded one; fp32 denormals are kept).
//
// The hierarchy.  F = the capacity, len <= F the filled length.  Level 0 holds the F leaves q[f]; level k + 1 holds one (sum, min) per PRB_FAN = 256 consecutive
// entries of level k: n_0 = F, n_{k+1} = ceil(n_k / 256), until a level has <= 256 entries (the top: 3 levels at F = 524288, at most PRB_MAX_LEVELS = 4).  A leaf
// at f >= len and an entry past n_k count as 0 for a sum and +inf for a min.  One NODE = 256 consecutive entries e_0 .. e_255 of one level, given to one wavefront:
//   lane l (0 .. 63)  takes e_{4l} .. e_{4l+3}:  c_0 = e_{4l};  c_1 = c_0 + e_{4l+1};  c_2 = c_1 + e_{4l+2};  c_3 = c_2 + e_{4l+3}                      prb_lane_chain
//   wavefront         the inclusive scan I of the lane sums c_3:  I_l = c_3 of lane l;  then for d = 1, 2, 4, 8, 16, 32, all lanes at once:
//                     I_l = I_l + I_{l-d} for the lanes l >= d;   E_l = I_{l-1}, E_0 = 0
//   prefixes          S_{4l+i} = E_l + c_i for i = 0, 1, 2;   S_{4l+3} = I_l;   S_{-1} = 0                                                                 prb_node_prefix
//   the node's sum    S_255 = I_63
//   the node's min    lane l: m = min(min(min(e_{4l}, e_{4l+1}), e_{4l+2}), e_{4l+3}); the butterfly m = min(m, m[lane ^ s]), s = 32, 16, 8, 4, 2, 1; lane 0's value,
//                     with min(a, b) = b < a ? b : a (a NaN is kept or dropped by that rule: the bits are still a function of the data alone)                prb_node_min
// total and q_min are the sum and the min of the ONE node over the top level.  No atomics; the shape of every sum is a function of F alone.
//
// The descent: a pure function of (levels, len, mass).  cnt_k = ceil(len / 256^k) entries of level k lie below len.  r = mass, node = 0; for k = top .. 0:
//   the node's entries e_j = level_k[256 node + j] (0 where 256 node + j >= cnt_k), its prefixes S_j as above;
//   last = min(255, cnt_k - 1 - 256 node);   j = the smallest j with r < S_j;  if no j qualifies (fp32 rounding between a parent's stored sum and its children's
//   prefixes, u = 1.0, a NaN): j = last;  j = min(j, last);   r = r - S_{j-1};   node = 256 node + j                                                       prb_pick, prb_descend
// 256 node < cnt_k holds at every level by induction (len >= 1), so the leaf index lies in [0, len) whatever the data: it is never formed from arithmetic on mass.
//
// The elements.
//   u        = rng_uniform_mid of the generator's word k, draw DRAW_REPLAY keyed (seed, counter, env = slot m, agent = 0) (sigmaenv_dist.h);  mass = u * total   prb_uniform
//   priority = powf(td + eps, alpha)                       extend and refresh;  powf: the device's is OCML's __ocml_pow_f32, a host's its libm's           prb_priority
//   weight   = powf(q[index] / q_min, -beta)               (-beta: fl(beta) negated);  the same powf                                                      prb_weight
//   x        = (sum over i = 0 .. N - 1, in that order, of |(r_i + (td_gamma * v_next) * nd) - v|) / N,  nd = 1 - done      (sigmaenv_gae's td_priority)   prb_x
//   td       = clamp(((x - min) / max(max - min, 1e-3)) * 10, 1e-3, 10),  min / max over the minibatch's slots (exact in any order)                       prb_norm
// The two powf are the only operations a host cannot reproduce to the bit.
#ifndef SIGMAENV_PRB_H
#define SIGMAENV_PRB_H
#include <math.h>
#include <stdint.h>

#include "sigmaenv_dist.h"  // the generator's draw table and its uniforms: as stand-alone as this header

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define PRB_FAN 256        /* entries of one node */
#define PRB_MAX_LEVELS 4   /* levels, the leaves included: capacity <= 2^30 */
#define PRB_MAX_CAPACITY (1 << 30)
#define PRB_DRAW DRAW_REPLAY /* the sampler's draw id */

// the sums as the descent reads them: sum[0] = the leaves, sum[k] = level k (what lies below len at a level follows from len: prb_cnt)
struct PrbLevels {
  const float* sum[PRB_MAX_LEVELS];
  int n_levels;
};

// n_0 = capacity, n_{k+1} = ceil(n_k / 256) until <= 256: returns the number of levels
static inline int prb_level_sizes(int64_t capacity, int* n) {
  int L = 0;
  int64_t m = capacity;
  n[L++] = (int)m;
  while (m > PRB_FAN && L < PRB_MAX_LEVELS) {
    m = (m + PRB_FAN - 1) / PRB_FAN;
    n[L++] = (int)m;
  }
  return L;
}
// entries of level k that lie below len: ceil(len / 256^k)
SIGMA_HD int prb_cnt(int len, int k) {
  int64_t c = len;
  for (int i = 0; i < k; ++i) c = (c + PRB_FAN - 1) / PRB_FAN;
  return (int)c;
}
SIGMA_HD float prb_min(float a, float b) { return b < a ? b : a; }
// lane l's chain over its four entries
SIGMA_HD void prb_lane_chain(float e0, float e1, float e2, float e3, float* c) {
  c[0] = e0;
  c[1] = c[0] + e1;
  c[2] = c[1] + e2;
  c[3] = c[2] + e3;
}
SIGMA_HD float prb_lane_min(float e0, float e1, float e2, float e3) { return prb_min(prb_min(prb_min(e0, e1), e2), e3); }
// the 256 entries of a node -> its 256 inclusive prefixes (the kernels do the scan with cross-lane moves: prb::node_scan, the same additions)
static inline void prb_node_prefix(const float* e, float* S) {
  float c[64][4], I[64], J[64];
  for (int l = 0; l < 64; ++l) {
    prb_lane_chain(e[4 * l], e[4 * l + 1], e[4 * l + 2], e[4 * l + 3], c[l]);
    I[l] = c[l][3];
  }
  for (int d = 1; d < 64; d <<= 1) {
    for (int l = 0; l < 64; ++l) J[l] = l >= d ? I[l] + I[l - d] : I[l];
    for (int l = 0; l < 64; ++l) I[l] = J[l];
  }
  for (int l = 0; l < 64; ++l) {
    const float E = l ? I[l - 1] : 0.0f;
    S[4 * l] = E + c[l][0];
    S[4 * l + 1] = E + c[l][1];
    S[4 * l + 2] = E + c[l][2];
    S[4 * l + 3] = I[l];
  }
}
static inline float prb_node_min(const float* e) {
  float m[64], u[64];
  for (int l = 0; l < 64; ++l) m[l] = prb_lane_min(e[4 * l], e[4 * l + 1], e[4 * l + 2], e[4 * l + 3]);
  for (int s = 32; s > 0; s >>= 1) {
    for (int l = 0; l < 64; ++l) u[l] = prb_min(m[l], m[l ^ s]);
    for (int l = 0; l < 64; ++l) m[l] = u[l];
  }
  return m[0];
}
// node `node` of a level of which `valid` entries count: its sum and min
static inline void prb_node(const float* level, int valid, int node, float* sum, float* mn) {
  float es[PRB_FAN], em[PRB_FAN], S[PRB_FAN];
  for (int j = 0; j < PRB_FAN; ++j) {
    const int64_t p = (int64_t)node * PRB_FAN + j;
    es[j] = p < valid ? level[p] : 0.0f;
    em[j] = p < valid ? level[p] : INFINITY;
  }
  prb_node_prefix(es, S);
  *sum = S[PRB_FAN - 1];
  *mn = prb_node_min(em);
}
// the smallest j with r < S_j, else `last`; never above `last`
static inline int prb_pick(const float* S, float r, int last) {
  int j = last;
  for (int i = 0; i < PRB_FAN; ++i)
    if (r < S[i]) { j = i; break; }
  return j < last ? j : last;
}
static inline int prb_descend(const PrbLevels& L, int len, float mass) {
  float r = mass;
  int node = 0;
  for (int k = L.n_levels - 1; k >= 0; --k) {
    const int cnt = prb_cnt(len, k);
    float e[PRB_FAN], S[PRB_FAN];
    for (int j = 0; j < PRB_FAN; ++j) {
      const int64_t p = (int64_t)node * PRB_FAN + j;
      e[j] = p < cnt ? L.sum[k][p] : 0.0f;
    }
    prb_node_prefix(e, S);
    const int left = cnt - 1 - node * PRB_FAN, last = left < PRB_FAN - 1 ? left : PRB_FAN - 1;
    const int j = prb_pick(S, r, last);
    r = r - (j ? S[j - 1] : 0.0f);
    node = node * PRB_FAN + j;
  }
  return node;
}

// ---- the elements ----------------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_HD float prb_uniform(uint32_t k) { return rng_uniform_mid(k); }
SIGMA_HD float prb_priority(float td, float eps, float alpha) { return powf(td + eps, alpha); }
SIGMA_HD float prb_weight(float q, float q_min, float neg_beta) { return powf(q / q_min, neg_beta); }
// reward[0 .. N) of the frame, its done flag, the critic's two values
SIGMA_HD float prb_x(const float* reward, int N, float done, float v, float v_next, float td_gamma) {
  const float nd = 1.0f - done, boot = (td_gamma * v_next) * nd;
  float x = 0.0f;
  for (int i = 0; i < N; ++i) x = x + fabsf((reward[i] + boot) - v);
  return x / (float)N;
}
SIGMA_HD float prb_norm(float x, float mn, float mx) {
  const float range = fmaxf(mx - mn, 1e-3f);
  const float y = ((x - mn) / range) * 10.0f;
  return fminf(fmaxf(y, 1e-3f), 10.0f);
}
#endif  // SIGMAENV_PRB_H
