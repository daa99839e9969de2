// sigmaenv_eval.h -- the arithmetic of a policy's evaluation on the device, stated ONCE: the four numbers per env the reference reduces a testing rollout to
// (sigmarl/evaluation_base.py:184-217, _evaluate_model_i): the average speed velocities.norm(dim=-1).mean(dim=(-2, -1)) (:205-207), the agent-agent collision rate
// is_collision_with_agents.squeeze(-1).any(dim=-1).sum(dim=-1) / num_steps (:208-210), the agent-lanelet collision rate (:211-214) and the mean centre-line
// deviation distance_ref.squeeze(-1).mean(dim=(-2, -1)) (:215-217).  The kernels of sigmaenv_eval.inc run these functions on the device; a host program runs them on
// the host (tests/test_eval_check.py holds them bit for bit to the float32 twin of tests/eval_check.py and, within a derived bound, to float64).
//
// Plain C++: no HIP include and no other file of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.  Every operator below is ONE IEEE operation in the order written (-ffp-contract=off; sqrtf and `/` are the
// correctly rounded ones; denormals are kept).
//
// A frame of env b is what the per-step output buffers hold at one moment, and nothing else:
//   state[b,i,5:7] = (vx, vy), the reference's info["vel"];  dist_ref[b,i] = info["distance_ref"];  col_agents[b,i,j] (u8);  byte 0 of col_flags[b,i,.] =
//   with_lanelets (bytes 1 .. 3 -- entry segment, exit segment, reset request -- are never counted).
// Per frame:
//   n_i = sqrtf(vx * vx + vy * vy)               two products, one addition, one square root, each fp32                                                evl_speed
//   aa  = OR over i, j of col_agents[b,i,j]      is_collision_with_agents.squeeze(-1).any(dim=-1) of the frame (:209)
//   al  = OR over i of col_flags[b,i,0]
// The frame's two sums over the agents, in fp64, in a fixed butterfly: lane group G = the smallest power of two >= N (<= 64: SIGMAENV_MAX_AGENTS); lane i holds
// (double)n_i -- or (double)dist_ref_i --, the padding lanes N .. G-1 hold +0.0; v = v + v[lane ^ m] for m = G/2, .., 1 (every lane ends with the same bits) evl_group, evl_butterfly
// Per env, over the frames in their order: sum_speed = sum_speed + frame_sum, sum_dref likewise (fp64, ONE addition per frame);  n_aa += aa, n_al += al, frames += 1
// (uint32)                                                                                                                                               evl_acc
// Finishing, F = frames:
//   m0 = (float)(sum_speed / (double)(F * N))    m1 = (float)n_aa / (float)F    m2 = (float)n_al / (float)F    m3 = (float)(sum_dref / (double)(F * N))    evl_mean, evl_rate
// F * N < 2^24 is required (EVL_MAX_TERMS), so the counts are exact floats and the two rates are ONE fp32 division of two exactly represented integers -- bit for
// bit the count / num_steps torch computes at :208-214.  F = 0: NaN in all four (0 / 0).  No atomics: every result is a function of the inputs and (N, B, F) alone.
// Against the exact mean of the exact terms: one fp32 rounding of the result, F + log2 G roundings of fp64 additions per chain (bounded by F N + log2 G), and each
// term's own half-ulp of the sqrtf:  |m - exact| <= 2^-24 |exact| + (F N + log2 G) 2^-53 sum|terms| / (F N)  (+ the terms' own rounding, carried the same way).
#ifndef SIGMAENV_EVAL_H
#define SIGMAENV_EVAL_H
#include <math.h>
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define EVL_MAX_TERMS (1 << 24) /* frames * N must stay below: the counts are reported through floats */
#define EVL_TRACE_COLS 8        /* a trace row: x, y, vx, vy, dist_ref, n_i, col_agents-any-j (0/1), col_lanelet (0/1) */
#define EVL_MAX_GROUP 64        /* (SIGMAENV_MAX_AGENTS) */

typedef struct evl_acc {
  double sum_speed, sum_dref;
  uint32_t n_aa, n_al, frames;
} evl_acc_t;

SIGMA_HD float evl_speed(float vx, float vy) {
  const float xx = vx * vx;
  const float yy = vy * vy;
  const float s = xx + yy;
  return sqrtf(s);
}
SIGMA_HD int evl_group(int N) {
  int G = 1;
  while (G < N) G <<= 1;
  return G;
}
SIGMA_HD double evl_add(double acc, double frame_sum) { return acc + frame_sum; }
SIGMA_HD float evl_mean(double sum, uint32_t F, int N) { return (float)(sum / (double)(F * (uint32_t)N)); }
SIGMA_HD float evl_rate(uint32_t n, uint32_t F) { return (float)n / (float)F; }
// would one more frame reach the limit?
SIGMA_HD int evl_full(uint64_t frames, int N) { return (frames + 1u) * (uint64_t)N >= (uint64_t)EVL_MAX_TERMS; }

// the butterfly over a lane group on a host: term[0 .. N-1] the agents' terms, padding +0.0.  (The kernel holds one term per lane and fetches lane ^ m with a
// cross-lane move: the same additions.)
static inline double evl_butterfly(const double* term, int N) {
  double v[EVL_MAX_GROUP], u[EVL_MAX_GROUP];
  const int G = evl_group(N);
  for (int l = 0; l < G; ++l) v[l] = l < N ? term[l] : 0.0;
  for (int m = G >> 1; m > 0; m >>= 1) {
    for (int l = 0; l < G; ++l) u[l] = v[l] + v[l ^ m];
    for (int l = 0; l < G; ++l) v[l] = u[l];
  }
  return v[0];
}

// ---- one frame of one env on a host: what sigmaenv_eval_accumulate does to the env's accumulators (and, with trace != NULL, the N trace rows of the frame) ----------
// state [N,8], dist_ref [N], col_agents [N,N] u8, col_flags [N,4] u8: the env's rows of the four buffers
static inline void evl_frame(const float* state, const float* dist_ref, const uint8_t* col_agents, const uint8_t* col_flags, int N, evl_acc_t* acc, float* trace) {
  double sp[EVL_MAX_GROUP], dr[EVL_MAX_GROUP];
  uint32_t aa = 0, al = 0;
  for (int i = 0; i < N; ++i) {
    const float n_i = evl_speed(state[i * 8 + 5], state[i * 8 + 6]);
    sp[i] = (double)n_i;
    dr[i] = (double)dist_ref[i];
    uint32_t row = 0;
    for (int j = 0; j < N; ++j) row |= col_agents[i * N + j] != 0;
    const uint32_t lane = col_flags[i * 4] != 0;
    aa |= row;
    al |= lane;
    if (trace) {
      float* r = trace + i * EVL_TRACE_COLS;
      r[0] = state[i * 8 + 0]; r[1] = state[i * 8 + 1]; r[2] = state[i * 8 + 5]; r[3] = state[i * 8 + 6];
      r[4] = dist_ref[i]; r[5] = n_i; r[6] = (float)row; r[7] = (float)lane;
    }
  }
  acc->sum_speed = evl_add(acc->sum_speed, evl_butterfly(sp, N));
  acc->sum_dref = evl_add(acc->sum_dref, evl_butterfly(dr, N));
  acc->n_aa += aa;
  acc->n_al += al;
  acc->frames += 1;
}

// ---- finishing: metrics[0 .. 3] of one env -----------------------------------------------------------------------------------------------------------------------------
SIGMA_HD void evl_finish(double sum_speed, double sum_dref, uint32_t n_aa, uint32_t n_al, uint32_t F, int N, float* metrics) {
  metrics[0] = evl_mean(sum_speed, F, N);
  metrics[1] = evl_rate(n_aa, F);
  metrics[2] = evl_rate(n_al, F);
  metrics[3] = evl_mean(sum_dref, F, N);
}
#endif  // SIGMAENV_EVAL_H
