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

// ==== the study of a CBF-filtered policy: six more numbers per env ========================================================================================================
// What sigmarl/evaluation_itsc26.py reduces a testing rollout to: compute_total_reward (:926-992, event rewards plus a driving-comfort penalty from acceleration and
// jerk of the applied speed command), compute_cbf_activation_percentage (:995-1035, normalised intervention degree and activation rate) and the task counters
// (:883-898, metric_task_success_rate :1450-1458).  The reference runs it with ONE env per process; here every env of the batch is such a run.  Same rules as above:
// every operator ONE IEEE operation in the order written, every Python scalar of the reference its nearest fp32 (torch's `x / 0.1` on an fp32 tensor is the IEEE
// fp32 division by fl32(0.1), `.abs() / 3.0` the one by 3.0f, `.pow(2)` is x * x: tests/test_eval_study_check.py repeats those checks).
//
// A study frame of agent i of env b adds to the frame above: (av, as) = the applied action SIGMAENV_BUF_ACTION[b,i,:]; (nv, ns) = the nominal action -- see
// evl_nominal_from_cbf --; the three event rewards, rows EVL_REW_GOAL, EVL_REW_AGENTS, EVL_REW_LANE of SIGMAENV_BUF_REWARD_INFO [12,B,N].
//   e = (r_goal + r_agents) + r_lane                                                                                                                   evl_study_terms
// An INITIAL frame -- the state after the reset -- takes av = as = nv = ns = e = 0 whatever the buffers hold (the reference's root info after a reset holds the
// zeros of a fresh scenario, road_traffic.py:670-675, 1522-1545), a = j = 0, and leaves the carry (v_prev, a_prev) = (0, 0).  Every other frame:
//   a = (av - v_prev) / EVL_DT      j = (a - a_prev) / EVL_DT      then v_prev = av, a_prev = a        (EVL_DT = fl32(0.1), the reference's constant, NOT Parameters.dt)
//   terms: q * q with q = |a| / 3.0f;  q * q with q = |j| / 20.0f;  |av - nv|;  |as - ns|;  |av|;  |as|;   activated = |av - nv| > fl32(1e-9) || |as - ns| > fl32(1e-9)
// The steering rate and its jerk are computed and discarded by the reference (:966-980): not accumulated.  A re-placement of testing mode does not touch the carry:
// the reference differences the stacked commands across it.  Per env and frame: the seven sums over the agents in evl_butterfly, ONE fp64 addition each into
// the seven accumulators (EVL_S_*), n_act += the number of activated agents (uint32).  No atomics.
// Finishing (evl_study_finish), M = F * N, each m the fp32-rounded mean (float)(sum / (double)M):
//   event = (float)sum_e    r_a = -0.2f * m_a2    r_j = -0.2f * m_j2    comfort = r_a + r_j    total = event + comfort
//   degree = 100.0f * (0.5f * (m_dv / (m_av + 1e-9f) + m_ds / (m_as + 1e-9f)))      rate = (float)((double)(100 * n_act) / (double)M)   (Python's 100 * int / int)
//   tries, success = the handle's SIGMAENV_BUF_TIMER columns 1, 2 minus their snapshot;  success_rate = (float)(100.0 * success / tries), NaN when tries <= 0
//   (the reference returns None).  F = 0: NaN wherever a mean enters.
// Against the exact value (derived in tests/eval_study_check.py): the sums as above (F + log2 G fp64 additions per chain), each term's own fp32 roundings, one fp32
// rounding per finishing operation.
#define EVL_STUDY_SUMS 7
#define EVL_S_EVENT 0
#define EVL_S_A2 1
#define EVL_S_J2 2
#define EVL_S_DV 3
#define EVL_S_DS 4
#define EVL_S_AV 5
#define EVL_S_AS 6
#define EVL_STUDY_METRICS 6 /* total_reward, event_reward, comfort_reward, cbf_activation_degree, cbf_activation_rate, task_success_rate */
#define EVL_STUDY_COUNTS 4  /* n_act, tries, success, frames */
#define EVL_REW_GOAL 1      /* rows of SIGMAENV_BUF_REWARD_INFO: rew_reach_goal, rew_collide_other_agents, rew_collide_lane */
#define EVL_REW_AGENTS 7
#define EVL_REW_LANE 8
#define EVL_DT 0.1f
#define EVL_A_NORM 3.0f
#define EVL_J_NORM 20.0f
#define EVL_W_COMF 0.2f
#define EVL_EPS 1e-9f

// Where the nominal action of a frame lies, stated once: SIGMAENV_BUF_CBF_NOMINAL when the chain runs the CBF-QP (world_state.nominal_action_* is then what CBFQP left
// behind, cbf_qp.py:1315-1379), the applied action itself otherwise (info() mirrors it, road_traffic.py:1522-1540).  The library asks it of a handle (a QP reward
// method with the CBF tables attached: what its chain does), sigmarl_amd/scenario.py of its Parameters ((is_using_cbf_training or is_using_cbf_testing) and
// is_solve_qp: what the reference's info() does).  ONE rule asked of two sets of facts, which can disagree: a "cbf" reward method with is_solve_qp and the tables
// attached but neither is_using_cbf_* set gives the nominal buffer here and the applied action there; a handle that never attached the tables, the opposite.  The
// evaluator follows the chain, because that is what wrote the buffers it reads.
SIGMA_HD int evl_nominal_from_cbf(int cbf_in_the_loop, int is_solve_qp) { return cbf_in_the_loop && is_solve_qp; }

typedef struct evl_study_acc {
  double sum[EVL_STUDY_SUMS];
  uint32_t n_act;
} evl_study_acc_t;

// one agent's terms of one frame; carry = (v_prev, a_prev) of the agent, read and written.  Returns activated (0 / 1).
SIGMA_HD uint32_t evl_study_terms(int initial, float av, float as, float nv, float ns, float r_goal, float r_agents, float r_lane, float* carry, float* term) {
  float e = r_goal + r_agents;
  e = e + r_lane;
  float a = 0.0f, j = 0.0f;
  if (initial) {
    av = 0.0f; as = 0.0f; nv = 0.0f; ns = 0.0f; e = 0.0f;
  } else {
    const float d1 = av - carry[0];
    a = d1 / EVL_DT;
    const float d2 = a - carry[1];
    j = d2 / EVL_DT;
  }
  carry[0] = av;
  carry[1] = a;
  const float qa = fabsf(a) / EVL_A_NORM;
  const float qj = fabsf(j) / EVL_J_NORM;
  const float dv = av - nv;
  const float ds = as - ns;
  term[EVL_S_EVENT] = e;
  term[EVL_S_A2] = qa * qa;
  term[EVL_S_J2] = qj * qj;
  term[EVL_S_DV] = fabsf(dv);
  term[EVL_S_DS] = fabsf(ds);
  term[EVL_S_AV] = fabsf(av);
  term[EVL_S_AS] = fabsf(as);
  return (fabsf(dv) > EVL_EPS) || (fabsf(ds) > EVL_EPS);
}

// one study frame of one env on a host: applied, nominal [N,2]; r_goal, r_agents, r_lane [N]; carry [N,2]
static inline void evl_study_frame(int initial, const float* applied, const float* nominal, const float* r_goal, const float* r_agents, const float* r_lane, int N, float* carry,
                                   evl_study_acc_t* acc) {
  double t[EVL_STUDY_SUMS][EVL_MAX_GROUP];
  uint32_t n = 0;
  for (int i = 0; i < N; ++i) {
    float term[EVL_STUDY_SUMS];
    n += evl_study_terms(initial, applied[i * 2], applied[i * 2 + 1], nominal[i * 2], nominal[i * 2 + 1], r_goal[i], r_agents[i], r_lane[i], carry + i * 2, term);
    for (int k = 0; k < EVL_STUDY_SUMS; ++k) t[k][i] = (double)term[k];
  }
  for (int k = 0; k < EVL_STUDY_SUMS; ++k) acc->sum[k] = evl_add(acc->sum[k], evl_butterfly(t[k], N));
  acc->n_act += n;
}

SIGMA_HD float evl_study_ratio(float m_diff, float m_abs) {
  const float den = m_abs + EVL_EPS;
  return m_diff / den;
}

// metrics[0 .. 5] and counts[0 .. 3] of one env; sum = the seven accumulators, tries / success = the counters' differences (int32: a counter never runs backwards)
SIGMA_HD void evl_study_finish(const double* sum, uint32_t n_act, int32_t tries, int32_t success, uint32_t F, int N, float* metrics, uint32_t* counts) {
  const float event = (float)sum[EVL_S_EVENT];
  const float r_a = -EVL_W_COMF * evl_mean(sum[EVL_S_A2], F, N);
  const float r_j = -EVL_W_COMF * evl_mean(sum[EVL_S_J2], F, N);
  const float comfort = r_a + r_j;
  const float rv = evl_study_ratio(evl_mean(sum[EVL_S_DV], F, N), evl_mean(sum[EVL_S_AV], F, N));
  const float rs = evl_study_ratio(evl_mean(sum[EVL_S_DS], F, N), evl_mean(sum[EVL_S_AS], F, N));
  const float both = rv + rs;
  const float half = 0.5f * both;
  metrics[0] = event + comfort;
  metrics[1] = event;
  metrics[2] = comfort;
  metrics[3] = 100.0f * half;
  metrics[4] = (float)((double)(100ull * (uint64_t)n_act) / (double)(F * (uint32_t)N));
  metrics[5] = tries > 0 ? (float)(100.0 * (double)success / (double)tries) : (float)NAN;
  if (counts) { counts[0] = n_act; counts[1] = (uint32_t)tries; counts[2] = (uint32_t)success; counts[3] = F; }
}
#endif  // SIGMAENV_EVAL_H
