// sigmaenv_episode.h -- the arithmetic of the episode return on the device, stated ONCE: torchrl's RewardSum transform as the reference wraps its env in it
// (sigmarl/mappo_cavs.py:178-183: in_keys = the agents' reward, out_keys = "episode_reward", reset by the env's done flag) and the number every iteration reports,
// episode_reward[done].mean() (_log_and_save, :468-478).  torchrl is third-party and absent: restated from its published behaviour.  The kernels of
// sigmaenv_episode.inc run these functions on the device; a host program runs them on the host (tests/test_episode_check.py holds them bit for bit to the float32
// twin of tests/episode_check.py and, within a derived bound, to float64).
//
// Plain C++: no HIP include and no other file of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.  Every operator below is ONE IEEE fp32 operation in the order written (-ffp-contract=off; `/` is the
// correctly rounded one; fp32 denormals are kept).
//
// The record.  r[t,b,i] and done[t,b] are read in place from the record rows of a rollout (offsets N*D + i and N*(D+1) of env b's row of step t), c[b,i] is the
// running return of agent i's open episode.  Forwards over t, sequentially -- the record IS the step-by-step fp32 sum, so there is no scan over t:
//   E[t,b,i] = c + r[t,b,i]                                                                                                                            epr_add
//   c        = done[t,b] != 0 ? 0 : E[t,b,i]                                                                                                           epr_carry
// with c = carry[b,i] before t = 0 and carry[b,i] = the last c after t = T - 1.  The frame that finishes an episode carries the whole episode's return; the next
// frame starts from zero.  Only the env's done flag resets: an agent re-placed on its own keeps its sum, as in the reference.
//
// The reduction over the done frames (t,b) -- K of them -- in a fixed order, a function of (T, B, N) alone; no atomics:
//   frame      x[t,b] = the chain x = 0; x = x + E[t,b,i] over i = 0 .. N-1                                                                             epr_frame_sum
//   env        s[b]   = the chain s = 0; s = s + x[t,b] over the done steps t of env b, t ascending;  k[b] = their number                                (in the walk over t)
//   all envs   ONE workgroup of EPR_LANES = 256 lanes = 4 wavefronts of 64: lane l the chain v = 0; v = v + s[b] over b = l, l + 256, ..;                 epr_lane_sum
//              per wavefront the butterfly v = v + v[lane ^ m], m = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits);
//              ((w0 + w1) + w2) + w3 over the four wavefronts -> S;  the counts k[b] the same way in int32 -> K                                          epr_reduce256
//   result     [0] = S / ((float)K * (float)N) (the product in fp32, one division: NaN at K = 0, as the mean of an empty selection is);  [1] = S;
//              [2] = (float)K (exact: T * B < 2^24 is required);  [3] = 0                                                                               epr_mean
// The longest chain of additions from an E to S: N (frame) + T (env: at most T done steps) + ceil(B / 256) (lane) + 6 (butterfly) + 3 (wavefronts)     epr_longest_chain
// The first addition of each of the three chains adds to 0 and is exact, so at most epr_longest_chain - 3 of them round: against the exact sum of the recorded E
// over the done frames |S - sum| <= ((1 + u)^(n-3) - 1) sum|E| <= n u sum|E| with u = 2^-24 for every n = epr_longest_chain below 10^4.
#ifndef SIGMAENV_EPISODE_H
#define SIGMAENV_EPISODE_H
#include <math.h>
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define EPR_LANES 256          /* lanes of the workgroup that adds the envs' sums */
#define EPR_MAX_FRAMES (1 << 24) /* T * B must stay below: K is reported as a float */

// ---- the record --------------------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_HD float epr_add(float c, float r) { return c + r; }
SIGMA_HD float epr_carry(float E, float done) { return done != 0.0f ? 0.0f : E; }

// ---- the reduction -----------------------------------------------------------------------------------------------------------------------------------------------------
// a done frame's sum over its agents, in order (the kernel fetches the E of agent i from the lane that holds it: the same additions)
SIGMA_HD float epr_frame_sum(const float* E, int N) {
  float x = 0.0f;
  for (int i = 0; i < N; ++i) x = x + E[i];
  return x;
}
// lane l's chains over the envs' sums and counts
SIGMA_HD float epr_lane_sum(const float* s, int B, int l) {
  float v = 0.0f;
  for (int b = l; b < B; b += EPR_LANES) v = v + s[b];
  return v;
}
SIGMA_HD int32_t epr_lane_count(const int32_t* k, int B, int l) {
  int32_t v = 0;
  for (int b = l; b < B; b += EPR_LANES) v = v + k[b];
  return v;
}
// the 256 lane values -> their sum: the butterfly per wavefront of 64 lanes, then the four wavefronts in order.  (The kernel does the butterfly with cross-lane
// moves and passes the four wavefront sums through LDS: the same additions.)
static inline float epr_reduce256(const float* lane) {
  float v[EPR_LANES], u[EPR_LANES];
  for (int t = 0; t < EPR_LANES; ++t) v[t] = lane[t];
  for (int m = 32; m > 0; m >>= 1) {
    for (int t = 0; t < EPR_LANES; ++t) u[t] = v[t] + v[t ^ m];
    for (int t = 0; t < EPR_LANES; ++t) v[t] = u[t];
  }
  return ((v[0] + v[64]) + v[128]) + v[192];
}
SIGMA_HD float epr_mean(float S, int32_t K, int N) { return S / ((float)K * (float)N); }
SIGMA_HD int epr_longest_chain(int T, int B, int N) { return N + T + (B + EPR_LANES - 1) / EPR_LANES + 6 + 3; }

// ---- the whole call on a host: what sigmaenv_episode_return leaves in carry, episode_reward (optional) and result ------------------------------------------------------
// slab: the record block of step t at slab + t * stride, env b's row at + b * W, W = N * (D + 1) + 1;  s / k: scratch of B entries each
static inline void epr_run(const float* slab, int64_t stride, int T, int B, int N, int D, float* carry, float* episode_reward, float* result, float* s, int32_t* k) {
  const int64_t W = (int64_t)N * (D + 1) + 1;
  for (int b = 0; b < B; ++b) {
    s[b] = 0.0f;
    k[b] = 0;
  }
  float E[64];  // (N <= SIGMAENV_MAX_AGENTS = 64)
  for (int t = 0; t < T; ++t)
    for (int b = 0; b < B; ++b) {
      const float* row = slab + (int64_t)t * stride + (int64_t)b * W + (int64_t)N * D;
      const float done = row[N];
      for (int i = 0; i < N; ++i) {
        E[i] = epr_add(carry[(int64_t)b * N + i], row[i]);
        if (episode_reward) episode_reward[((int64_t)t * B + b) * N + i] = E[i];
        carry[(int64_t)b * N + i] = epr_carry(E[i], done);
      }
      if (done != 0.0f) {
        s[b] = s[b] + epr_frame_sum(E, N);
        k[b] = k[b] + 1;
      }
    }
  float lane[EPR_LANES];
  int32_t K = 0;
  for (int l = 0; l < EPR_LANES; ++l) {
    lane[l] = epr_lane_sum(s, B, l);
    K += epr_lane_count(k, B, l);
  }
  const float S = epr_reduce256(lane);
  result[0] = epr_mean(S, K, N);
  result[1] = S;
  result[2] = (float)K;
  result[3] = 0.0f;
}
#endif  // SIGMAENV_EPISODE_H
