// sigmaenv_dist.h -- everything that samples on the device, stated ONCE: the counter-based generator, the table of its draw ids, the conversions of a word into a
// uniform / a bounded integer / a normal pair, and the TanhNormal head of the policies (torchrl's NormalParamExtractor "biased_softplus_1.0" + TanhNormal as
// sigmarl/modules/decision_making_module.py:50-82 and priority_module.py:34-66 build them; torchrl is third-party and absent: restated from its published
// behaviour).  The kernels of sigmaenv.hip, sigmaenv_actor.inc, sigmaenv_wrappers.inc, sigmaenv_ppo.inc, sigmaenv_prb.inc and sigmaenv_isb.inc run these functions on the device; a host
// program runs them on the host (tests/test_dist_check.py holds the generator, the uniforms and the bounded draw bit for bit to tests/policy_head_check.py, the
// normals and the head to its float64 reference within its criterion, and the table to every Python mirror; tests/test_comm_noise_check.py holds the communication noise
// at the end of this file to tests/comm_noise_check.py).
//
// Plain C++: no HIP include and no other file of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.  Every operator below is ONE IEEE fp32 operation in the order written (-ffp-contract=off).  logf / expf /
// log1pf / tanhf / sincosf / cosf are the device's OCML functions on the device and libm's on a host: the only operations a host cannot reproduce to the bit.
#ifndef SIGMAENV_DIST_H
#define SIGMAENV_DIST_H
#include <math.h>
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

// ---- the generator -----------------------------------------------------------------------------------------------------------------------------------------------------
// counter-based RNG (specification shared with the oracle): 32-bit multiplicative mix + murmur3 finalisers over (seed, counter, env, agent, draw)
SIGMA_HD uint32_t rng_u32(uint64_t seed, uint64_t counter, uint32_t env, uint32_t agent, uint32_t draw) {
  uint32_t h = (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x9E3779B9u);
  h ^= ((uint32_t)counter + 0x7F4A7C15u) * 0x85EBCA6Bu;
  h ^= (env + 0x165667B1u) * 0xC2B2AE35u;
  h ^= (agent + 0x27D4EB2Fu) * 0x9E3779B1u;
  h ^= (draw + 0x61C88647u) * 0x85EBCA77u;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;   /* murmur3 fmix32, twice */
  h += 0x9E3779B9u;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// ---- the draw table: the `draw` of every stream, who draws it and what (env, agent) are in its key ---------------------------------------------------------------------
// (env: always the env's index in the WHOLE batch, sigmaenv_config_t.env_index_base + b, unless said otherwise)
#define AUTO_RESET_MAX_TRIES 64  /* tries of a reset: one per lane of a wavefront */
#define DRAW_RESET_TRY 0u        /* + 2 t: the path, + 2 t + 1: the point of try t of a full-env reset           reset_candidate     (env, agent) */
#define DRAW_RESET_SPEED 1000u   /* the start speed after a full-env reset                                       auto_reset_tile     (env, agent) */
#define DRAW_AGENT_TRY 2000u     /* + 2 t, + 2 t + 1: try t of a single-agent reset                              reset_candidate     (env, agent) */
#define DRAW_AGENT_SPEED 3000u   /* the start speed after a single-agent reset                                   auto_reset_tile     (env, agent) */
#define DRAW_SCENARIO 5000u      /* cpm_mixed: the sub-scenario a finished env draws                             draw_scenario       (env, 0) */
#define DRAW_ISB_RECORD 5100u    /* initial-state bank: does a collided env record?                               isb record          (env, 0)   sigmaenv_isb.h */
#define DRAW_ISB_USE 5101u       /* does a finished env restart from the bank?                                   isb restart         (env, 0) */
#define DRAW_ISB_INDEX 5102u     /* which bank entry                                                             isb restart         (env, 0) */
#define DRAW_ACTOR 7000u         /* u1, + 1: u2 of the actor's normal pair                                       actor_distribution  (env, agent) */
#define DRAW_PRIORITY 7100u      /* u1, + 1: u2 of the priority score's normal (cosine branch)                   priority_head       (env, agent) */
#define DRAW_SHUFFLE 7200u       /* the random priority order: position i draws j in [0, i]                      priority_random     (env, agent = i) */
#define DRAW_ENTROPY 7300u       /* u1, + 1: u2 of the PPO entropy sample                                        ppo_head            (env = frame, agent) */
#define DRAW_PRIORITY_ENTROPY 7350u /* u1, + 1: u2 of the priority PPO entropy sample (cosine branch)           ppo_head_1d         (env = frame, agent) */
#define DRAW_REPLAY 7400u        /* the replay sampler's uniform                                                 prb sample          (env = slot m, 0) */
#define COMM_NOISE_MAX_COLUMNS 8u /* 2 K action columns of a base observation at the largest K the library accepts (SIGMAENV_MAX_NEARING = 4) */
#define DRAW_COMM_NOISE 7500u    /* + 2 q: u1, + 2 q + 1: u2 of the normal (cosine branch) on action column q of a turn      turn_gather         (env, agent = the acting one) */
#define DRAW_OBS_NOISE 9000u     /* + k: element k of an observation row; open-ended, so the highest             obs_noise           (env, agent) */
static_assert(DRAW_RESET_TRY + 2u * AUTO_RESET_MAX_TRIES <= DRAW_RESET_SPEED && DRAW_RESET_SPEED < DRAW_AGENT_TRY, "full-env reset tries run into the next stream");
static_assert(DRAW_AGENT_TRY + 2u * AUTO_RESET_MAX_TRIES <= DRAW_AGENT_SPEED && DRAW_AGENT_SPEED < DRAW_SCENARIO, "single-agent reset tries run into the next stream");
static_assert(DRAW_SCENARIO < DRAW_ACTOR && DRAW_ACTOR + 1u < DRAW_PRIORITY && DRAW_PRIORITY + 1u < DRAW_SHUFFLE && DRAW_SHUFFLE < DRAW_ENTROPY &&
              DRAW_ENTROPY + 1u < DRAW_PRIORITY_ENTROPY && DRAW_PRIORITY_ENTROPY + 1u < DRAW_REPLAY && DRAW_REPLAY < DRAW_COMM_NOISE && DRAW_COMM_NOISE + 2u * COMM_NOISE_MAX_COLUMNS <= DRAW_OBS_NOISE,
              "the streams overlap, or the open-ended noise range is not the highest");
static_assert(DRAW_SCENARIO < DRAW_ISB_RECORD && DRAW_ISB_RECORD < DRAW_ISB_USE && DRAW_ISB_USE < DRAW_ISB_INDEX && DRAW_ISB_INDEX < DRAW_ACTOR,
              "the initial-state bank's draws leave their gap between the scenario draw and the actor's");

// ---- a word -> a number ------------------------------------------------------------------------------------------------------------------------------------------------
// U[0, 1): (k >> 8) * 2^-24, exact in fp32; never 1
SIGMA_HD float rng_uniform(uint32_t k) { return (float)(k >> 8) * (1.0f / 16777216.0f); }
// (0, 1]: the centre of the same cell; from k >> 8 = 2^23 on the + 0.5f rounds to even, so 1.0f is reachable (log u = 0) and 0 is not
SIGMA_HD float rng_uniform_mid(uint32_t k) { return ((float)(k >> 8) + 0.5f) * (1.0f / 16777216.0f); }
// an integer in [0, n): the high word of k * n
SIGMA_HD uint32_t rng_below(uint32_t k, uint32_t n) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umulhi(k, n);
#else
  return (uint32_t)(((uint64_t)k * n) >> 32);
#endif
}
// Box-Muller from the draws `draw` (u1) and `draw + 1` (u2) of one key: (z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2), ONE sincosf
#define RNG_TWO_PI 6.283185307179586f
SIGMA_HD void rng_normal_pair(uint64_t seed, uint64_t counter, uint32_t env, uint32_t agent, uint32_t draw, float* z0, float* z1) {
  const float u1 = rng_uniform_mid(rng_u32(seed, counter, env, agent, draw)), u2 = rng_uniform_mid(rng_u32(seed, counter, env, agent, draw + 1u));
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(RNG_TWO_PI * u2, &sn, &cs);
  *z0 = rad * cs;
  *z1 = rad * sn;
}
// z0 alone, through cosf (cosf(a) and the cosine of sincosf(a) are not known to agree bit for bit on the device: two functions)
SIGMA_HD float rng_normal_cos(uint64_t seed, uint64_t counter, uint32_t env, uint32_t agent, uint32_t draw) {
  const float u1 = rng_uniform_mid(rng_u32(seed, counter, env, agent, draw)), u2 = rng_uniform_mid(rng_u32(seed, counter, env, agent, draw + 1u));
  return sqrtf(-2.0f * logf(u1)) * cosf(RNG_TWO_PI * u2);
}

// ---- the TanhNormal head, one dimension --------------------------------------------------------------------------------------------------------------------------------
//   scale    = clamp_min(softplus(raw + inv_softplus(1.0 - 0.01)) + 0.01, 1e-4)     ("biased_softplus_1.0": bias 1.0, min_val 0.01, scale_lb 1e-4)
//   x = loc + scale * z;  y = clamp(tanh(x), -1 + 1e-6, 1 - 1e-6) (SafeTanhTransform, eps = finfo(float32).resolution);  action = low + (y + 1) * h, h = (high - low) / 2
//   log_prob = sum_d [ Normal(loc, scale).log_prob(x) - 2 (log 2 - x - softplus(-2 x)) - log h ]       (the caller subtracts log h; the 1-D priority head has none)
#define TN_BIAS 0.5254587192925021f /* ln(e^0.99 - 1) */
#define TN_LOG_SQRT_2PI 0.91893853320467274f
#define TN_LOG2 0.69314718055994531f
#define TN_EPS 1e-6f
#define TN_SCALE_LB 1e-4f
SIGMA_HD float tn_softplus(float v) { return v > 20.0f ? v : log1pf(expf(v)); }
SIGMA_HD float tn_raw_scale(float raw) { return tn_softplus(raw + TN_BIAS) + 0.01f; }
SIGMA_HD float tn_scale(float raw) { return fmaxf(tn_raw_scale(raw), TN_SCALE_LB); }
// d scale / d raw = sigmoid(raw + bias); 0 where the floor acts on s0 = tn_raw_scale(raw)
SIGMA_HD float tn_scale_slope(float raw, float s0) { return s0 < TN_SCALE_LB ? 0.0f : 1.0f / (1.0f + expf(-(raw + TN_BIAS))); }
SIGMA_HD float tn_clamp(float y) { return fminf(fmaxf(y, -1.0f + TN_EPS), 1.0f - TN_EPS); }
SIGMA_HD float tn_squash(float x) { return tn_clamp(tanhf(x)); }
SIGMA_HD float tn_affine(float low, float y, float h) { return low + (y + 1.0f) * h; }
// q = (x - loc) / scale (a sample's own x: q = z);  without the - log h of the affine map
SIGMA_HD float tn_log_density(float q, float log_scale, float x) {
  return -0.5f * q * q - log_scale - TN_LOG_SQRT_2PI - 2.0f * (TN_LOG2 - x - tn_softplus(-2.0f * x));
}

// ---- communication noise on the propagated actions (prioritized_ap_policy, sigmarl/helper_training.py:1271-1287) ------------------------------------------------------
// The acting agent sees column q of its 2 K neighbour-action columns as v + std z: the fp32 product rounded, then the fp32 sum rounded -- two operations whatever
// the compiler's contraction setting is (torch multiplies the draws by the std, then adds the tensor).  z: rng_normal_cos of DRAW_COMM_NOISE + 2 q under the key
// (seed, counter, env, the acting agent).
// The std goes by the column's POSITION, not by its quantity: the reference adds cat([s_v randn(2), s_d randn(2)]) to [a(n0).speed, a(n0).steer, a(n1).speed,
// a(n1).steer], so columns 0 and 1 take the speed's std and columns 2 and 3 the steering's.  (The 4-vector fits 2 K = 4 columns only: K = 2.)
SIGMA_HD float comm_noise_std(int q, float s_v, float s_d) { return q < 2 ? s_v : s_d; }
SIGMA_HD float comm_noise_seen(float v, float std, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const float p = std * z;
#else
  volatile float p = std * z;  /* (no pragma that every host compiler honours: the product is forced through memory) */
#endif
  return v + p;
}
#endif  // SIGMAENV_DIST_H
