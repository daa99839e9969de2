// sigmaenv_optim.h -- the arithmetic of the optimiser step on the device, stated ONCE: the global gradient norm of torch.nn.utils.clip_grad_norm_ (norm_type = 2,
// error_if_nonfinite = False) over ALL given tensors of ALL given networks together -- the reference clips over loss_module.parameters(), actor and critic in one
// norm (sigmarl/mappo_cavs.py:421-426) -- and one element's update by torch.optim.Adam as sigmarl/modules/optimization_module.py:69 builds it (weight_decay = 0,
// amsgrad = False, maximize = False).  The kernels of sigmaenv_optim.inc run these functions on the device; a host program runs them on the host
// (tests/test_optim_check.py holds them bit for bit to the float32 twin of tests/optim_check.py and, within derived bounds, to float64).
//
// Plain C++: no HIP include and no other file of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.  Every operator below is ONE IEEE fp32 operation in the order written (-ffp-contract=off; `/` and sqrtf are
// the correctly rounded ones, the compiler's default for this translation unit: no fast-math, no approximate division or square root; fp32 denormals are kept).
//
// The norm.  The tensors in the order given, each cut into chunks of OPTIM_CHUNK = 1024 consecutive elements (a tensor's last chunk may be short; a chunk never
// spans two tensors); chunk c is the c-th of that sequence and belongs to one workgroup of 256 lanes = 4 wavefronts of 64:
//   lane t           the chain s = 0; s = s + g[i] g[i] over the chunk's elements i = t, t + 256, t + 512, t + 768 (those below its length)      optim_lane_sumsq
//   wavefront        the butterfly v = v + v[lane ^ s], s = 32, 16, 8, 4, 2, 1 over its 64 consecutive lanes: every lane ends with the same bits
//   chunk            ((w0 + w1) + w2) + w3 over the four wavefronts                                                                                optim_reduce256
// The P chunk partials are then added the same way once more (the second level: actor and critic together have about 400 partials, more than 256 lanes):
//   lane t           the chain s = 0; s = s + partial[c] over c = t, t + 256, ..                                                                     optim_lane_sum
//   then the same butterfly and the same four wavefronts in order                                                                                   optim_total_sumsq
// No atomics; the shape of every sum is a function of the tensors' element counts alone: the same inputs give the same bits on every run.
//   total_norm = sqrtf(sum);   clip_coef = min(1, max_grad_norm / (total_norm + 1e-6f))                                                              optim_clip_coef
// A non-finite gradient does what torch does: the coefficient is NaN (min keeps it) and every parameter becomes NaN.
//
// Adam, step t >= 1 (the scalars that depend on t or are differences are formed on the host in double and rounded to fp32 once: optim_scalars):
//   one_minus_beta1 = fl(1 - beta1);  one_minus_beta2 = fl(1 - beta2);  step_size = fl(lr / (1 - beta1^t));  sqrt_bc2 = fl(sqrt(1 - beta2^t));  beta2, eps: fl
//   g' = g coef;   m = m + (g' - m) one_minus_beta1;   v = beta2 v + (one_minus_beta2 g') g';   p = p - step_size (m / (sqrtf(v) / sqrt_bc2 + eps))        optim_adam
#ifndef SIGMAENV_OPTIM_H
#define SIGMAENV_OPTIM_H
#include <math.h>
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define OPTIM_CHUNK 1024      /* elements of one chunk = one workgroup */
#define OPTIM_LANES 256       /* lanes of a workgroup */
#define OPTIM_MAX_TENSORS 32  /* tensors (weights and biases) of one step */
#define OPTIM_MAX_NETS 4      /* networks of one step */

// ---- the norm ------------------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_HD int optim_chunks(int64_t n) { return (int)((n + OPTIM_CHUNK - 1) / OPTIM_CHUNK); }
// lane t's chain over a chunk of n <= OPTIM_CHUNK elements
SIGMA_HD float optim_lane_sumsq(const float* g, int n, int t) {
  float s = 0.0f;
  for (int i = t; i < n; i += OPTIM_LANES) s = s + g[i] * g[i];
  return s;
}
// lane t's chain over the P chunk partials
SIGMA_HD float optim_lane_sum(const float* partial, int P, int t) {
  float s = 0.0f;
  for (int c = t; c < P; c += OPTIM_LANES) s = s + partial[c];
  return s;
}
// the 256 lane values of a workgroup -> their sum: the butterfly per wavefront of 64 lanes, then the four wavefronts in order.  (The kernels do the butterfly with
// cross-lane moves and pass the four wavefront sums through LDS: optim::block_sum, the same additions.)
static inline float optim_reduce256(const float* lane) {
  float v[OPTIM_LANES], u[OPTIM_LANES];
  for (int t = 0; t < OPTIM_LANES; ++t) v[t] = lane[t];
  for (int s = 32; s > 0; s >>= 1) {
    for (int t = 0; t < OPTIM_LANES; ++t) u[t] = v[t] + v[t ^ s];
    for (int t = 0; t < OPTIM_LANES; ++t) v[t] = u[t];
  }
  return ((v[0] + v[64]) + v[128]) + v[192];
}
static inline float optim_chunk_sumsq(const float* g, int n) {
  float lane[OPTIM_LANES];
  for (int t = 0; t < OPTIM_LANES; ++t) lane[t] = optim_lane_sumsq(g, n, t);
  return optim_reduce256(lane);
}
static inline float optim_total_sumsq(const float* partial, int P) {
  float lane[OPTIM_LANES];
  for (int t = 0; t < OPTIM_LANES; ++t) lane[t] = optim_lane_sum(partial, P, t);
  return optim_reduce256(lane);
}
SIGMA_HD float optim_total_norm(float sumsq) { return sqrtf(sumsq); }
// min(1, max_grad_norm / (total_norm + 1e-6)); a NaN stays a NaN (torch.clamp(max = 1))
SIGMA_HD float optim_clip_coef(float total_norm, float max_grad_norm) {
  const float c = max_grad_norm / (total_norm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

// ---- Adam ----------------------------------------------------------------------------------------------------------------------------------------------------------
struct OptimScalars {
  float beta2, one_minus_beta1, one_minus_beta2, step_size, sqrt_bc2, eps, max_grad_norm;
};
// the host's part, in double, each scalar rounded to fp32 once; t >= 1
static inline OptimScalars optim_scalars(double lr, double beta1, double beta2, double eps, double max_grad_norm, int64_t t) {
  OptimScalars s;
  s.beta2 = (float)beta2;
  s.one_minus_beta1 = (float)(1.0 - beta1);
  s.one_minus_beta2 = (float)(1.0 - beta2);
  s.step_size = (float)(lr / (1.0 - pow(beta1, (double)t)));
  s.sqrt_bc2 = (float)sqrt(1.0 - pow(beta2, (double)t));
  s.eps = (float)eps;
  s.max_grad_norm = (float)max_grad_norm;
  return s;
}
// one element: p, m (exp_avg), v (exp_avg_sq) in place; g is read
SIGMA_HD void optim_adam(const OptimScalars& s, float coef, float g, float& p, float& m, float& v) {
  const float gc = g * coef;
  m = m + (gc - m) * s.one_minus_beta1;
  v = s.beta2 * v + (s.one_minus_beta2 * gc) * gc;
  const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
  p = p - s.step_size * (m / denom);
}
#endif  // SIGMAENV_OPTIM_H
