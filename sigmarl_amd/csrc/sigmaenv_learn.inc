// sigmaenv_learn.inc -- what the trainer computes right after collector.rollout(), on the rollout's records where they lie (included by sigmaenv.hip after
// sigmaenv_wrappers.inc; the contracts are in include/sigmaenv.h, sigmaenv_gae).
//
// What it restates:
//   _compute_gae          sigmarl/mappo_cavs.py:357-386 with the GAE(gamma, lmbda, value_network = critic, average_gae = False) of
//                         sigmarl/modules/optimization_module.py:62-67 (torchrl's generalized advantage estimate; torchrl is third-party and absent: restated from
//                         its published behaviour, DESIGN.md section 2)
//   compute_td_error      sigmarl/helper_training.py:1029-1068 (the priorities of the prioritized replay buffer)
// The critic's two passes over the records are sigmaenv_mlp32_forward_rows (sigmaenv_mlp32.inc); these kernels take its [T, B] values.
//
// Mapping.  T * B * N is 2 M elements at the metric's shape (32 x 4096 x 16): 24 MB of traffic, a latency-bound launch.  GAE is a recursion over t and independent
// over (env, agent): one lane per (env, agent) walks t downwards, the loads of GAE_UNROLL steps are issued before the first of them is used (the recursion itself is
// three dependent operations per step).  Reward and done are read in place from the record rows (a lane's reward is 4 bytes of a W-float row: the N lanes of an env
// share the cache lines).  The TD priorities are one lane per (t, env) for the raw error, a wavefront reduction and one vector atomic min / max per wavefront on
// the bits of the non-negative floats (order-independent: the result does not depend on scheduling), then one pass that normalises in place.
// -ffp-contract=off (Makefile): every operator below is one IEEE fp32 operation.

namespace learn {

#define GAE_UNROLL 4

__global__ void __launch_bounds__(256) sigmaenv_gae_kernel(const float* __restrict__ slab, long long slab_stride, int T, int B, int N, int D, const float* __restrict__ v,
                                                           const float* __restrict__ vn, float gamma, float c, float* __restrict__ adv, float* __restrict__ vt) {
  sigma_poison_lds();
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * N) return;
  const int b = (int)(e / N), i = (int)(e - (long long)b * N);
  const long long W = (long long)N * (D + 1) + 1;
  const float* row = slab + (long long)b * W + (long long)N * D;  // the env's [N reward | done] tail in block 0
  float a_next = 0.0f;
  for (int t1 = T; t1 > 0; t1 -= GAE_UNROLL) {
    float r[GAE_UNROLL] = {}, dn[GAE_UNROLL] = {}, sv[GAE_UNROLL] = {}, nv[GAE_UNROLL] = {};
#pragma unroll
    for (int u = 0; u < GAE_UNROLL; ++u) {
      const int t = t1 - 1 - u;
      if (t >= 0) {
        const float* p = row + (long long)t * slab_stride;
        r[u] = p[i]; dn[u] = p[N];
        sv[u] = v[(long long)t * B + b]; nv[u] = vn[(long long)t * B + b];
      }
    }
#pragma unroll
    for (int u = 0; u < GAE_UNROLL; ++u) {
      const int t = t1 - 1 - u;
      if (t >= 0) {
        const float nd = 1.0f - dn[u];
        const float d = (r[u] + (gamma * nv[u]) * nd) - sv[u];
        const float a = d + ((c * nd) * a_next);
        const long long o = ((long long)t * B + b) * N + i;
        adv[o] = a;
        vt[o] = a + sv[u];
        a_next = a;
      }
    }
  }
}

// raw[t, b] = (sum_i |(r_i + (td_gamma v_next) nd) - v|) / N, the sum in the order i = 0 .. N - 1; mm[0] / mm[1]: the bits of the smallest / largest raw value
__global__ void __launch_bounds__(256) sigmaenv_td_raw_kernel(const float* __restrict__ slab, long long slab_stride, int T, int B, int N, int D, const float* __restrict__ v,
                                                              const float* __restrict__ vn, float td_gamma, float* __restrict__ raw, uint32_t* __restrict__ mm) {
  sigma_poison_lds();
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = e < (long long)T * B;
  float x = 0.0f;
  if (on) {
    const int t = (int)(e / B), b = (int)(e - (long long)t * B);
    const float* p = slab + (long long)t * slab_stride + (long long)b * ((long long)N * (D + 1) + 1) + (long long)N * D;
    const float nd = 1.0f - p[N], sv = v[e], boot = (td_gamma * vn[e]) * nd;
    for (int i = 0; i < N; ++i) x = x + fabsf((p[i] + boot) - sv);
    x = x / (float)N;
    raw[e] = x;
  }
  // |.| >= 0: the unsigned order of the bits is the order of the values (a NaN, if the inputs hold one, sorts above every number).  Lanes past the end are neutral.
  uint32_t lo = on ? __float_as_uint(x) : 0xFFFFFFFFu, hi = on ? __float_as_uint(x) : 0u;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const uint32_t lo2 = (uint32_t)__shfl_xor((int)lo, s), hi2 = (uint32_t)__shfl_xor((int)hi, s);
    lo = lo2 < lo ? lo2 : lo;
    hi = hi2 > hi ? hi2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}

// ((x - min) / max(max - min, 1e-3)) * 10 clamped to [1e-3, 10], in place
__global__ void __launch_bounds__(256) sigmaenv_td_norm_kernel(float* __restrict__ raw, long long n, const uint32_t* __restrict__ mm) {
  sigma_poison_lds();
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float mn = __uint_as_float(mm[0]), mx = __uint_as_float(mm[1]);
  const float range = fmaxf(mx - mn, 1e-3f);
  const float y = ((raw[e] - mn) / range) * 10.0f;
  raw[e] = fminf(fmaxf(y, 1e-3f), 10.0f);
}

}  // namespace learn

extern "C" int sigmaenv_gae(sigmaenv_t* h, const sigmaenv_gae_args_t* a) {
  if (!h || !a) return SIGMAENV_EINVAL;
  if (a->n_steps < 1 || !a->slab || !a->state_value || !a->next_state_value || !a->advantage || !a->value_target) {
    h->err = "gae: n_steps >= 1, slab, state_value, next_state_value, advantage and value_target are required";
    return SIGMAENV_EINVAL;
  }
  const long long W = (long long)h->N * (h->D + 1) + 1, own = (long long)h->B * W;
  if (a->slab_stride != 0 && a->slab_stride < own) { h->err = "gae: slab_stride below the handle's own record block B * (N * (D + 1) + 1)"; return SIGMAENV_EINVAL; }
  if ((long long)a->n_steps * h->B * h->N > 0x7FFFFFFFll * 256) { h->err = "gae: n_steps * B * N too large for one launch"; return SIGMAENV_EINVAL; }
  const long long stride = a->slab_stride ? a->slab_stride : own;
  HIPCHK(h, hipSetDevice(h->device));
  const float c = a->gamma * a->lmbda;  // fl32(fl32(gamma) fl32(lmbda)): formed once, here (host code is built without contraction as well)
  const long long BN = (long long)h->B * h->N, TB = (long long)a->n_steps * h->B;
  hipLaunchKernelGGL(learn::sigmaenv_gae_kernel, dim3((unsigned)((BN + 255) / 256)), dim3(256), 0, h->stream, a->slab, stride, (int)a->n_steps, h->B, h->N, h->D, a->state_value,
                     a->next_state_value, a->gamma, c, a->advantage, a->value_target);
  HIPCHK(h, hipGetLastError());
  if (!a->td_priority) return SIGMAENV_OK;
  if (!h->learn_minmax) {
    const int rc = dev_alloc(h, (void**)&h->learn_minmax, 2 * sizeof(uint32_t), true);
    if (rc) return rc;
  }
  HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->learn_minmax, (int)0xFFFFFFFFu, 1, h->stream));
  HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(h->learn_minmax + 1), 0, 1, h->stream));
  hipLaunchKernelGGL(learn::sigmaenv_td_raw_kernel, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, h->stream, a->slab, stride, (int)a->n_steps, h->B, h->N, h->D, a->state_value,
                     a->next_state_value, a->td_gamma, a->td_priority, h->learn_minmax);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(learn::sigmaenv_td_norm_kernel, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, h->stream, a->td_priority, TB, (const uint32_t*)h->learn_minmax);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}
