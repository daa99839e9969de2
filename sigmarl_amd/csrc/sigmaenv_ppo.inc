// sigmaenv_ppo.inc -- the clip-PPO loss head of a minibatch update, on the learner's records where they lie (included by sigmaenv.hip after sigmaenv_learn.inc; the
// contract -- every formula, the outputs and the order of the sums -- is in include/sigmaenv.h, sigmaenv_ppo_head).
//
// What it restates: torchrl's ClipPPOLoss as sigmarl/modules/optimization_module.py:44-66 configures it (clip_epsilon, entropy_coeff = entropy_eps,
// normalize_advantage = False, the default smooth-L1 critic loss, samples_mc_entropy = 1) on the TanhNormal of actor_distribution (sigmaenv_actor.inc), for the
// minibatches of frames of sigmarl/mappo_cavs.py:321-340 / 389-407.  torchrl is third-party and absent: restated from its published behaviour (sigmaenv_actor.inc).
//
// Mapping.  One lane per (minibatch slot m, agent n) row: the network's four outputs are one 16-byte load, dout_actor one 16-byte store; the frame's index entry and the
// critic's value are loaded once per lane, i.e. once per frame and agent (the N lanes of a frame read the same words); the four records are read through the index.
// A few hundred bytes and ~20 transcendental calls per row: memory- and latency-bound, nothing to tune beyond coalescing.  dout_critic[m] sums over the frame's
// agents: the lane of agent 0 walks them in order (N more 4-byte loads of value_target, which its neighbours have just brought into the cache) -- no cross-lane
// sum whose shape would depend on where a frame falls in a wavefront.  The five means: a butterfly over the wavefront's 64 lanes, the four wavefronts in order
// (PPO_SUMS partial sums per workgroup), then sigmaenv_ppo_sum_kernel, ONE wavefront: lane k adds the workgroups k, k + 64, .. in order, the same butterfly, and the
// scalars are formed by lane 0.  No atomics; the shape of every sum is a function of (M, N) alone.
//
// sigmaenv_ppo_head_1d: the same loss on the priority module's 1-D TanhNormal on [-1, 1] (priority_module.py:93-126: a second ClipPPOLoss over the priority actor
// and its own critic).  Mapping: one lane per (m, n) row again; the network's two outputs (loc, raw scale) are one 8-byte load, dout_actor one 8-byte store; the
// recorded score, its log-probability, the advantage and the value target are 4-byte loads through the index.  No affine map and no - log h (the bounds are the
// trivial ones: sigmaenv_priority_head_kernel's expressions, sigmaenv_wrappers.inc); the entropy sample is the cosine branch of a normal pair under
// DRAW_PRIORITY_ENTROPY, so both heads run on one (seed, counter) without sharing a draw.  The sums and sigmaenv_ppo_sum_kernel are the 2-D head's.  The 2-D
// kernel is not touched: its instantiation keeps its bits.
// -ffp-contract=off (Makefile): every operator below is one IEEE fp32 operation.

namespace ppo {

#define PPO_SUMS 5  // sum of min(g1, g2) | of logp' | of the smooth-L1 terms | of the clipped flags | of -lw

struct HeadArgs {
  const int32_t* index;
  const float *out, *value, *action, *old_logp, *adv, *vtarget;
  float *dout_actor, *dout_critic, *partial;
  int M, N, F, groups;
  float low[2], high[2];
  float log_lo, log_hi;  // log1p(-eps), log1p(eps): rounded once, on the host
  float inv;             // 1 / (M N)
  float ce_inv, cc_inv;  // entropy_coeff * inv, critic_coeff * inv (one rounding each, on the host)
  uint64_t seed, counter;
};

// v + the other 63 lanes' v: the same tree in every lane (fp32 addition commutes), so every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = v + __shfl_xor(v, s);
  return v;
}

__global__ void __launch_bounds__(256) sigmaenv_ppo_head_kernel(HeadArgs a) {
  sigma_poison_lds();
  __shared__ float wsum[PPO_SUMS][4];
  const int tid = threadIdx.x;
  const long long r = (long long)blockIdx.x * blockDim.x + tid, R = (long long)a.M * a.N;
  float t[PPO_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (r < R) {
    const int m = (int)(r / a.N), n = (int)(r - (long long)m * a.N);
    const int f = a.index[m];
    float4 d4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)f < (unsigned)a.F) {  // (an entry outside the records is never an address: the row contributes zeros)
      const long long fr = (long long)f * a.N + n;
      const float4 o = reinterpret_cast<const float4*>(a.out)[r];
      const float2 act = reinterpret_cast<const float2*>(a.action)[fr];
      const float old = a.old_logp[fr], A = a.adv[fr], vt = a.vtarget[fr], v = a.value[m];
      // the entropy sample's draw: actor_distribution's normal pair with the frame as the env
      float z[2];
      rng_normal_pair(a.seed, a.counter, (uint32_t)f, (uint32_t)n, DRAW_ENTROPY, &z[0], &z[1]);
      const float loc[2] = {o.x, o.y}, raw[2] = {o.z, o.w}, ac[2] = {act.x, act.y};
      float sig[2], dsdr[2], q[2], xs[2], lp = 0.0f, lps = 0.0f;
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const float s0 = tn_raw_scale(raw[d]);
        sig[d] = fmaxf(s0, TN_SCALE_LB);
        dsdr[d] = tn_scale_slope(raw[d], s0);
        const float h = 0.5f * (a.high[d] - a.low[d]), logh = logf(h), logs = logf(sig[d]);
        // log-probability of the recorded action through the inverse transform
        const float y = tn_clamp((ac[d] - a.low[d]) / h - 1.0f);
        const float x = 0.5f * (log1pf(y) - log1pf(-y));
        q[d] = (x - loc[d]) / sig[d];
        const float lpd = tn_log_density(q[d], logs, x) - logh;
        lp = d ? lp + lpd : lpd;
        // the entropy sample (never clamped: actor_distribution's expression)
        xs[d] = loc[d] + sig[d] * z[d];
        const float lpsd = tn_log_density(z[d], logs, xs[d]) - logh;
        lps = d ? lps + lpsd : lpsd;
      }
      const float lw = lp - old;
      const float cl = fminf(fmaxf(lw, a.log_lo), a.log_hi);
      const float g1 = expf(lw) * A, g2 = expf(cl) * A;
      const float dlw = g1 <= g2 ? g1 : 0.0f;  // on a tie the unclamped branch carries the gradient; the clamped branch of a strict minimum is flat (lw outside the band)
      const float e = v - vt, ae = fabsf(e);
      t[0] = fminf(g1, g2);
      t[1] = lps;
      t[2] = ae < 1.0f ? 0.5f * e * e : ae - 0.5f;
      t[3] = cl != lw ? 1.0f : 0.0f;
      t[4] = -lw;
      const float wobj = -a.inv * dlw;
      float dl[2], dr[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const float th2 = 2.0f * tanhf(xs[d]);  // d logp' / d x' = 2 tanh(x')
        dl[d] = wobj * (q[d] / sig[d]) + a.ce_inv * th2;
        const float dsig = wobj * ((q[d] * q[d] - 1.0f) / sig[d]) + a.ce_inv * (th2 * z[d] - 1.0f / sig[d]);
        dr[d] = dsig * dsdr[d];
      }
      d4 = make_float4(dl[0], dl[1], dr[0], dr[1]);
      if (n == 0) {  // d loss_critic / d value[m]: the frame's agents in order
        float s = 0.0f;
        for (int i = 0; i < a.N; ++i) s = s + fminf(fmaxf(v - a.vtarget[(long long)f * a.N + i], -1.0f), 1.0f);
        a.dout_critic[m] = a.cc_inv * s;
      }
    } else if (n == 0) {
      a.dout_critic[m] = 0.0f;
    }
    reinterpret_cast<float4*>(a.dout_actor)[r] = d4;
  }
#pragma unroll
  for (int k = 0; k < PPO_SUMS; ++k) {
    const float s = wave_sum(t[k]);
    if ((tid & 63) == 0) wsum[k][tid >> 6] = s;
  }
  __syncthreads();
  if (tid < PPO_SUMS) a.partial[(size_t)tid * a.groups + blockIdx.x] = ((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3];
}

// the 1-D head: `action` = the recorded scores [F, N], `out` / `dout_actor` [M, N, 2]; low / high are not read
__global__ void __launch_bounds__(256) sigmaenv_ppo_head_1d_kernel(HeadArgs a) {
  sigma_poison_lds();
  __shared__ float wsum[PPO_SUMS][4];
  const int tid = threadIdx.x;
  const long long r = (long long)blockIdx.x * blockDim.x + tid, R = (long long)a.M * a.N;
  float t[PPO_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (r < R) {
    const int m = (int)(r / a.N), n = (int)(r - (long long)m * a.N);
    const int f = a.index[m];
    float2 d2 = make_float2(0.f, 0.f);
    if ((unsigned)f < (unsigned)a.F) {  // (an entry outside the records is never an address: the row contributes zeros)
      const long long fr = (long long)f * a.N + n;
      const float2 o = reinterpret_cast<const float2*>(a.out)[r];
      const float score = a.action[fr], old = a.old_logp[fr], A = a.adv[fr], vt = a.vtarget[fr], v = a.value[m];
      const float z = rng_normal_cos(a.seed, a.counter, (uint32_t)f, (uint32_t)n, DRAW_PRIORITY_ENTROPY);
      const float loc = o.x, s0 = tn_raw_scale(o.y), sig = fmaxf(s0, TN_SCALE_LB), dsdr = tn_scale_slope(o.y, s0), logs = logf(sig);
      // log-probability of the recorded score through the inverse transform: the score IS the clamped tanh (no affine map)
      const float y = tn_clamp(score);
      const float x = 0.5f * (log1pf(y) - log1pf(-y));
      const float q = (x - loc) / sig;
      const float lp = tn_log_density(q, logs, x);
      // the entropy sample (never clamped)
      const float xs = loc + sig * z;
      const float lps = tn_log_density(z, logs, xs);
      const float lw = lp - old;
      const float cl = fminf(fmaxf(lw, a.log_lo), a.log_hi);
      const float g1 = expf(lw) * A, g2 = expf(cl) * A;
      const float dlw = g1 <= g2 ? g1 : 0.0f;  // on a tie the unclamped branch carries the gradient
      const float e = v - vt, ae = fabsf(e);
      t[0] = fminf(g1, g2);
      t[1] = lps;
      t[2] = ae < 1.0f ? 0.5f * e * e : ae - 0.5f;
      t[3] = cl != lw ? 1.0f : 0.0f;
      t[4] = -lw;
      const float wobj = -a.inv * dlw;
      const float th2 = 2.0f * tanhf(xs);  // d logp' / d x' = 2 tanh(x')
      const float dl = wobj * (q / sig) + a.ce_inv * th2;
      const float dsig = wobj * ((q * q - 1.0f) / sig) + a.ce_inv * (th2 * z - 1.0f / sig);
      d2 = make_float2(dl, dsig * dsdr);
      if (n == 0) {  // d loss_critic / d value[m]: the frame's agents in order
        float s = 0.0f;
        for (int i = 0; i < a.N; ++i) s = s + fminf(fmaxf(v - a.vtarget[(long long)f * a.N + i], -1.0f), 1.0f);
        a.dout_critic[m] = a.cc_inv * s;
      }
    } else if (n == 0) {
      a.dout_critic[m] = 0.0f;
    }
    reinterpret_cast<float2*>(a.dout_actor)[r] = d2;
  }
#pragma unroll
  for (int k = 0; k < PPO_SUMS; ++k) {
    const float s = wave_sum(t[k]);
    if ((tid & 63) == 0) wsum[k][tid >> 6] = s;
  }
  __syncthreads();
  if (tid < PPO_SUMS) a.partial[(size_t)tid * a.groups + blockIdx.x] = ((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3];
}

// result[0 .. 5] = loss_objective, loss_entropy, loss_critic, entropy, clip_fraction, kl_approx; [6], [7] = 0.  One wavefront.
__global__ void __launch_bounds__(64) sigmaenv_ppo_sum_kernel(const float* __restrict__ partial, int groups, float inv, float entropy_coeff, float critic_coeff,
                                                              float* __restrict__ result) {
  sigma_poison_lds();
  const int lane = threadIdx.x;
  float s[PPO_SUMS];
#pragma unroll
  for (int k = 0; k < PPO_SUMS; ++k) {
    float v = 0.0f;
    for (int g = lane; g < groups; g += 64) v = v + partial[(size_t)k * groups + g];
    s[k] = wave_sum(v);
  }
  if (lane == 0) {
    const float entropy = -(s[1] * inv);
    result[0] = -(s[0] * inv);
    result[1] = -(entropy_coeff * entropy);
    result[2] = critic_coeff * (s[2] * inv);
    result[3] = entropy;
    result[4] = s[3] * inv;
    result[5] = s[4] * inv;
    result[6] = 0.0f;
    result[7] = 0.0f;
  }
}

}  // namespace ppo

extern "C" int sigmaenv_ppo_head(sigmaenv_t* h, const sigmaenv_ppo_head_args_t* a) {
  if (!h || !a) return SIGMAENV_EINVAL;
  if (a->n_index < 1 || a->n_frames < 1) { h->err = "ppo_head: at least one minibatch slot and one frame"; return SIGMAENV_EINVAL; }
  if ((long long)a->n_index * h->N > 0x7FFFFFFFll) { h->err = "ppo_head: more than 2^31 - 1 rows"; return SIGMAENV_EINVAL; }
  const void* ptrs[] = {a->index, a->out, a->value, a->action, a->sample_log_prob, a->advantage, a->value_target, a->dout_actor, a->dout_critic, a->result, a->workspace};
  for (const void* p : ptrs)
    if (!p || ((uintptr_t)p & 3)) { h->err = "ppo_head: a null tensor or one that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  if (((uintptr_t)a->out & 15) || ((uintptr_t)a->dout_actor & 15) || ((uintptr_t)a->action & 7)) {
    h->err = "ppo_head: out / dout_actor must be 16-byte aligned, action 8-byte aligned";
    return SIGMAENV_EINVAL;
  }
  if (!(a->clip_epsilon > 0.0f && a->clip_epsilon < 1.0f) || !(a->high[0] > a->low[0]) || !(a->high[1] > a->low[1])) {
    h->err = "ppo_head: clip_epsilon must be in (0, 1) and high > low";
    return SIGMAENV_EINVAL;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const long long R = (long long)a->n_index * h->N;
  ppo::HeadArgs k{};
  k.index = a->index; k.out = a->out; k.value = a->value; k.action = a->action; k.old_logp = a->sample_log_prob; k.adv = a->advantage; k.vtarget = a->value_target;
  k.dout_actor = a->dout_actor; k.dout_critic = a->dout_critic; k.partial = a->workspace;
  k.M = a->n_index; k.N = h->N; k.F = a->n_frames; k.groups = (int)((R + 255) / 256);
  for (int d = 0; d < 2; ++d) { k.low[d] = a->low[d]; k.high[d] = a->high[d]; }
  k.log_lo = (float)std::log1p(-(double)a->clip_epsilon);
  k.log_hi = (float)std::log1p((double)a->clip_epsilon);
  k.inv = 1.0f / (float)R;
  k.ce_inv = a->entropy_coeff * k.inv;
  k.cc_inv = a->critic_coeff * k.inv;
  k.seed = a->seed; k.counter = a->counter;
  hipLaunchKernelGGL(ppo::sigmaenv_ppo_head_kernel, dim3((unsigned)k.groups), dim3(256), 0, h->stream, k);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(ppo::sigmaenv_ppo_sum_kernel, dim3(1), dim3(64), 0, h->stream, (const float*)a->workspace, k.groups, k.inv, a->entropy_coeff, a->critic_coeff, a->result);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_ppo_head_1d(sigmaenv_t* h, const sigmaenv_ppo_head_1d_args_t* a) {
  if (!h || !a) return SIGMAENV_EINVAL;
  if (a->n_index < 1 || a->n_frames < 1) { h->err = "ppo_head_1d: at least one minibatch slot and one frame"; return SIGMAENV_EINVAL; }
  if ((long long)a->n_index * h->N > 0x7FFFFFFFll) { h->err = "ppo_head_1d: more than 2^31 - 1 rows"; return SIGMAENV_EINVAL; }
  const void* ptrs[] = {a->index, a->out, a->value, a->scores, a->score_log_prob, a->advantage, a->value_target, a->dout_actor, a->dout_critic, a->result, a->workspace};
  for (const void* p : ptrs)
    if (!p || ((uintptr_t)p & 3)) { h->err = "ppo_head_1d: a null tensor or one that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  if (((uintptr_t)a->out & 7) || ((uintptr_t)a->dout_actor & 7)) { h->err = "ppo_head_1d: out / dout_actor must be 8-byte aligned"; return SIGMAENV_EINVAL; }
  if (!(a->clip_epsilon > 0.0f && a->clip_epsilon < 1.0f)) { h->err = "ppo_head_1d: clip_epsilon must be in (0, 1)"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  const long long R = (long long)a->n_index * h->N;
  ppo::HeadArgs k{};
  k.index = a->index; k.out = a->out; k.value = a->value; k.action = a->scores; k.old_logp = a->score_log_prob; k.adv = a->advantage; k.vtarget = a->value_target;
  k.dout_actor = a->dout_actor; k.dout_critic = a->dout_critic; k.partial = a->workspace;
  k.M = a->n_index; k.N = h->N; k.F = a->n_frames; k.groups = (int)((R + 255) / 256);
  k.log_lo = (float)std::log1p(-(double)a->clip_epsilon);
  k.log_hi = (float)std::log1p((double)a->clip_epsilon);
  k.inv = 1.0f / (float)R;
  k.ce_inv = a->entropy_coeff * k.inv;
  k.cc_inv = a->critic_coeff * k.inv;
  k.seed = a->seed; k.counter = a->counter;
  hipLaunchKernelGGL(ppo::sigmaenv_ppo_head_1d_kernel, dim3((unsigned)k.groups), dim3(256), 0, h->stream, k);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(ppo::sigmaenv_ppo_sum_kernel, dim3(1), dim3(64), 0, h->stream, (const float*)a->workspace, k.groups, k.inv, a->entropy_coeff, a->critic_coeff, a->result);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}
