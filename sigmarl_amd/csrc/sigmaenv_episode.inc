// sigmaenv_episode.inc -- the episode return of a rollout's records and its done-frame mean, on the records where they lie (included by sigmaenv.hip after
// sigmaenv_episode.h, which states the arithmetic; the contract is in include/sigmaenv.h, sigmaenv_episode_return).
//
// What it restates: torchrl's RewardSum as sigmarl/mappo_cavs.py:178-183 wraps the env in it and episode_reward[done].mean() of _log_and_save (:468-478).
//
// Mapping.  The recurrence is sequential in t and independent over (env, agent): one lane per (env, agent) walks t upwards, as sigmaenv_gae walks it downwards, and
// the loads of EPR_UNROLL steps are issued before the first of them is used (the recurrence itself is one addition and one select per step: the launch is bound by
// the latency of those loads, not by bandwidth -- a lane reads 8 of every 4 (N*(D+1)+1) record bytes).  A done frame's sum runs over the env's agents in order,
// so the lanes of one env lie in ONE wavefront: a wavefront holds G = 64 / N whole envs in its lanes 0 .. G N - 1 (the others idle: none at N = 16, one at N = 3,
// up to 31 at N = 33) and fetches the agents' E with cross-lane moves -- no LDS, no workgroup barrier inside the walk, and only in the steps where one of its envs
// is done.  The N lanes of an env read N consecutive floats of a row whose width is odd: the G segments of a wavefront's load are unaligned whatever the mapping;
// the record's writes (lane e at E + e) are consecutive over the wavefront's active lanes.  Each env's lane of agent 0 keeps the env's sum and count in registers
// and writes them once; sigmaenv_episode_sum_kernel, one workgroup, adds them in the header's order.  No atomics; the shape of every sum is a function of
// (T, B, N) alone.  -ffp-contract=off (Makefile): every operator is one IEEE fp32 operation.

namespace episode {

#define EPR_UNROLL 8
#define EPR_FETCH 8  // cross-lane moves issued before the first of them is used (one at a time, a done frame of 16 agents waits 16 LDS round trips in a row)

__global__ void __launch_bounds__(256) sigmaenv_episode_walk_kernel(const float* __restrict__ slab, long long slab_stride, int T, int B, int N, int D, int G,
                                                                    float* __restrict__ carry, float* __restrict__ out, float* __restrict__ env_sum,
                                                                    int32_t* __restrict__ env_cnt) {
  sigma_poison_lds();
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int g = lane / N, i = lane - g * N;
  const long long bl = wave * G + g;
  const bool on = g < G && bl < B;  // (no lane leaves early: the cross-lane moves below need the whole wavefront)
  const long long b = on ? bl : 0;
  const int first = (g * N) & 63;   // the lane of the env's agent 0
  const long long W = (long long)N * (D + 1) + 1;
  const float* row = slab + b * W + (long long)N * D;  // the env's [N reward | done] tail in block 0
  float c = on ? carry[b * N + i] : 0.0f;
  float s = 0.0f;
  int32_t k = 0;
  for (int t0 = 0; t0 < T; t0 += EPR_UNROLL) {
    float r[EPR_UNROLL] = {}, dn[EPR_UNROLL] = {};
#pragma unroll
    for (int u = 0; u < EPR_UNROLL; ++u) {
      const int t = t0 + u;
      if (on && t < T) {
        const float* p = row + (long long)t * slab_stride;
        r[u] = p[i]; dn[u] = p[N];
      }
    }
#pragma unroll
    for (int u = 0; u < EPR_UNROLL; ++u) {
      const int t = t0 + u;
      if (t < T) {
        const float E = epr_add(c, r[u]);
        if (on && out) out[((long long)t * B + b) * N + i] = E;
        const bool d = on && dn[u] != 0.0f;
        if (__any(d)) {  // the same in every lane of the wavefront
          float x = 0.0f;  // epr_frame_sum, the E of agent j from the lane that holds it: EPR_FETCH moves in flight, then their additions in order
          for (int j0 = 0; j0 < N; j0 += EPR_FETCH) {
            float v[EPR_FETCH];
#pragma unroll
            for (int q = 0; q < EPR_FETCH; ++q) v[q] = __shfl(E, (first + j0 + q) & 63);
#pragma unroll
            for (int q = 0; q < EPR_FETCH; ++q)
              if (j0 + q < N) x = x + v[q];
          }
          if (d) { s = s + x; k = k + 1; }
        }
        c = epr_carry(E, dn[u]);
      }
    }
  }
  if (on) {
    carry[b * N + i] = c;
    if (i == 0) { env_sum[b] = s; env_cnt[b] = k; }
  }
}

// S, K and the mean from the envs' sums and counts: ONE workgroup of EPR_LANES lanes, the order of sigmaenv_episode.h
__global__ void __launch_bounds__(EPR_LANES) sigmaenv_episode_sum_kernel(const float* __restrict__ env_sum, const int32_t* __restrict__ env_cnt, int B, int N,
                                                                         float* __restrict__ result) {
  sigma_poison_lds();
  __shared__ float ws[4];
  __shared__ int32_t wk[4];
  const int tid = threadIdx.x;
  float v = epr_lane_sum(env_sum, B, tid);
  int32_t n = epr_lane_count(env_cnt, B, tid);
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    v = v + __shfl_xor(v, m);
    n = n + __shfl_xor(n, m);
  }
  if ((tid & 63) == 0) { ws[tid >> 6] = v; wk[tid >> 6] = n; }
  __syncthreads();
  if (tid == 0) {
    const float S = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    const int32_t K = ((wk[0] + wk[1]) + wk[2]) + wk[3];
    result[0] = epr_mean(S, K, N);
    result[1] = S;
    result[2] = (float)K;
    result[3] = 0.0f;
  }
}

}  // namespace episode

extern "C" int sigmaenv_episode_return(sigmaenv_t* h, const sigmaenv_episode_args_t* a) {
  if (!h || !a) return SIGMAENV_EINVAL;
  if (a->n_steps < 1 || !a->slab || !a->carry || !a->result) { h->err = "episode_return: n_steps >= 1, slab, carry and result are required"; return SIGMAENV_EINVAL; }
  if ((long long)a->n_steps * h->B >= (long long)EPR_MAX_FRAMES) { h->err = "episode_return: n_steps * B must stay below 2^24 (the done-frame count is a float)"; return SIGMAENV_EINVAL; }
  const long long W = (long long)h->N * (h->D + 1) + 1, own = (long long)h->B * W;
  if (a->slab_stride != 0 && a->slab_stride < own) { h->err = "episode_return: slab_stride below the handle's own record block B * (N * (D + 1) + 1)"; return SIGMAENV_EINVAL; }
  const void* ptrs[] = {a->slab, a->carry, a->result, a->episode_reward};
  for (const void* p : ptrs)
    if ((uintptr_t)p & 3) { h->err = "episode_return: a tensor that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  const long long stride = a->slab_stride ? a->slab_stride : own;
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->episode_ws) {  // the envs' sums [B] f32, then their counts [B] i32
    const int rc = dev_alloc(h, (void**)&h->episode_ws, 2 * (size_t)h->B * sizeof(float), true);
    if (rc) return rc;
  }
  float* env_sum = h->episode_ws;
  int32_t* env_cnt = (int32_t*)(h->episode_ws + h->B);
  const int G = 64 / h->N;  // whole envs per wavefront (N <= SIGMAENV_MAX_AGENTS = 64)
  const long long waves = ((long long)h->B + G - 1) / G;
  hipLaunchKernelGGL(episode::sigmaenv_episode_walk_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, h->stream, a->slab, stride, (int)a->n_steps, h->B, h->N, h->D, G,
                     a->carry, a->episode_reward, env_sum, env_cnt);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(episode::sigmaenv_episode_sum_kernel, dim3(1), dim3(EPR_LANES), 0, h->stream, (const float*)env_sum, (const int32_t*)env_cnt, h->B, h->N, a->result);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}
