// sigmaenv_opponent_fill.inc -- opponent modelling's gather into the placeholder columns of the observation row (SIGMAENV_OBS_OPPONENT_PAD).
// (The rows of the non-default observation switches themselves are assembled by observe_tile_variant in sigmaenv.hip, inside every kernel that refreshes
// observations -- the fused step and its T-step loop incl. the rollout record, the resets, sigmaenv_observe.)
namespace obsvar {

// opponent_modeling's gather (helper_training.py:1117-1137): obs[b, i, -(K - k) * 2 : +2] = actions[b, nearing[b, i, k]]; one lane per (env, agent, k).
// rec (optional, [B, N, K, 2]): the same pairs once more (the rollout's record of what the policy saw, sigmaenv_rollout_f32_ex)
__global__ void __launch_bounds__(256) sigmaenv_opponent_fill_kernel(float* __restrict__ obs, int D, const int32_t* __restrict__ nearing, const float* __restrict__ actions, int B, int N, int K,
                                                                     float* __restrict__ rec) {
  sigma_poison_lds();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * N * K) return;
  const size_t bi = t / K;
  const int k = (int)(t - bi * K);
  const size_t b = bi / N;
  const int j = nearing[t];
  const float2 a = reinterpret_cast<const float2*>(actions)[b * N + j];
  float* dst = obs + bi * D + (D - 2 * (K - k));
  dst[0] = a.x;
  dst[1] = a.y;
  if (rec) reinterpret_cast<float2*>(rec)[t] = a;
}

}  // namespace obsvar
