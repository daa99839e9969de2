// sigmaenv_wrappers.inc -- the policy wrappers of the training collector in the device rollout (included by sigmaenv.hip after sigmaenv_mlp32.inc).
//
// What it restates (include/sigmaenv.h, sigmaenv_rollout_f32_ex):
//   opponent modelling              opponent_modeling, sigmarl/helper_training.py:1071-1142: policy -> neighbours' tentative actions into the placeholder
//                                   columns (sigmaenv_opponent_fill_kernel) -> policy again
//   prioritized action propagation  prioritized_ap_policy, helper_training.py:1162-1315, with the priority module of sigmarl/modules/priority_module.py: agents
//                                   ranked by a priority score act one at a time, each seeing the actions its observed neighbours have already chosen
// Both run inside rollout_loop (sigmaenv_actor.inc) as its policy hook, so the step, the record and the resets are the plain rollout's.
//
// Mapping.  The reference runs prioritized propagation as N + 1 network passes over all B x N rows per step and keeps one agent per env from each.  Here turn k
// gathers just the B rows that act (one per env: rank k) into a compact [B, obs_dim + 2 K] buffer and runs the fp32 actor on those; the head maps network row
// b back to agent row b * N + rank[b, k] (Mlp32sHead::row_map), which both places the outputs and keys the random draw, so the turn's sample is the one a
// full-batch forward would give that row.  A turn is B / 64 workgroups of the network kernel: the turns are launch-bound at the batch sizes of a rollout
// (tools/wrapper_timing.py).

namespace wrap {

// NormalParamExtractor + 1-D TanhNormal on [-1, 1] of the priority actor (priority_module.py:34-66), one agent row; `out2` = (loc, raw scale).  With the
// trivial bounds torchrl applies no affine map: the score is the clamped tanh itself (the head of sigmaenv_dist.h in one dimension).
__global__ void __launch_bounds__(256) sigmaenv_priority_head_kernel(const float* __restrict__ out2, int R, int n_agents, int env_base, float* __restrict__ scores,
                                                                     float* __restrict__ log_prob, uint64_t seed, uint64_t counter, int deterministic) {
  sigma_poison_lds();
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= R) return;
  const float2 o = reinterpret_cast<const float2*>(out2)[row];
  const float sc = tn_scale(o.y);
  float z = 0.0f;
  if (!deterministic) {  // the cosine branch of a normal pair of the env's counter-based generator
    const uint32_t env = (uint32_t)(env_base + row / n_agents), agent = (uint32_t)(row - (row / n_agents) * n_agents);
    z = rng_normal_cos(seed, counter, env, agent, DRAW_PRIORITY);
  }
  const float x = o.x + sc * z;
  scores[row] = tn_squash(x);
  if (log_prob) log_prob[row] = tn_log_density(z, logf(sc), x);
}

// rank_agents (priority_module.py:118-135): position of agent i in env b = the number of agents that sort before it (higher score, or equal score and lower
// index: a stable descending order; NaN below everything).  One lane per (env, agent); every position of a row is written exactly once.
__global__ void __launch_bounds__(256) sigmaenv_priority_rank_kernel(const float* __restrict__ scores, int B, int N, int32_t* __restrict__ ranks) {
  sigma_poison_lds();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * N) return;
  const size_t b = t / N;
  const int i = (int)(t - b * N);
  const float* s = scores + b * N;
  auto key = [](float v) { return v != v ? -INFINITY : v; };
  const float si = key(s[i]);
  int pos = 0;
  for (int j = 0; j < N; ++j) {
    const float sj = key(s[j]);
    pos += (sj > si) || (sj == si && j < i);
  }
  ranks[b * N + pos] = i;
}

// prioritization_method "random" (priority_module.py:147-153): inside-out Fisher-Yates, one lane per env (position i draws j uniform in [0, i])
__global__ void __launch_bounds__(256) sigmaenv_priority_random_kernel(int B, int N, int env_base, uint64_t seed, uint64_t counter, int32_t* __restrict__ ranks) {
  sigma_poison_lds();
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int32_t* r = ranks + (size_t)b * N;
  for (int i = 0; i < N; ++i) {
    const int j = (int)rng_below(rng_u32(seed, counter, (uint32_t)(env_base + b), (uint32_t)i, DRAW_SHUFFLE), (uint32_t)(i + 1));
    if (j != i) r[i] = r[j];
    r[j] = i;
  }
}

// turn k of prioritized action propagation: compact[b, :] = the base observation of agent i = ranks[b, k] (its SIGMAENV_BUF_OBS row, then 2 K columns with the
// current actions of its observed neighbours: `actions` is zero for those that have not acted, as combined_action, helper_training.py:1219-1300);
// row_map[b] = b N + i (-1 when ranks holds no agent index).  rec (optional, [B, N, K, 2]): the neighbour actions agent i saw.  base_rec (optional,
// [B, N, D + 2 K]): the whole compact row at agent i's place -- the base observation a learner trains the actor on; one more store per gathered element, coalesced
// over the row as the compact one is.  One lane per (env, column).
//
// The body is one template; sigmaenv_turn_gather_kernel is its noise-free instantiation under the signature it always had, sigmaenv_turn_gather_noise_kernel the noisy one.
// NOISE (is_communication_noise, helper_training.py:1271-1287; K = 2): every one of the 2 K columns -- the zero of an undecided neighbour and the column of a
// neighbour index that is no agent included -- is seen as comm_noise_seen(v, std of its position, z) (sigmaenv_dist.h), z drawn per (env, acting agent, step,
// column).  compact, rec and base_rec take the noisy value: the actor is evaluated on it and the learner trains on it.  `actions` is only read, so the step and the
// later turns' gathers get the clean actions (combined_action).  The stds: std_env[b] = (s_v, s_d) of env b when given, else the launch's pair.
struct TurnNoise {
  float s_v, s_d;
  const float* std_env;  // optional [B, 2]
  uint64_t seed, counter;
  int env_base;
};

static_assert(COMM_NOISE_MAX_COLUMNS == 2u * SIGMAENV_MAX_NEARING, "the draw ids reserved for communication noise are those of 2 K columns at the largest K");

template <bool NOISE>
__device__ __forceinline__ void turn_gather(const float* __restrict__ obs, int D, const int32_t* __restrict__ nearing, int K, const float* __restrict__ actions,
                                            const int32_t* __restrict__ ranks, int k, int B, int N, float* __restrict__ compact, int32_t* __restrict__ row_map,
                                            float* __restrict__ rec, float* __restrict__ base_rec, const TurnNoise& nz) {
  sigma_poison_lds();
  const int Dc = D + 2 * K;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * Dc) return;
  const size_t b = t / Dc;
  const int c = (int)(t - b * Dc);
  const int i = ranks[b * N + k];
  const bool ok = i >= 0 && i < N;
  if (c == 0) row_map[b] = ok ? (int32_t)(b * N + i) : -1;
  float v = 0.0f;
  if (ok) {
    const size_t bi = b * N + i;
    if (c < D) {
      v = obs[bi * D + c];
    } else {
      const int q = c - D, j = q >> 1;
      const int n = nearing[bi * K + j];
      if (n >= 0 && n < N) v = actions[(b * N + n) * 2 + (q & 1)];
      if (NOISE) {
        float s_v = nz.s_v, s_d = nz.s_d;
        if (nz.std_env) {
          const float2 s = reinterpret_cast<const float2*>(nz.std_env)[b];
          s_v = s.x;
          s_d = s.y;
        }
        const float z = rng_normal_cos(nz.seed, nz.counter, (uint32_t)(nz.env_base + (int)b), (uint32_t)i, DRAW_COMM_NOISE + 2u * (uint32_t)q);
        v = comm_noise_seen(v, comm_noise_std(q, s_v, s_d), z);
      }
      if (rec) rec[(bi * K + j) * 2 + (q & 1)] = v;
    }
    if (base_rec) base_rec[bi * Dc + c] = v;
  }
  compact[t] = v;
}

__global__ void __launch_bounds__(256) sigmaenv_turn_gather_kernel(const float* __restrict__ obs, int D, const int32_t* __restrict__ nearing, int K, const float* __restrict__ actions,
                                                                   const int32_t* __restrict__ ranks, int k, int B, int N, float* __restrict__ compact, int32_t* __restrict__ row_map,
                                                                   float* __restrict__ rec, float* __restrict__ base_rec) {
  turn_gather<false>(obs, D, nearing, K, actions, ranks, k, B, N, compact, row_map, rec, base_rec, TurnNoise{});
}

__global__ void __launch_bounds__(256) sigmaenv_turn_gather_noise_kernel(const float* __restrict__ obs, int D, const int32_t* __restrict__ nearing, int K, const float* __restrict__ actions,
                                                                         const int32_t* __restrict__ ranks, int k, int B, int N, float* __restrict__ compact, int32_t* __restrict__ row_map,
                                                                         float* __restrict__ rec, float* __restrict__ base_rec, TurnNoise nz) {
  turn_gather<true>(obs, D, nearing, K, actions, ranks, k, B, N, compact, row_map, rec, base_rec, nz);
}

}  // namespace wrap

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int wrap_workspace(sigmaenv_t* h, size_t bytes) {
  if (h->wrap_ws && h->wrap_ws_bytes >= bytes) return SIGMAENV_OK;
  dev_free(h, h->wrap_ws);
  h->wrap_ws = nullptr;
  h->wrap_ws_bytes = 0;
  const int rc = dev_alloc(h, &h->wrap_ws, bytes, true);
  if (rc) return rc;
  h->wrap_ws_bytes = bytes;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_priority_rank(sigmaenv_t* h, const float* scores, int32_t* ranks) {
  if (!h || !scores || !ranks) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->B * h->N;
  hipLaunchKernelGGL(wrap::sigmaenv_priority_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, scores, h->B, h->N, ranks);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_priority_random(sigmaenv_t* h, uint64_t seed, uint64_t counter, int32_t* ranks) {
  if (!h || !ranks) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(wrap::sigmaenv_priority_random_kernel, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->B, h->N, h->cfg.env_index_base, seed, counter, ranks);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_priority_forward(sigmaenv_t* h, sigmaenv_mlp32* pm, const float* obs, float* scratch, float* scores, float* log_prob, int32_t* ranks,
                                         uint64_t seed, uint64_t counter, int32_t deterministic) {
  if (!h || !pm || !scratch || !scores || pm->out_dim != 2 || (!obs && pm->in_dim != h->D)) {
    if (h) h->err = "priority_forward: a network with 2 outputs (loc, scale) on the observation width, scratch and scores are required";
    return SIGMAENV_EINVAL;
  }
  const int R = h->B * h->N;
  int rc = mlp32_forward_impl(h, pm, obs ? obs : h->buf.obs, R, scratch, nullptr, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(wrap::sigmaenv_priority_head_kernel, dim3((R + 255) / 256), dim3(256), 0, h->stream, scratch, R, h->N, h->cfg.env_index_base, scores, log_prob, seed, counter,
                     (int)deterministic);
  HIPCHK(h, hipGetLastError());
  return ranks ? sigmaenv_priority_rank(h, scores, ranks) : SIGMAENV_OK;
}

extern "C" int sigmaenv_rollout_f32_ex(sigmaenv_t* h, sigmaenv_mlp32* m, const float* low, const float* high, float* scratch, int32_t n_steps, float* actions_buf,
                                       float* slab_base, float* logp_base, float* actions_rec, uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count,
                                       int32_t deterministic, const sigmaenv_rollout_opts_t* opts) {
  const int wrapper = opts ? opts->wrapper : SIGMAENV_WRAP_PLAIN;
  // communication noise: all zero (what a caller from before the fields existed passes as reserved[4]) means off
  const bool noise = opts && (opts->comm_noise_std[0] != 0.0f || opts->comm_noise_std[1] != 0.0f || opts->comm_noise_std_env);
  if (noise) {
    if (!h) return SIGMAENV_EINVAL;
    if (wrapper != SIGMAENV_WRAP_PRIORITIZED) {
      h->err = "rollout_f32_ex: communication noise acts on the propagated actions of SIGMAENV_WRAP_PRIORITIZED only";
      return SIGMAENV_EINVAL;
    }
    if (h->cfg.n_nearing != 2) {
      h->err = "rollout_f32_ex: communication noise needs n_nearing == 2 (its 4 stds fit 2 K = 4 columns only: raises in the reference as well)";
      return SIGMAENV_EINVAL;
    }
    for (int d = 0; d < 2; ++d)
      if (!(opts->comm_noise_std[d] >= 0.0f) || isinf(opts->comm_noise_std[d])) {
        h->err = "rollout_f32_ex: comm_noise_std must be finite and >= 0";
        return SIGMAENV_EINVAL;
      }
  }
  if (wrapper == SIGMAENV_WRAP_PLAIN)
    return sigmaenv_rollout_f32(h, m, low, high, scratch, n_steps, actions_buf, slab_base, logp_base, actions_rec, seed, counter0, path_first, path_count, deterministic);
  if (!h || !m || !low || !high || !scratch || !actions_buf || n_steps < 1 || m->out_dim != 4) return SIGMAENV_EINVAL;
  if (wrapper != SIGMAENV_WRAP_OPPONENT && wrapper != SIGMAENV_WRAP_PRIORITIZED) { h->err = "rollout_f32_ex: wrapper must be 0 (plain), 1 (opponent) or 2 (prioritized)"; return SIGMAENV_EINVAL; }
  if (h->cfg.rew_flags & (SIGMAENV_REW_CBF | SIGMAENV_REW_CBF_QP)) {
    h->err = "rollout_f32_ex: a policy wrapper on a handle with a \"cbf\" rew_method -- the collector runs CBF training OR opponent modelling OR prioritized propagation, never two";
    return SIGMAENV_EINVAL;
  }
  const int B = h->B, N = h->N, K = h->cfg.n_nearing, D = h->D;
  const size_t BN = (size_t)B * N;
  auto align = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  HIPCHK(h, hipSetDevice(h->device));
  if (wrapper == SIGMAENV_WRAP_OPPONENT) {
    if (!(h->cfg.obs_flags & SIGMAENV_OBS_OPPONENT_PAD)) { h->err = "rollout_f32_ex: opponent modelling needs the placeholder columns (SIGMAENV_OBS_OPPONENT_PAD)"; return SIGMAENV_EINVAL; }
    if (m->in_dim != D) { h->err = "rollout_f32_ex: the actor's input width is not the handle's obs_dim"; return SIGMAENV_EINVAL; }
    int rc = wrap_workspace(h, align(BN * 2 * sizeof(float)));
    if (rc) return rc;
    float* tent = (float*)h->wrap_ws;
    const uint64_t seed_tent = seed ^ (1ull << 63);
    return rollout_loop(h, [&](int t, float* act, float* logp) {
      int r = actor_rows_f32(h, m, h->buf.obs, (int)BN, nullptr, scratch, low, high, tent, nullptr, nullptr, seed_tent, counter0 + (uint64_t)t, deterministic);
      if (!r) r = opponent_fill_impl(h, tent, opts->tentative_rec ? opts->tentative_rec + (size_t)t * BN * K * 2 : nullptr);
      if (!r) r = actor_rows_f32(h, m, h->buf.obs, (int)BN, nullptr, scratch, low, high, act, logp, nullptr, seed, counter0 + (uint64_t)t, deterministic);
      return r;
    }, n_steps, actions_buf, slab_base, logp_base, actions_rec, seed, counter0, path_first, path_count);
  }
  // prioritized action propagation
  const int Dc = D + 2 * K, src = opts->priority_source;
  if (m->in_dim != Dc) { h->err = "rollout_f32_ex: the prioritized actor takes obs_dim + 2 n_nearing inputs (the base observation)"; return SIGMAENV_EINVAL; }
  if (src == SIGMAENV_PRIORITY_NET) {
    if (!opts->priority_net || opts->priority_net->in_dim != D || opts->priority_net->out_dim != 2) {
      h->err = "rollout_f32_ex: SIGMAENV_PRIORITY_NET needs a priority network obs_dim -> ... -> 2";
      return SIGMAENV_EINVAL;
    }
  } else if (src == SIGMAENV_PRIORITY_GIVEN) {
    if (!opts->ranks_given) { h->err = "rollout_f32_ex: SIGMAENV_PRIORITY_GIVEN needs ranks_given"; return SIGMAENV_EINVAL; }
  } else if (src != SIGMAENV_PRIORITY_RANDOM) {
    h->err = "rollout_f32_ex: priority_source must be 0 (network), 1 (random) or 2 (given)";
    return SIGMAENV_EINVAL;
  }
  // workspace: compact rows [B, Dc] | row map [B] | ranks [B, N] | scores [B, N] | score log-probabilities [B, N]
  const size_t o_map = align((size_t)B * Dc * sizeof(float)), o_rank = o_map + align((size_t)B * 4), o_score = o_rank + align(BN * 4), o_slp = o_score + align(BN * 4);
  int rc = wrap_workspace(h, o_slp + align(BN * 4));
  if (rc) return rc;
  char* ws = (char*)h->wrap_ws;
  float* compact = (float*)ws;
  int32_t* row_map = (int32_t*)(ws + o_map);
  return rollout_loop(h, [&](int t, float* act, float* logp) {
    const uint64_t ctr = counter0 + (uint64_t)t;
    const int32_t* ranks = opts->ranks_given;
    if (src != SIGMAENV_PRIORITY_GIVEN) {
      int32_t* rk = opts->rank_rec ? opts->rank_rec + (size_t)t * BN : (int32_t*)(ws + o_rank);
      int r = SIGMAENV_OK;
      if (src == SIGMAENV_PRIORITY_RANDOM) {
        r = sigmaenv_priority_random(h, seed, ctr, rk);
      } else {
        float* sc = opts->score_rec ? opts->score_rec + (size_t)t * BN : (float*)(ws + o_score);
        float* slp = opts->score_logp_rec ? opts->score_logp_rec + (size_t)t * BN : (float*)(ws + o_slp);
        r = sigmaenv_priority_forward(h, opts->priority_net, nullptr, scratch, sc, slp, rk, seed, ctr, deterministic);
      }
      if (r) return r;
      ranks = rk;
    } else if (opts->rank_rec) {
      HIPCHK(h, hipMemcpyAsync(opts->rank_rec + (size_t)t * BN, ranks, BN * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(act, 0, BN * 2 * sizeof(float), h->stream));  // combined_action / combined_sample_log_prob start at zero
    if (logp) HIPCHK(h, hipMemsetAsync(logp, 0, BN * sizeof(float), h->stream));
    float* rec = opts->tentative_rec ? opts->tentative_rec + (size_t)t * BN * K * 2 : nullptr;
    float* base_rec = opts->base_obs_rec ? opts->base_obs_rec + (size_t)t * BN * Dc : nullptr;
    const size_t n_gather = (size_t)B * Dc;
    const wrap::TurnNoise nz = {noise ? opts->comm_noise_std[0] : 0.0f, noise ? opts->comm_noise_std[1] : 0.0f, noise ? opts->comm_noise_std_env : nullptr, seed, ctr,
                                h->cfg.env_index_base};
    for (int k = 0; k < N; ++k) {
      if (noise)
        hipLaunchKernelGGL(wrap::sigmaenv_turn_gather_noise_kernel, dim3((unsigned)((n_gather + 255) / 256)), dim3(256), 0, h->stream, h->buf.obs, D, h->buf.nearing, K, act, ranks, k,
                           B, N, compact, row_map, rec, base_rec, nz);
      else
        hipLaunchKernelGGL(wrap::sigmaenv_turn_gather_kernel, dim3((unsigned)((n_gather + 255) / 256)), dim3(256), 0, h->stream, h->buf.obs, D, h->buf.nearing, K, act, ranks, k, B, N,
                           compact, row_map, rec, base_rec);
      HIPCHK(h, hipGetLastError());
      const int r = actor_rows_f32(h, m, compact, B, row_map, scratch, low, high, act, logp, nullptr, seed, ctr, deterministic);
      if (r) return r;
    }
    return SIGMAENV_OK;
  }, n_steps, actions_buf, slab_base, logp_base, actions_rec, seed, counter0, path_first, path_count);
}

// the per-column stds of communication noise at `level` as the reference forms them (helper_training.py:1274-1284): the double products AGENTS["max_speed"] * level
// and AGENTS["max_steering"] * level, each rounded to fp32 where it multiplies the fp32 draws, laid out by position (comm_noise_std)
extern "C" int sigmaenv_comm_noise_stds(double level, float* stds4) {
  if (!stds4 || !(level >= 0.0) || isinf(level)) return SIGMAENV_EINVAL;
  const float s_v = (float)(SIGMAENV_AGENT_MAX_SPEED * level), s_d = (float)(SIGMAENV_AGENT_MAX_STEERING * level);
  for (int q = 0; q < 4; ++q) stds4[q] = comm_noise_std(q, s_v, s_d);
  return SIGMAENV_OK;
}
