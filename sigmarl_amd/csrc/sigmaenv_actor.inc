// sigmaenv_actor.inc -- the policy (actor) forward pass on the device, so that a rollout needs no host round trip per step
// (SURVEY.md section 8f, rank 3).  Included at the end of sigmaenv.hip (it uses the handle's stream and buffers).
//
// What it restates: the actor of sigmarl/modules/decision_making_module.py:34-82 -- torchrl MultiAgentMLP(n_agent_inputs = obs_dim,
// n_agent_outputs = 2 * 2, depth = 3, num_cells = 256, activation = Tanh, share_params = True, centralised = False), i.e. for every
// agent row  Linear(D,256) Tanh Linear(256,256) Tanh Linear(256,256) Tanh Linear(256,4);  NormalParamExtractor: loc = out[0:2],
// scale = max(softplus(out[2:4] + ln(e^0.99 - 1)) + 0.01, 1e-4) ("biased_softplus_1.0");  TanhNormal(loc, scale, low, high): x = loc + scale * z,
// y = tanh(x), action = low + (y + 1) / 2 * (high - low), log-probability summed over the two action dimensions (actor_distribution).
// torchrl / tensordict are third-party and absent here: the distribution details are restated from their documented behaviour.  Pinned: the draw of every
// row (generator key, uniforms, Box-Muller branch), the action and the log-probability against fp64 on all four head paths (tests/test_gpu_policy_head.py,
// with the host restatement tests/policy_head_check.py); the MLP against torch.nn / fp64 (tests/test_gpu_actor.py, tests/test_gpu_networks.py).  The kernel
// takes the log-probability from the UNCLAMPED x = loc + scale z (never from atanh of the clamped y).  Not pinned (no torchrl here): whether torchrl's
// TanhNormal.log_prob of a saturated sample uses x (its cache) or atanh(clamped y).
//
// MI355X mapping.  This is the one GEMM-shaped piece next to the env step: B*N = 65536 rows x (D*256 + 2*256*256 + 256*4) MACs per
// step = 18 GFLOP -> matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulate), bf16 weights and activations.
//  * Transposed product: out^T[features, rows] = W[features, K] * X^T[K, rows].  The weights are the A operand (16 features x 32 k per
//    MFMA, one ds_read_b128 per lane from LDS), the activations the B operand (32 k x 16 rows) and live in REGISTERS for the whole
//    network: the accumulator of a layer (feature = 16 ft + 4 (lane >> 4) + reg, row = lane & 15) is, after tanh and conversion to
//    bf16, directly the B fragment of the next layer when that layer's weight matrix has its K axis permuted accordingly -- k slot
//    (kb, g, j) <-> input feature 16 (2 kb + (j >> 2)) + 4 g + (j & 3) -- which the packing does once (sigmaenv_pack.h).  No transpose, no
//    LDS round trip between layers.
//  * One workgroup of 8 wavefronts per CU, every wavefront owns 2 row tiles (32 rows): each weight fragment read from LDS feeds two
//    MFMAs.  LDS holds one big layer at a time (W2 or W3: 128 KB bf16 of the 160 KB) plus the small first / last layer.
//  * Sampling: counter-based RNG (rng_u32, the env's generator) + Box-Muller, one (z0, z1) pair per agent row.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

#include "sigmaenv_pack.h"  // ACT_H (the hidden width) and the packed bf16 form of the weights
#ifndef ACT_RT
#define ACT_RT 2             /* MFMA row tiles (16 rows) per wavefront */
#endif
#define ACT_ROWS_PER_WAVE (16 * ACT_RT)
#define ACT_WAVES (16 / ACT_RT)

struct ActorWeights {
  // packed bf16 weights: layer l as [K/32][4][F][8] (the bf16 form of sigmaenv_pack.h), biases fp32
  const __bf16 *w1, *w2, *w3, *w4;
  const float *b1, *b2, *b3, *b4;
  int D;            // observation width (multiple of 8, <= 32)
  float low[2], high[2];
};

__device__ __forceinline__ float fast_tanh(float x) {
  // 1 - 2 / (1 + e^{2x}) with the hardware exp2 / rcp (absolute error ~1e-7: far below the bf16 rounding that follows)
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e);
}

// One hidden layer for the wavefront's two row tiles, output pair by output pair: the two 16-feature tiles (2 p, 2 p + 1) that form
// k block p of the NEXT layer's B fragment are accumulated over all k blocks, then squashed and packed at once.  Only 4 accumulator
// tiles are live, and the tanh of pair p (vector unit) is independent of the MFMAs of pair p + 1 (matrix unit), so the two overlap.
template <int KB>
__device__ __forceinline__ void actor_hidden_layer(const __bf16* __restrict__ w_lds, const float* __restrict__ bias, const bf16x8_t (&x)[8][ACT_RT],
                                                   bf16x8_t (&xn)[8][ACT_RT], int lane) {
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const float4 b0 = *reinterpret_cast<const float4*>(bias + (2 * p) * 16 + 4 * g), b1 = *reinterpret_cast<const float4*>(bias + (2 * p + 1) * 16 + 4 * g);
    f32x4_t a0[ACT_RT], a1[ACT_RT];
#pragma unroll
    for (int rt = 0; rt < ACT_RT; ++rt) { a0[rt] = f32x4_t{b0.x, b0.y, b0.z, b0.w}; a1[rt] = f32x4_t{b1.x, b1.y, b1.z, b1.w}; }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const __bf16* base = w_lds + ((size_t)((kb * 4 + g) * ACT_H + c)) * 8;
      const bf16x8_t w0 = *reinterpret_cast<const bf16x8_t*>(base + (size_t)(2 * p) * 16 * 8);
      const bf16x8_t w1 = *reinterpret_cast<const bf16x8_t*>(base + (size_t)(2 * p + 1) * 16 * 8);
#pragma unroll
      for (int rt = 0; rt < ACT_RT; ++rt) {
        a0[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x[kb][rt], a0[rt], 0, 0, 0);
        a1[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x[kb][rt], a1[rt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rt = 0; rt < ACT_RT; ++rt) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = (__bf16)fast_tanh(a0[rt][j]);
        v[4 + j] = (__bf16)fast_tanh(a1[rt][j]);
      }
      xn[p][rt] = v;
    }
  }
}

// output layer: 4 features padded to one tile of 16
__device__ __forceinline__ void actor_output_layer(const __bf16* __restrict__ w_lds, const float* __restrict__ bias, const bf16x8_t (&x)[8][ACT_RT], f32x4_t (&out)[ACT_RT],
                                                   int lane) {
  const int g = lane >> 4, c = lane & 15;
  const float4 bb = *reinterpret_cast<const float4*>(bias + 4 * g);
#pragma unroll
  for (int rt = 0; rt < ACT_RT; ++rt) out[rt] = f32x4_t{bb.x, bb.y, bb.z, bb.w};
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) {
    const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(w_lds + ((size_t)((kb * 4 + g) * 16 + c)) * 8);
#pragma unroll
    for (int rt = 0; rt < ACT_RT; ++rt) out[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, x[kb][rt], out[rt], 0, 0, 0);
  }
}

// NormalParamExtractor + TanhNormal of the actor (decision_making_module.py:50-82), one agent row: the head of sigmaenv_dist.h in two dimensions
__device__ __forceinline__ void actor_distribution(const float (&low)[2], const float (&high)[2], int row, int n_agents, int env_base, float loc0, float loc1, float raw0, float raw1,
                                                   float* __restrict__ actions, float* __restrict__ log_prob, float* __restrict__ loc_scale, uint64_t seed,
                                                   uint64_t counter, int deterministic) {
  const float sc0 = tn_scale(raw0), sc1 = tn_scale(raw1);
  if (loc_scale) *reinterpret_cast<float4*>(loc_scale + (size_t)row * 4) = make_float4(loc0, loc1, sc0, sc1);
  float z0 = 0.0f, z1 = 0.0f;
  if (!deterministic) {  // one normal pair of the env's counter-based generator (row = env * n_agents + agent)
    const uint32_t env = (uint32_t)(env_base + row / n_agents), agent = (uint32_t)(row - (row / n_agents) * n_agents);  // env: index in the whole batch (sigmaenv_config_t.env_index_base)
    rng_normal_pair(seed, counter, env, agent, DRAW_ACTOR, &z0, &z1);
  }
  const float x0 = loc0 + sc0 * z0, x1 = loc1 + sc1 * z1;
  const float h0 = 0.5f * (high[0] - low[0]), h1 = 0.5f * (high[1] - low[1]);
  *reinterpret_cast<float2*>(actions + (size_t)row * 2) = make_float2(tn_affine(low[0], tn_squash(x0), h0), tn_affine(low[1], tn_squash(x1), h1));
  if (log_prob) log_prob[row] = (tn_log_density(z0, logf(sc0), x0) - logf(h0)) + (tn_log_density(z1, logf(sc1), x1) - logf(h1));
}

// weights global (L2) -> LDS, eight 16-byte loads in flight per thread (the copy is a chain of L2 round trips otherwise)
__device__ __forceinline__ void lds_fill(__bf16* dst, const __bf16* __restrict__ src, size_t n_bf16) {
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  const size_t n = n_bf16 / 8, stride = blockDim.x;
  size_t k = threadIdx.x;
  for (; k + 7 * stride < n; k += 8 * stride) {
    uint4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = s4[k + u * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) d4[k + u * stride] = v[u];
  }
  for (; k < n; k += stride) d4[k] = s4[k];
}

__global__ void __launch_bounds__(64 * ACT_WAVES, 1) sigmaenv_actor_kernel(ActorWeights aw, const float* __restrict__ obs, int R, int n_agents, int env_base, float* __restrict__ actions,
                                                                 float* __restrict__ log_prob, float* __restrict__ loc_scale, uint64_t seed, uint64_t counter,
                                                                 int deterministic) {
  sigma_poison_lds();
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __bf16* w_small = reinterpret_cast<__bf16*>(smem_raw);                  // W1 ([1][4][256][8] = 16 KB), later W4 ([8][4][16][8] = 8 KB)
  __bf16* w_big = reinterpret_cast<__bf16*>(smem_raw + 16 * 1024);         // W2, later W3 ([8][4][256][8] = 128 KB)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int KB1 = aw.D / 32 > 0 ? aw.D / 32 : 1;                           // D = 32: one k block
  lds_fill(w_small, aw.w1, (size_t)KB1 * 4 * ACT_H * 8);
  lds_fill(w_big, aw.w2, (size_t)8 * 4 * ACT_H * 8);
  const int row0 = (blockIdx.x * ACT_WAVES + wave) * ACT_ROWS_PER_WAVE;
  // layer-1 input: B fragment (k slot (0, g, j) <-> feature 8 g + j): eight consecutive observation entries of row (row0 + 16 rt + c)
  bf16x8_t x[8][ACT_RT];
#pragma unroll
  for (int rt = 0; rt < ACT_RT; ++rt) {
    const int row = row0 + 16 * rt + c;
    bf16x8_t v;
    if (row < R && 8 * g < aw.D) {
      const float4 lo = *reinterpret_cast<const float4*>(obs + (size_t)row * aw.D + 8 * g);
      const float4 hi = *reinterpret_cast<const float4*>(obs + (size_t)row * aw.D + 8 * g + 4);
      v[0] = (__bf16)lo.x; v[1] = (__bf16)lo.y; v[2] = (__bf16)lo.z; v[3] = (__bf16)lo.w;
      v[4] = (__bf16)hi.x; v[5] = (__bf16)hi.y; v[6] = (__bf16)hi.z; v[7] = (__bf16)hi.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
    }
    x[0][rt] = v;
  }
  __syncthreads();
  bf16x8_t y[8][ACT_RT];
  actor_hidden_layer<1>(w_small, aw.b1, x, y, lane);
  actor_hidden_layer<8>(w_big, aw.b2, y, x, lane);
  __syncthreads();  // everyone is done with W1 / W2
  lds_fill(w_small, aw.w4, (size_t)8 * 4 * 16 * 8);
  lds_fill(w_big, aw.w3, (size_t)8 * 4 * ACT_H * 8);
  __syncthreads();
  actor_hidden_layer<8>(w_big, aw.b3, x, y, lane);
  // features 0..3 of the output tile = (loc0, loc1, raw_scale0, raw_scale1) sit in lane group 0
  f32x4_t outv[ACT_RT];
  actor_output_layer(w_small, aw.b4, y, outv, lane);
  if (g == 0) {
#pragma unroll
    for (int rt = 0; rt < ACT_RT; ++rt) {
      const int row = row0 + 16 * rt + c;
      if (row >= R) continue;
      actor_distribution(aw.low, aw.high, row, n_agents, env_base, outv[rt][0], outv[rt][1], outv[rt][2], outv[rt][3], actions, log_prob, loc_scale, seed, counter, deterministic);
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct sigmaenv_actor {
  ActorWeights w{};
  std::vector<void*> allocs;
  int D = 0;
};

// one packed buffer of a network handle on the device (sigmaenv_actor_create, sigmaenv_mlp32_create): allocated, recorded in the handle's allocs, filled from host memory
static int pack_upload(std::vector<void*>& allocs, const void* src, size_t bytes, const void** dst) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return SIGMAENV_ENOMEM;
  allocs.push_back(p);
  if (hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return SIGMAENV_EHIP;
  *dst = p;
  return SIGMAENV_OK;
}

extern "C" void sigmaenv_actor_destroy(sigmaenv_actor* a) {
  if (!a) return;
  for (void* p : a->allocs) (void)hipFree(p);
  delete a;
}

// weights / biases: host pointers in torch.nn.Linear layout (w_l: [out, in] row-major fp32).  low / high: action bounds (2 each).
extern "C" int sigmaenv_actor_create(int32_t obs_dim, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                                     const float* w4, const float* b4, const float* low, const float* high, sigmaenv_actor** out) {
  if (!out || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4 || !low || !high || obs_dim < 8 || obs_dim > 32 || (obs_dim % 8)) return SIGMAENV_EINVAL;
  auto* a = new sigmaenv_actor();
  a->D = obs_dim;
  // the per-slot function of sigmaenv_pack.h over every lane index of every layer, on the host (sigmaenv_actor_load_device: the same function on the device)
  const float *ws[4] = {w1, w2, w3, w4}, *bs[4] = {b1, b2, b3, b4};
  const __bf16** pw[4] = {&a->w.w1, &a->w.w2, &a->w.w3, &a->w.w4};
  const float** pb[4] = {&a->w.b1, &a->w.b2, &a->w.b3, &a->w.b4};
  for (int l = 0; l < 4; ++l) {
    ActorLayer y = pack_actor_layer(obs_dim, l);
    std::vector<uint16_t> sw(y.n_slots);
    std::vector<float> sb(y.nb);
    y.w = ws[l]; y.b = bs[l]; y.pw = sw.data(); y.pb = sb.data();
    for (int i = 0; i < y.n_slots + y.nb; ++i) pack_actor_slot(y, i);
    int rc = pack_upload(a->allocs, sw.data(), sw.size() * 2, (const void**)pw[l]);
    if (!rc) rc = pack_upload(a->allocs, sb.data(), sb.size() * 4, (const void**)pb[l]);
    if (rc) { sigmaenv_actor_destroy(a); return rc; }
  }
  a->w.D = obs_dim;
  for (int i = 0; i < 2; ++i) { a->w.low[i] = low[i]; a->w.high[i] = high[i]; }
  const int smem = 16 * 1024 + 128 * 1024;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sigmaenv_actor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  *out = a;
  return SIGMAENV_OK;
}

// actions := policy(observation) for every agent row of the handle (observation = SIGMAENV_BUF_OBS, or `obs` when given: device
// pointer f32 [B*N, obs_dim]).  actions: device f32 [B, N, 2]; log_prob (optional): device f32 [B, N]; loc_scale (optional): device f32
// [B, N, 4] = (loc0, loc1, scale0, scale1).  Enqueued on the handle's stream.
extern "C" int sigmaenv_actor_forward(sigmaenv_t* h, sigmaenv_actor* a, const float* obs, float* actions, float* log_prob, float* loc_scale, uint64_t seed,
                                      uint64_t counter, int32_t deterministic) {
  if (!h || !a || !actions || (!obs && a->D != h->D)) return SIGMAENV_EINVAL;  // (with a caller's obs the width is the caller's contract)
  HIPCHK(h, hipSetDevice(h->device));
  const int R = h->B * h->N;
  const int rows_per_block = ACT_WAVES * ACT_ROWS_PER_WAVE;
  const int slot = timer_begin(h, SIGMAENV_KERNEL_ACTOR_BF16);
  hipLaunchKernelGGL(sigmaenv_actor_kernel, dim3((R + rows_per_block - 1) / rows_per_block), dim3(64 * ACT_WAVES), 16 * 1024 + 128 * 1024, h->stream, a->w,
                     obs ? obs : h->buf.obs, R, h->N, h->cfg.env_index_base, actions, log_prob, loc_scale, seed, counter, (int)deterministic);
  HIPCHK(h, hipGetLastError());
  timer_end(h, SIGMAENV_KERNEL_ACTOR_BF16, slot);
  return SIGMAENV_OK;
}

// T steps of (policy -> fused step + record + resets) without returning to the caller: actions_buf device f32 [B, N, 2] (scratch),
// slab_base (optional) device f32 [T, B, W]: row block t receives the record of step t; logp_base (optional) device f32 [T, B, N].
// the loop shared by sigmaenv_rollout (bf16 actor) and sigmaenv_rollout_f32 (the reference's fp32 actor): policy(t) enqueues the actor forward
// of step t writing the actions (and log-probabilities) to the given pointers
static int eval_check_frames(sigmaenv* h, const sigmaenv_eval* ev, uint64_t more, const char* what);  // sigmaenv_eval.inc
template <class Policy>
static int rollout_loop(sigmaenv_t* h, Policy policy, int32_t n_steps, float* actions_buf, float* slab_base, float* logp_base, float* actions_rec, uint64_t seed,
                        uint64_t counter0, int32_t path_first, int32_t path_count) {
  if (!h || !actions_buf || n_steps < 1) return SIGMAENV_EINVAL;
  if (path_count != 0 && !paths_ok(h, path_first, path_count)) { h->err = "rollout: path range outside the table (or no scenario lists set)"; return SIGMAENV_EINVAL; }
  const size_t W = (size_t)h->N * (h->D + 1) + 1, BN = (size_t)h->B * h->N;
  const size_t slab_stride = h->rollout_slab_stride ? h->rollout_slab_stride : (size_t)h->B * W;
  if (h->eval_attached) {  // an attached evaluator takes one frame per step: refused here, before the first launch, if it could not take them all
    const int rc = eval_check_frames(h, h->eval_attached, (uint64_t)n_steps, "rollout (evaluator attached)");
    if (rc) return rc;
  }
  for (int t = 0; t < n_steps; ++t) {
    float* act = actions_rec ? actions_rec + (size_t)t * BN * 2 : actions_buf;
    int rc = policy(t, act, logp_base ? logp_base + (size_t)t * BN : nullptr);
    if (rc) return rc;
    if (h->rollout_obs_rec) {  // the rows the step's final actor forward read (sigmaenv_set_rollout_obs_record): the step overwrites them
      const size_t own = BN * (size_t)h->D;
      HIPCHK(h, hipMemcpyAsync(h->rollout_obs_rec + (size_t)t * (h->rollout_obs_stride ? h->rollout_obs_stride : own), h->buf.obs, own * sizeof(float), hipMemcpyDeviceToDevice,
                               h->stream));
    }
    // step t records into row block t of slab_base, or -- without one -- wherever the handle records (sigmaenv_set_slab); the handle's target is only read
    rc = launch_cbf_then_step(h, {act, slab_base ? slab_base + (size_t)t * slab_stride : h->buf.slab, seed, counter0 + (uint64_t)t, path_first, path_count}, true);
    if (rc) return rc;
  }
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_rollout(sigmaenv_t* h, sigmaenv_actor* a, int32_t n_steps, float* actions_buf, float* slab_base, float* logp_base, float* actions_rec,
                                uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count, int32_t deterministic) {
  if (!h || !a) return SIGMAENV_EINVAL;
  return rollout_loop(h, [&](int t, float* act, float* logp) { return sigmaenv_actor_forward(h, a, nullptr, act, logp, nullptr, seed, counter0 + (uint64_t)t, deterministic); },
                      n_steps, actions_buf, slab_base, logp_base, actions_rec, seed, counter0, path_first, path_count);
}
