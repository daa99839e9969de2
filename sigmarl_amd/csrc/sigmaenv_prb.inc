// sigmaenv_prb.inc -- the prioritized replay buffer ON THE DEVICE: the priorities and their sum / min hierarchy, sampling with replacement proportional to priority,
// the importance weights, and the TD-error refresh of the sampled frames after an optimiser step (included by sigmaenv.hip after sigmaenv_ppo.inc; the contract is
// in include/sigmaenv.h, sigmaenv_prb_*).
//
// What it replaces: torchrl's TensorDictPrioritizedReplayBuffer as sigmarl/mappo_cavs.py:321-332 builds it (a C++ segment tree and np.random.uniform on the host),
// its sample() before every minibatch (:397-407) and _update_priorities_after_training behind every optimiser step (:431-456: compute_td_error,
// sigmarl/helper_training.py:1029-1068, then update_tensordict_priority) -- num_epochs x frames // minibatch_size times per iteration, each a device-to-host round
// trip in a loop that otherwise has none.  The arithmetic -- the order of every sum, the descent, every element formula -- is stated once, in sigmaenv_prb.h.
//
// Mapping.  One NODE (256 consecutive entries of a level) per wavefront everywhere: lane l loads its four entries as one 16-byte word (every level is allocated
// in whole nodes), the lane sums are scanned with cross-lane moves (prb::node_scan) -- no LDS, no atomics.
//  rebuild  one launch per level, bottom up: wavefront w of the launch over level k writes (sum, min) of node w into level k + 1; the launch over the top level has
//           one wavefront and writes the words total / q_min.  F = 524288: 2048 + 8 + 1 nodes in three launches over 2 MB of leaves that stay in L2 / MALL.
//           extend and refresh both end with this full rebuild: after either, every level is the same function of the leaves.
//  sample   one wavefront per slot: per level the node's prefixes, a ballot for the first child whose prefix exceeds the remaining mass, the descent (three nodes
//           at F = 524288).  total and q_min are read from the device words.
//  refresh  (1) one lane per slot: x_m from the record row of frame index[m] and the critic's two values; per workgroup the min / max of the bits of its valid
//           slots (x >= 0: the unsigned order of the bits is the order of the values) -> partial[2 P];  (2) every workgroup folds the P partials itself (lane t the
//           chain over c = t, t + 256, .., the butterfly, the four wavefronts: any P), normalises its slots, takes the power and scatters into the leaves
//           (duplicates of a frame write the same bits);  (3) the rebuild.
// -ffp-contract=off (Makefile): every operator is one IEEE fp32 operation.
struct sigmaenv_prb {
  int device = 0;
  int capacity = 0, len = 0, n_levels = 0, max_index = 0;
  int n[PRB_MAX_LEVELS + 1] = {0};       // entries per level; n[n_levels] = 1: the words
  float* sum[PRB_MAX_LEVELS + 1] = {nullptr};  // sum[0] = the leaves; sum[n_levels] = &words[0]
  float* mn[PRB_MAX_LEVELS + 1] = {nullptr};   // mn[0] = the leaves;  mn[n_levels] = &words[1]
  float* words = nullptr;                // [2] total, q_min
  float* ws_x = nullptr;                 // [max_index] raw TD errors of a refresh
  uint32_t* ws_mm = nullptr;             // [2 * ceil(max_index / 256)] per-workgroup min / max bits
  float alpha = 0.0f, neg_beta = 0.0f, eps = 0.0f;
  std::vector<void*> allocs;
};

namespace prb {

// the wavefront's node: lane l holds e = its four entries (already masked).  Returns c[0 .. 3] (the lane chain), I (the inclusive scan of the lane sums) and E (the
// exclusive one) -- prb_node_prefix's additions
__device__ __forceinline__ void node_scan(const float4& e, int lane, float* c, float& I, float& E) {
  prb_lane_chain(e.x, e.y, e.z, e.w, c);
  I = c[3];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(I, d, 64);
    if (lane >= d) I = I + t;
  }
  E = __shfl_up(I, 1, 64);
  if (lane == 0) E = 0.0f;
}

__device__ __forceinline__ float4 load_node(const float* __restrict__ level, long long base, int lane, long long valid, float fill) {
  const long long p = base + 4 * lane;
  float4 e = *reinterpret_cast<const float4*>(level + p);  // (every level is allocated in whole nodes)
  e.x = p < valid ? e.x : fill;
  e.y = p + 1 < valid ? e.y : fill;
  e.z = p + 2 < valid ? e.z : fill;
  e.w = p + 3 < valid ? e.w : fill;
  return e;
}

// wavefront w: node w of (src_sum, src_min) with `valid` entries -> dst_sum[w], dst_min[w]
__global__ void __launch_bounds__(256) sigmaenv_prb_level_kernel(const float* __restrict__ src_sum, const float* __restrict__ src_min, int valid, int n_nodes,
                                                                 float* __restrict__ dst_sum, float* __restrict__ dst_min) {
  sigma_poison_lds();
  const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_nodes) return;
  const long long base = (long long)w * PRB_FAN;
  const float4 es = load_node(src_sum, base, lane, valid, 0.0f), em = load_node(src_min, base, lane, valid, INFINITY);
  float c[4], I, E;
  node_scan(es, lane, c, I, E);
  float m = prb_lane_min(em.x, em.y, em.z, em.w);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = prb_min(m, __shfl_xor(m, s, 64));
  const float total = __shfl(I, 63, 64);
  m = __shfl(m, 0, 64);
  if (lane == 0) { dst_sum[w] = total; dst_min[w] = m; }
}

__global__ void __launch_bounds__(256) sigmaenv_prb_leaf_kernel(const float* __restrict__ td, int n, float eps, float alpha, float* __restrict__ leaves) {
  sigma_poison_lds();
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n) leaves[f] = prb_priority(td[f], eps, alpha);
}

__global__ void __launch_bounds__(256) sigmaenv_prb_sample_kernel(PrbLevels L, const float* __restrict__ words, int len, int M, uint64_t seed, uint64_t counter, float neg_beta,
                                                                  int32_t* __restrict__ index_out, float* __restrict__ weight_out) {
  sigma_poison_lds();
  const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float total = words[0], q_min = words[1];
  float r = prb_uniform(rng_u32(seed, counter, (uint32_t)m, 0u, PRB_DRAW)) * total;
  int node = 0;
  for (int k = L.n_levels - 1; k >= 0; --k) {
    const int cnt = prb_cnt(len, k);
    const long long base = (long long)node * PRB_FAN;
    const float4 e = load_node(L.sum[k], base, lane, cnt, 0.0f);
    float c[4], I, E;
    node_scan(e, lane, c, I, E);
    const float S0 = E + c[0], S1 = E + c[1], S2 = E + c[2], S3 = I;
    const int i = r < S0 ? 0 : r < S1 ? 1 : r < S2 ? 2 : r < S3 ? 3 : 4;
    const unsigned long long hit = __ballot(i < 4);
    const int left = cnt - 1 - (int)base, last = left < PRB_FAN - 1 ? left : PRB_FAN - 1;
    int j = last;
    if (hit) {
      const int first = __ffsll((long long)hit) - 1;
      j = 4 * first + __shfl(i, first, 64);
    }
    j = j < last ? j : last;
    // S_{j-1}: element (j - 1) & 3 of lane (j - 1) >> 2 (j is wavefront-uniform)
    const int el = (j - 1) & 3;
    const float mine = el == 0 ? S0 : el == 1 ? S1 : el == 2 ? S2 : S3;
    const float prev = __shfl(mine, j > 0 ? (j - 1) >> 2 : 0, 64);
    r = r - (j > 0 ? prev : 0.0f);
    node = (int)base + j;
  }
  if (lane == 0) {
    index_out[m] = node;
    weight_out[m] = prb_weight(L.sum[0][node], q_min, neg_beta);
  }
}

// the workgroup's 256 (lo, hi) pairs -> their min / max in every lane
__device__ __forceinline__ void block_minmax(uint32_t& lo, uint32_t& hi, uint32_t* wlo, uint32_t* whi) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const uint32_t lo2 = (uint32_t)__shfl_xor((int)lo, s, 64), hi2 = (uint32_t)__shfl_xor((int)hi, s, 64);
    lo = lo2 < lo ? lo2 : lo;
    hi = hi2 > hi ? hi2 : hi;
  }
  if ((threadIdx.x & 63) == 0) { wlo[threadIdx.x >> 6] = lo; whi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  lo = wlo[0]; hi = whi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) { lo = wlo[w] < lo ? wlo[w] : lo; hi = whi[w] > hi ? whi[w] : hi; }
}

struct RefreshArgs {
  const int32_t* index;
  const float *v, *vn, *slab;
  int M, len, N, D, P;
  float td_gamma, eps, alpha;
};

__global__ void __launch_bounds__(256) sigmaenv_prb_x_kernel(RefreshArgs a, float* __restrict__ x_out, uint32_t* __restrict__ partial) {
  sigma_poison_lds();
  __shared__ uint32_t wlo[4], whi[4];
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  bool on = false;
  float x = 0.0f;
  if (m < a.M) {
    const int f = a.index[m];
    on = f >= 0 && f < a.len;  // an entry outside [0, len) is never used as an address
    if (on) {
      const float* p = a.slab + (long long)f * ((long long)a.N * (a.D + 1) + 1) + (long long)a.N * a.D;
      x = prb_x(p, a.N, p[a.N], a.v[m], a.vn[m], a.td_gamma);
      x_out[m] = x;
    }
  }
  uint32_t lo = on ? __float_as_uint(x) : 0xFFFFFFFFu, hi = on ? __float_as_uint(x) : 0u;
  block_minmax(lo, hi, wlo, whi);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo; partial[2 * blockIdx.x + 1] = hi; }
}

__global__ void __launch_bounds__(256) sigmaenv_prb_scatter_kernel(RefreshArgs a, const float* __restrict__ x_in, const uint32_t* __restrict__ partial, float* __restrict__ leaves,
                                                                   float* __restrict__ td_out) {
  sigma_poison_lds();
  __shared__ uint32_t wlo[4], whi[4];
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (int c = threadIdx.x; c < a.P; c += 256) {
    const uint32_t l2 = partial[2 * c], h2 = partial[2 * c + 1];
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  block_minmax(lo, hi, wlo, whi);
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= a.M) return;
  const int f = a.index[m];
  if (f < 0 || f >= a.len) return;  // its slot writes nothing
  const float td = prb_norm(x_in[m], __uint_as_float(lo), __uint_as_float(hi));
  if (td_out) td_out[m] = td;
  leaves[f] = prb_priority(td, a.eps, a.alpha);
}

static int rebuild(sigmaenv* h, sigmaenv_prb* b) {
  for (int k = 0; k < b->n_levels; ++k) {
    const int valid = k == 0 ? b->len : b->n[k], nodes = b->n[k + 1];
    hipLaunchKernelGGL(sigmaenv_prb_level_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, h->stream, (const float*)b->sum[k], (const float*)b->mn[k], valid, nodes,
                       b->sum[k + 1], b->mn[k + 1]);
    HIPCHK(h, hipGetLastError());
  }
  return SIGMAENV_OK;
}

static bool bad_ptr(const void* p) { return !p || ((uintptr_t)p & 3); }

}  // namespace prb

extern "C" void sigmaenv_prb_destroy(sigmaenv_prb* b) {
  if (!b) return;
  for (void* p : b->allocs) (void)hipFree(p);
  delete b;
}

extern "C" int sigmaenv_prb_create(sigmaenv_t* h, int64_t capacity, double alpha, double beta, double eps, sigmaenv_prb** out) {
  if (!h || !out) return SIGMAENV_EINVAL;
  *out = nullptr;
  if (capacity < 1 || capacity > PRB_MAX_CAPACITY || !(alpha >= 0.0 && alpha <= 1.0) || !(beta >= 0.0 && std::isfinite(beta)) || !(eps >= 0.0 && std::isfinite(eps))) {
    h->err = "prb_create: capacity in [1, 2^30], alpha in [0, 1], beta >= 0 and eps >= 0, all finite";
    return SIGMAENV_EINVAL;
  }
  HIPCHK(h, hipSetDevice(h->device));
  auto* b = new sigmaenv_prb();
  b->device = h->device;
  b->capacity = (int)capacity;
  b->alpha = (float)alpha; b->neg_beta = -(float)beta; b->eps = (float)eps;
  b->n_levels = prb_level_sizes(capacity, b->n);
  b->n[b->n_levels] = 1;
  b->max_index = b->capacity > 65536 ? b->capacity : 65536;
  // every level in whole nodes (a wavefront loads 16 bytes per lane); the fill: zeros, 0xFF bytes for the workspace in the poison build (as dev_alloc's scratch)
  auto alloc = [&](void** p, size_t bytes, bool scratch) -> int {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { h->err = std::string("prb_create: hipMalloc: ") + hipGetErrorString(e); return SIGMAENV_ENOMEM; }
    b->allocs.push_back(*p);
#ifdef SIGMAENV_POISON
    e = hipMemsetAsync(*p, scratch ? 0xFF : 0, bytes, h->stream);
#else
    (void)scratch;
    e = hipMemsetAsync(*p, 0, bytes, h->stream);
#endif
    if (e != hipSuccess) { h->err = std::string("prb_create: hipMemsetAsync: ") + hipGetErrorString(e); return SIGMAENV_EHIP; }
    return SIGMAENV_OK;
  };
  int rc = SIGMAENV_OK;
  for (int k = 0; k < b->n_levels && rc == SIGMAENV_OK; ++k) {
    const size_t padded = ((size_t)b->n[k] + PRB_FAN - 1) / PRB_FAN * PRB_FAN * sizeof(float);
    rc = alloc((void**)&b->sum[k], padded, false);
    if (k == 0) b->mn[0] = b->sum[0];
    else if (rc == SIGMAENV_OK) rc = alloc((void**)&b->mn[k], padded, false);
  }
  if (rc == SIGMAENV_OK) rc = alloc((void**)&b->words, 2 * sizeof(float), false);
  if (rc == SIGMAENV_OK) rc = alloc((void**)&b->ws_x, (size_t)b->max_index * sizeof(float), true);
  if (rc == SIGMAENV_OK) rc = alloc((void**)&b->ws_mm, (size_t)((b->max_index + 255) / 256) * 2 * sizeof(uint32_t), true);
  if (rc != SIGMAENV_OK) { sigmaenv_prb_destroy(b); return rc; }
  b->sum[b->n_levels] = b->words;
  b->mn[b->n_levels] = b->words + 1;
  *out = b;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_prb_extend(sigmaenv_t* h, sigmaenv_prb* b, const float* td, int64_t n) {
  if (!h) return SIGMAENV_EINVAL;
  if (!b) { h->err = "prb_extend: null buffer handle"; return SIGMAENV_EINVAL; }
  if (prb::bad_ptr(td)) { h->err = "prb_extend: td is null or not 4-byte aligned"; return SIGMAENV_EINVAL; }
  if (n < 1 || n > b->capacity) { h->err = "prb_extend: n = " + std::to_string(n) + " is not in [1, capacity = " + std::to_string(b->capacity) + "]"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  b->len = (int)n;
  hipLaunchKernelGGL(prb::sigmaenv_prb_leaf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, td, (int)n, b->eps, b->alpha, b->sum[0]);
  HIPCHK(h, hipGetLastError());
  return prb::rebuild(h, b);
}

extern "C" int sigmaenv_prb_sample(sigmaenv_t* h, sigmaenv_prb* b, int32_t n_index, uint64_t seed, uint64_t counter, int32_t* index_out, float* weight_out) {
  if (!h) return SIGMAENV_EINVAL;
  if (!b) { h->err = "prb_sample: null buffer handle"; return SIGMAENV_EINVAL; }
  if (b->len < 1) { h->err = "prb_sample: the buffer is empty (sigmaenv_prb_extend first)"; return SIGMAENV_EINVAL; }
  if (n_index < 1) { h->err = "prb_sample: n_index >= 1"; return SIGMAENV_EINVAL; }
  if (prb::bad_ptr(index_out) || prb::bad_ptr(weight_out)) { h->err = "prb_sample: index_out or weight_out is null or not 4-byte aligned"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  PrbLevels L{};
  L.n_levels = b->n_levels;
  for (int k = 0; k < b->n_levels; ++k) L.sum[k] = b->sum[k];
  hipLaunchKernelGGL(prb::sigmaenv_prb_sample_kernel, dim3((unsigned)((n_index + 3) / 4)), dim3(256), 0, h->stream, L, (const float*)b->words, b->len, (int)n_index, seed, counter,
                     b->neg_beta, index_out, weight_out);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_prb_refresh(sigmaenv_t* h, sigmaenv_prb* b, const sigmaenv_prb_refresh_args_t* a) {
  if (!h) return SIGMAENV_EINVAL;
  if (!b || !a) { h->err = "prb_refresh: null buffer handle or arguments"; return SIGMAENV_EINVAL; }
  if (b->len < 1) { h->err = "prb_refresh: the buffer is empty (sigmaenv_prb_extend first)"; return SIGMAENV_EINVAL; }
  if (a->n_index < 1 || a->n_index > b->max_index) { h->err = "prb_refresh: n_index in [1, max(capacity, 65536)]"; return SIGMAENV_EINVAL; }
  if (prb::bad_ptr(a->index) || prb::bad_ptr(a->state_value) || prb::bad_ptr(a->next_state_value) || prb::bad_ptr(a->slab) || (a->td_out && ((uintptr_t)a->td_out & 3))) {
    h->err = "prb_refresh: index, state_value, next_state_value and slab are required, every tensor 4-byte aligned";
    return SIGMAENV_EINVAL;
  }
  if (!(a->td_gamma >= 0.0f && a->td_gamma <= 1.0f)) { h->err = "prb_refresh: td_gamma in [0, 1]"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  prb::RefreshArgs r{};
  r.index = a->index; r.v = a->state_value; r.vn = a->next_state_value; r.slab = a->slab;
  r.M = a->n_index; r.len = b->len; r.N = h->N; r.D = h->D; r.P = (a->n_index + 255) / 256;
  r.td_gamma = a->td_gamma; r.eps = b->eps; r.alpha = b->alpha;
  hipLaunchKernelGGL(prb::sigmaenv_prb_x_kernel, dim3((unsigned)r.P), dim3(256), 0, h->stream, r, b->ws_x, b->ws_mm);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(prb::sigmaenv_prb_scatter_kernel, dim3((unsigned)r.P), dim3(256), 0, h->stream, r, (const float*)b->ws_x, (const uint32_t*)b->ws_mm, b->sum[0], a->td_out);
  HIPCHK(h, hipGetLastError());
  return prb::rebuild(h, b);
}

extern "C" int sigmaenv_prb_get(sigmaenv_t* h, sigmaenv_prb* b, int32_t what, void* host_out) {
  if (!h) return SIGMAENV_EINVAL;
  if (!b || !host_out) { h->err = "prb_get: null buffer handle or destination"; return SIGMAENV_EINVAL; }
  if (what == SIGMAENV_PRB_LEN) { *(int32_t*)host_out = b->len; return SIGMAENV_OK; }
  if (what == SIGMAENV_PRB_N_LEVELS) { *(int32_t*)host_out = b->n_levels; return SIGMAENV_OK; }
  const void* src = nullptr;
  size_t bytes = 0;
  if (what == SIGMAENV_PRB_LEAVES) { src = b->sum[0]; bytes = (size_t)b->len * 4; }
  else if (what == SIGMAENV_PRB_TOTAL) { src = b->words; bytes = 4; }
  else if (what == SIGMAENV_PRB_QMIN) { src = b->words + 1; bytes = 4; }
  else if (what >= SIGMAENV_PRB_LEVEL_SUM + 1 && what < SIGMAENV_PRB_LEVEL_SUM + b->n_levels) { src = b->sum[what - SIGMAENV_PRB_LEVEL_SUM]; bytes = (size_t)b->n[what - SIGMAENV_PRB_LEVEL_SUM] * 4; }
  else if (what >= SIGMAENV_PRB_LEVEL_MIN + 1 && what < SIGMAENV_PRB_LEVEL_MIN + b->n_levels) { src = b->mn[what - SIGMAENV_PRB_LEVEL_MIN]; bytes = (size_t)b->n[what - SIGMAENV_PRB_LEVEL_MIN] * 4; }
  else { h->err = "prb_get: unknown item " + std::to_string(what); return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  if (bytes) {
    HIPCHK(h, hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));  // the one call of the buffer that waits
  return SIGMAENV_OK;
}
