// sigmaenv_optim.inc -- the optimiser step of a minibatch update ON THE DEVICE: the global gradient-norm clip, Adam and the repack of every network's weight forms
// (included by sigmaenv.hip after sigmaenv_load.inc and sigmaenv_grad.inc; the contract is in include/sigmaenv.h, sigmaenv_optim_step / sigmaenv_mlp32_resolve_mode).
//
// What it replaces: the last three lines of _train_on_batch (sigmarl/mappo_cavs.py:421-426: clip_grad_norm_, optim.step(), optim.zero_grad()) and the two loads
// that followed them here -- foreach kernels over 16 tensors, two snapshot copies, one pack launch per layer and form, and per network a host wait for the 4-byte
// range word.  The arithmetic -- the order of every sum, every operation of the element update -- is stated once, in sigmaenv_optim.h; "what word goes into
// destination slot i" once, in sigmaenv_pack.h.
//
// Mapping.  About 400 000 parameters, 6.5 MB read and 5 MB written: microseconds of HBM time, so the step is latency-bound and there is nothing to tune beyond
// coalescing.  Three launches for all networks together on the handle's stream; none of them waits:
//  1. norm partials: one workgroup of 256 lanes per chunk of 1024 consecutive elements of one tensor; lane t squares and adds the elements t, t + 256, .. (4-byte
//     loads, consecutive lanes consecutive words: 4-byte alignment of every tensor suffices and no access is wider), butterfly, the four wavefronts in order.
//  2. apply: the same grid.  EVERY workgroup adds all partials in the header's order (a few hundred words from L2), so every workgroup holds the same bits of the
//     coefficient without a launch in between; then p, m, v of its chunk in place, the gradient read only.  Workgroup 0 also writes (total_norm, clip_coef) and
//     zeroes each network's range word for launch 3.
//  3. pack: blockIdx.y picks a layer of the layer table, blockIdx.x strides over that layer's lanes: the exact fragments, the split pairs and both bias vectors
//     (pack_mlp32_slot), the transposed exact fragments (pack_mlp32_t_slot) and, where an actor handle is given, the bf16 form (pack_actor_slot) -- the functions
//     sigmaenv_mlp32_create / sigmaenv_actor_create / *_load_device loop over, reading the parameters themselves (no snapshot copy).  The split form's range
//     predicate is ORed into each network's own word with the vector atomicOr, as the load kernel does.
// The tensor table and the layer table travel in the kernel arguments (indexed by a workgroup-uniform index only).
namespace optim {

struct Tensors {
  float* p[OPTIM_MAX_TENSORS];
  const float* g[OPTIM_MAX_TENSORS];
  float* m[OPTIM_MAX_TENSORS];
  float* v[OPTIM_MAX_TENSORS];
  int n[OPTIM_MAX_TENSORS];      // elements
  int first[OPTIM_MAX_TENSORS];  // the tensor's first chunk
  int n_tensors, P;              // P: chunks of all tensors
};

struct PackLayer {
  Mlp32Layer a;  // exact and split form, both bias vectors
  float* tw;     // transposed exact form (layers >= 1), n_t slots
  ActorLayer y;  // bf16 form (y.pw == nullptr: no actor handle)
  int n_a, n_t, n_y;
};
struct PackTable {
  PackLayer layer[OPTIM_MAX_NETS * MLP32_MAX_LAYERS];
};
struct RangeWords {
  uint32_t* word[OPTIM_MAX_NETS];
  int n;
};

// the workgroup's 256 lane values -> their sum in every lane: optim_reduce256's additions (sigmaenv_optim.h)
__device__ __forceinline__ float block_sum(float v, float* wsum) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = v + __shfl_xor(v, s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// chunk c -> its tensor (the last one whose first chunk is <= c) -- workgroup-uniform
__device__ __forceinline__ int tensor_of(const Tensors& a, int c) {
  int t = 0;
  for (int i = 1; i < a.n_tensors; ++i) t = a.first[i] <= c ? i : t;
  return t;
}

__global__ void __launch_bounds__(256) sigmaenv_optim_norm_kernel(Tensors a, float* __restrict__ partial) {
  sigma_poison_lds();
  __shared__ float wsum[4];
  const int c = blockIdx.x, t = tensor_of(a, c);
  const int off = (c - a.first[t]) * OPTIM_CHUNK, n = a.n[t] - off < OPTIM_CHUNK ? a.n[t] - off : OPTIM_CHUNK;
  const float s = block_sum(optim_lane_sumsq(a.g[t] + off, n, threadIdx.x), wsum);
  if (threadIdx.x == 0) partial[c] = s;
}

__global__ void __launch_bounds__(256) sigmaenv_optim_apply_kernel(Tensors a, const float* __restrict__ partial, OptimScalars sc, RangeWords rw, float* __restrict__ result) {
  sigma_poison_lds();
  __shared__ float wsum[4];
  const int c = blockIdx.x, t = tensor_of(a, c), tid = threadIdx.x;
  const float total_norm = optim_total_norm(block_sum(optim_lane_sum(partial, a.P, tid), wsum));
  const float coef = optim_clip_coef(total_norm, sc.max_grad_norm);
  if (c == 0 && tid == 0) { result[0] = total_norm; result[1] = coef; }
  if (c == 0 && tid == 0) {  // (launch 3 ORs into them)
    if (rw.n > 0) *rw.word[0] = 0u;
    if (rw.n > 1) *rw.word[1] = 0u;
    if (rw.n > 2) *rw.word[2] = 0u;
    if (rw.n > 3) *rw.word[3] = 0u;
  }
  const int off = (c - a.first[t]) * OPTIM_CHUNK, n = a.n[t] - off < OPTIM_CHUNK ? a.n[t] - off : OPTIM_CHUNK;
  const float* g = a.g[t] + off;
  float *p = a.p[t] + off, *m = a.m[t] + off, *v = a.v[t] + off;
  for (int i = tid; i < n; i += OPTIM_LANES) {
    float pi = p[i], mi = m[i], vi = v[i];
    optim_adam(sc, coef, g[i], pi, mi, vi);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

__global__ void __launch_bounds__(256) sigmaenv_optim_pack_kernel(PackTable tb) {
  sigma_poison_lds();
  const PackLayer& L = tb.layer[blockIdx.y];
  const int total = L.n_a + L.n_t + L.n_y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < L.n_a) { if (pack_mlp32_slot(L.a, i)) atomicOr(L.a.range, 1u); }
    else if (i < L.n_a + L.n_t) pack_mlp32_t_slot(L.a.w, L.tw, L.a.F, L.a.K, i - L.n_a);
    else pack_actor_slot(L.y, i - L.n_a - L.n_t);
  }
}

// what both entry points walk: the networks' tensors in the order given -- per network, per layer: weight, bias
static int count(sigmaenv_t* h, const sigmaenv_optim_args_t* a, const char* what, int* n_tensors, int64_t* chunks) {
  if (a->n_networks < 1 || a->n_networks > OPTIM_MAX_NETS) { h->err = std::string(what) + ": 1 to " + std::to_string(OPTIM_MAX_NETS) + " networks"; return SIGMAENV_EINVAL; }
  int nt = 0;
  int64_t P = 0;
  for (int k = 0; k < a->n_networks; ++k) {
    const sigmaenv_mlp32* m = a->net[k].mlp32;
    if (!m || !m->range_word) { h->err = std::string(what) + ": network " + std::to_string(k) + ": null network handle"; return SIGMAENV_EINVAL; }
    for (int l = 0; l < m->w.n_layers; ++l) {
      nt += 2;
      P += optim_chunks((int64_t)m->dims[l] * m->dims[l + 1]) + optim_chunks(m->dims[l + 1]);
    }
  }
  if (nt > OPTIM_MAX_TENSORS) { h->err = std::string(what) + ": " + std::to_string(nt) + " tensors, at most " + std::to_string(OPTIM_MAX_TENSORS); return SIGMAENV_EINVAL; }
  *n_tensors = nt;
  *chunks = P;
  return SIGMAENV_OK;
}

}  // namespace optim

extern "C" int sigmaenv_optim_workspace(sigmaenv_t* h, const sigmaenv_optim_args_t* a, uint64_t* n_floats) {
  if (!h || !a || !n_floats) return SIGMAENV_EINVAL;
  int nt = 0;
  int64_t P = 0;
  if (const int rc = optim::count(h, a, "optim_workspace", &nt, &P)) return rc;
  *n_floats = (uint64_t)P;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_optim_step(sigmaenv_t* h, const sigmaenv_optim_args_t* a) {
  if (!h || !a) return SIGMAENV_EINVAL;
  int nt = 0;
  int64_t P = 0;
  if (const int rc = optim::count(h, a, "optim_step", &nt, &P)) return rc;
  auto finite_nonneg = [](double x) { return std::isfinite(x) && x >= 0.0; };
  if (a->t < 1 || !(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !finite_nonneg(a->eps) || !finite_nonneg(a->lr) ||
      !finite_nonneg(a->max_grad_norm)) {
    h->err = "optim_step: t >= 1, beta1 and beta2 in [0, 1), and eps, lr and max_grad_norm finite and not negative";
    return SIGMAENV_EINVAL;
  }
  if (!a->workspace || !a->result || ((uintptr_t)a->workspace & 3) || ((uintptr_t)a->result & 3)) {
    h->err = "optim_step: a null workspace or result, or one that is not 4-byte aligned";
    return SIGMAENV_EINVAL;
  }
  optim::Tensors ts{};
  optim::PackTable tb{};
  optim::RangeWords rw{};
  int it = 0, il = 0, chunk = 0, max_lanes = 1;
  for (int k = 0; k < a->n_networks; ++k) {
    const sigmaenv_optim_net_t& nk = a->net[k];
    sigmaenv_mlp32* m = nk.mlp32;
    const int n = m->w.n_layers;
    const void* const* arrays[] = {(const void* const*)nk.weights, (const void* const*)nk.biases, (const void* const*)nk.grad_weights, (const void* const*)nk.grad_biases,
                                   (const void* const*)nk.exp_avg_weights, (const void* const*)nk.exp_avg_biases, (const void* const*)nk.exp_avg_sq_weights,
                                   (const void* const*)nk.exp_avg_sq_biases};
    for (const void* const* arr : arrays) {
      if (!arr) { h->err = "optim_step: network " + std::to_string(k) + ": null pointer array"; return SIGMAENV_EINVAL; }
      for (int l = 0; l < n; ++l)
        if (!arr[l] || ((uintptr_t)arr[l] & 3)) {
          h->err = "optim_step: network " + std::to_string(k) + " layer " + std::to_string(l) + ": a null tensor or one that is not 4-byte aligned";
          return SIGMAENV_EINVAL;
        }
    }
    if (nk.actor && (n != 4 || m->in_dim != nk.actor->D || m->out_dim != 4)) {
      h->err = "optim_step: network " + std::to_string(k) + ": the bf16 actor handle is not of the fp32 network's shape";
      return SIGMAENV_EINVAL;
    }
    rw.word[k] = m->range_word;
    const __bf16* pw[4] = {nullptr, nullptr, nullptr, nullptr};
    const float* pb[4] = {nullptr, nullptr, nullptr, nullptr};
    if (nk.actor) {
      const __bf16* w_[4] = {nk.actor->w.w1, nk.actor->w.w2, nk.actor->w.w3, nk.actor->w.w4};
      const float* b_[4] = {nk.actor->w.b1, nk.actor->w.b2, nk.actor->w.b3, nk.actor->w.b4};
      for (int l = 0; l < 4; ++l) { pw[l] = w_[l]; pb[l] = b_[l]; }
    }
    for (int l = 0; l < n; ++l) {
      const int K = m->dims[l], F = m->dims[l + 1];
      for (int wb = 0; wb < 2; ++wb, ++it) {  // weight, bias
        ts.p[it] = wb ? nk.biases[l] : nk.weights[l];
        ts.g[it] = wb ? nk.grad_biases[l] : nk.grad_weights[l];
        ts.m[it] = wb ? nk.exp_avg_biases[l] : nk.exp_avg_weights[l];
        ts.v[it] = wb ? nk.exp_avg_sq_biases[l] : nk.exp_avg_sq_weights[l];
        ts.n[it] = wb ? F : F * K;
        ts.first[it] = chunk;
        chunk += optim_chunks(ts.n[it]);
      }
      optim::PackLayer& L = tb.layer[il++];
      L.a = pack_mlp32_layer(m->dims, l, n, m->split_fits);
      L.a.w = nk.weights[l]; L.a.b = nk.biases[l];
      L.a.ew = const_cast<float*>(m->w.w[l]); L.a.eb = const_cast<float*>(m->w.b[l]);
      L.a.sw = reinterpret_cast<uint16_t*>(const_cast<f16x8_t*>(m->ws.w[l])); L.a.sb = const_cast<float*>(m->ws.b[l]);
      L.a.range = m->range_word;
      L.n_a = pack_mlp32_lanes(L.a);
      L.tw = m->wt[l];  // (layer 0: only a handle made by sigmaenv_mlp32_create_input_grad holds the form)
      L.n_t = m->wt[l] ? load_exact_t_slots(F, K) : 0;
      if (nk.actor) {
        L.y = pack_actor_layer(nk.actor->D, l);
        L.y.w = nk.weights[l]; L.y.b = nk.biases[l];
        L.y.pw = reinterpret_cast<uint16_t*>(const_cast<__bf16*>(pw[l])); L.y.pb = const_cast<float*>(pb[l]);
        L.n_y = L.y.n_slots + L.y.nb;
      }
      const int lanes = L.n_a + L.n_t + L.n_y;
      max_lanes = lanes > max_lanes ? lanes : max_lanes;
    }
  }
  ts.n_tensors = it; ts.P = chunk; rw.n = a->n_networks;
  const OptimScalars sc = optim_scalars(a->lr, a->beta1, a->beta2, a->eps, a->max_grad_norm, a->t);
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(optim::sigmaenv_optim_norm_kernel, dim3((unsigned)chunk), dim3(256), 0, h->stream, ts, a->workspace);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(optim::sigmaenv_optim_apply_kernel, dim3((unsigned)chunk), dim3(256), 0, h->stream, ts, (const float*)a->workspace, sc, rw, a->result);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(optim::sigmaenv_optim_pack_kernel, dim3((unsigned)load::grid_for(max_lanes), (unsigned)il), dim3(256), 0, h->stream, tb);
  HIPCHK(h, hipGetLastError());
  // the deferred mode: the exact form is valid for every weight; sigmaenv_mlp32_resolve_mode reads the range word when a caller wants the split form back
  for (int k = 0; k < a->n_networks; ++k) {
    sigmaenv_mlp32* m = a->net[k].mlp32;
    m->split_ok = false;
    m->mode = SIGMAENV_MLP32_EXACT;
  }
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_mlp32_resolve_mode(sigmaenv_t* h, sigmaenv_mlp32* m) {
  if (!h) return SIGMAENV_EINVAL;
  if (!m || !m->range_word) { h->err = "mlp32_resolve_mode: null network handle"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  uint32_t bad = 0;
  HIPCHK(h, hipMemcpyAsync(&bad, m->range_word, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // the one host wait of the device route
  m->split_ok = m->split_fits && bad == 0;
  m->mode = (m->requested == SIGMAENV_MLP32_SPLIT && m->split_ok) ? SIGMAENV_MLP32_SPLIT : SIGMAENV_MLP32_EXACT;
  return SIGMAENV_OK;
}
