// sigmaenv_load.inc -- a network's weights refreshed ON THE DEVICE from a learner's tensors (included by sigmaenv.hip after sigmaenv_mlp32.inc / sigmaenv_actor.inc;
// the contracts are in include/sigmaenv.h, sigmaenv_mlp32_load_device / sigmaenv_actor_load_device).
//
// The packed forms, their roundings and "what word goes into destination slot i" are stated once, in sigmaenv_pack.h; the kernels here loop over those per-slot
// functions on the device as sigmaenv_mlp32_create / sigmaenv_actor_create loop over them on the host, so a loaded handle holds word for word what *_create makes
// from the same numbers (tests/test_gpu_weight_load.py compares the two compilations bit for bit; tests/test_weight_load_host.py holds the functions to the frozen
// packers of tests/weight_pack_reference.h).
//
// Mapping.  The whole job is 1 - 2 MB: nothing to tune.  One launch per layer, one lane per destination slot (grid-stride): consecutive lanes store consecutive
// words, padding slots are written as zeros like every other slot (no slot of a packed buffer keeps an old value), the source is gathered with 4-byte loads
// (torch.nn.Linear layout, 4-byte alignment suffices).  The exact pack reads every source weight exactly once: it also reduces the split form's range predicate
// (load_out_of_range: !(|w| < 255), so a NaN is out of range) into one device word with a vector atomic OR.
namespace load {

__global__ void __launch_bounds__(256) sigmaenv_load_mlp32_kernel(Mlp32Layer a) {
  sigma_poison_lds();
  const int total = pack_mlp32_lanes(a);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
    if (pack_mlp32_slot(a, i)) atomicOr(a.range, 1u);
}

__global__ void __launch_bounds__(256) sigmaenv_load_actor_kernel(ActorLayer a) {
  sigma_poison_lds();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n_slots + a.nb; i += gridDim.x * blockDim.x) pack_actor_slot(a, i);
}

static int check_pointers(sigmaenv_t* h, const char* what, const float* const* weights_dev, const float* const* biases_dev, int n) {
  if (!weights_dev || !biases_dev) { h->err = std::string(what) + ": null pointer array"; return SIGMAENV_EINVAL; }
  for (int l = 0; l < n; ++l)
    if (!weights_dev[l] || !biases_dev[l] || ((uintptr_t)weights_dev[l] & 3) || ((uintptr_t)biases_dev[l] & 3)) {
      h->err = std::string(what) + ": layer " + std::to_string(l) + ": a null tensor or one that is not 4-byte aligned";
      return SIGMAENV_EINVAL;
    }
  return SIGMAENV_OK;
}

static inline int grid_for(int total) { return (total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024; }

}  // namespace load

static int mlp32_grad_load(sigmaenv_t* h, sigmaenv_mlp32* m, const float* const* weights_dev);  // sigmaenv_grad.inc: the transposed forms, same stream

extern "C" int sigmaenv_mlp32_load_device(sigmaenv_t* h, sigmaenv_mlp32* m, const float* const* weights_dev, const float* const* biases_dev) {
  if (!h) return SIGMAENV_EINVAL;
  if (!m || !m->range_word) { h->err = "mlp32_load_device: null network handle"; return SIGMAENV_EINVAL; }
  const int n = m->w.n_layers;
  if (int rc = load::check_pointers(h, "mlp32_load_device", weights_dev, biases_dev, n)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(m->range_word, 0, 4, h->stream));
  for (int l = 0; l < n; ++l) {
    Mlp32Layer a = pack_mlp32_layer(m->dims, l, n, m->split_fits);
    a.w = weights_dev[l]; a.b = biases_dev[l];
    a.ew = const_cast<float*>(m->w.w[l]); a.eb = const_cast<float*>(m->w.b[l]);
    a.sw = reinterpret_cast<uint16_t*>(const_cast<f16x8_t*>(m->ws.w[l])); a.sb = const_cast<float*>(m->ws.b[l]);
    a.range = m->range_word;
    hipLaunchKernelGGL(load::sigmaenv_load_mlp32_kernel, dim3(load::grid_for(pack_mlp32_lanes(a))), dim3(256), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
  }
  if (const int rc = mlp32_grad_load(h, m, weights_dev)) return rc;
  // the one host wait: the range word decides which form the next forward launches
  uint32_t bad = 0;
  HIPCHK(h, hipMemcpyAsync(&bad, m->range_word, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  m->split_ok = m->split_fits && bad == 0;
  m->mode = (m->requested == SIGMAENV_MLP32_SPLIT && m->split_ok) ? SIGMAENV_MLP32_SPLIT : SIGMAENV_MLP32_EXACT;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_actor_load_device(sigmaenv_t* h, sigmaenv_actor* a, const float* const* weights_dev, const float* const* biases_dev) {
  if (!h) return SIGMAENV_EINVAL;
  if (!a) { h->err = "actor_load_device: null network handle"; return SIGMAENV_EINVAL; }
  if (int rc = load::check_pointers(h, "actor_load_device", weights_dev, biases_dev, 4)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const __bf16* pw[4] = {a->w.w1, a->w.w2, a->w.w3, a->w.w4};
  const float* pb[4] = {a->w.b1, a->w.b2, a->w.b3, a->w.b4};
  for (int l = 0; l < 4; ++l) {
    ActorLayer y = pack_actor_layer(a->D, l);
    y.w = weights_dev[l]; y.b = biases_dev[l];
    y.pw = reinterpret_cast<uint16_t*>(const_cast<__bf16*>(pw[l])); y.pb = const_cast<float*>(pb[l]);
    hipLaunchKernelGGL(load::sigmaenv_load_actor_kernel, dim3(load::grid_for(y.n_slots + y.nb)), dim3(256), 0, h->stream, y);
    HIPCHK(h, hipGetLastError());
  }
  return SIGMAENV_OK;
}
