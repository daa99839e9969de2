// sigmaenv_isb.inc -- the challenging initial-state buffer on the device (included by sigmaenv.hip after sigmaenv_isb.h, which states the index arithmetic and the
// decisions; the contract is in include/sigmaenv.h, sigmaenv_isb_*).  No state, index or probability visits the host.
//
// Mapping.  An entry is N state rows (two float4 each) and N path rows (one int4 each): every copy below moves 16 bytes per load and store.
//   sigmaenv_isb_env_kernel      every per-env decision of record / settle / reset, 16 envs per workgroup: one lane per env reads and writes the env's words (head / held,
//                                the episode copy, pending, the record flag) and hands the ring slot to the workgroup through LDS; after the barrier all 256 lanes move the
//                                envs' rows into their rings, consecutive lanes consecutive 16-byte pieces, and 16 lanes per env share the OR over its collision block.
//                                (One lane per env moving all 48 N bytes of its rows took 18 us per launch at 16 x 4096; see DESIGN.md section 7 for the figures.)
//   sigmaenv_isb_record_kernel   ONE workgroup of ISB_CHUNK lanes walks the record flags in chunks of ISB_CHUNK envs and carries the running rank offset: per chunk a
//                                wavefront ballot and popcount, the wavefronts' counts scanned in LDS, the chunk's recorders compacted into an LDS list, and the list's
//                                entries (those of the last `capacity` ranks) copied ring -> bank by all lanes together.  The kept ranks are at most `capacity`
//                                consecutive numbers, so no two of them share a bank slot; ptr / count are written by lane 0 with ordinary stores after the walk.
//   sigmaenv_isb_restart_kernel  one lane per (env, agent): the use decision and the entry index (recomputed per agent: two words of the generator), the entry's rows
//                                into the entry arrays of sigmaenv_reset's scatter kernel; an env that does not restart writes env index -1, which the scatter kernel
//                                skips.  sigmaenv_reset_scatter_kernel and sigmaenv_reset_derive_kernel then do what sigmaenv_reset(full_env = 1) does: ONE derivation.
// No atomics in these kernels, no wait of one workgroup on another, no host wait in record / restart / settle.

struct sigmaenv_isb {
  sigmaenv* owner = nullptr;  // the handle it was created on (null once that handle is destroyed)
  int B = 0, N = 0, capacity = 0, S = 0;
  float p_record = 1.0f, p_use = 0.2f;
  void* mem = nullptr;      // bank, words, rings, held, head, episode copies, pending: one allocation, zero-filled
  void* scratch = nullptr;  // record flags and the entry arrays: produced and consumed inside one call (0xFF bytes in the poison build)
  float* bank_state = nullptr;    // [capacity, N, 8]
  int32_t* bank_path = nullptr;   // [capacity, N, 4]
  int32_t* words = nullptr;       // ptr, count
  float* ring_state = nullptr;    // [B, S, N, 8]
  int32_t* ring_path = nullptr;   // [B, S, N, 4]
  int32_t *held = nullptr, *head = nullptr, *epi = nullptr;  // [B] each
  uint8_t* pending = nullptr;     // [B]
  uint8_t* rec = nullptr;         // [B] scratch: this step's record flags
  int32_t *e_env = nullptr, *e_agent = nullptr, *e_path = nullptr;  // [B N], [B N], [B N, 4] scratch: the entries of the restart
  float* e_state = nullptr;       // [B N, 8]
  size_t mem_bytes = 0, scratch_bytes = 0;
};

namespace isb {

#define ISB_BLOCK 256
enum { MODE_RESET = 0, MODE_RECORD = 1, MODE_SETTLE = 2 };

struct Dev {
  float4* bank_state; int4* bank_path; int32_t* words;
  float4* ring_state; int4* ring_path;
  int32_t *held, *head, *epi;
  uint8_t *pending, *rec;
  int B, N, S, capacity;
};

#define ISB_EPB 16                     /* envs per workgroup of the per-env kernel */
#define ISB_SUB (ISB_BLOCK / ISB_EPB)  /* lanes that share the scan of one env's collision block */

__global__ void __launch_bounds__(ISB_BLOCK) sigmaenv_isb_env_kernel(Dev d, const float4* __restrict__ state, const int4* __restrict__ path, const uint8_t* __restrict__ col_agents,
                                                                     const uint8_t* __restrict__ col_flags, const uint8_t* __restrict__ done, const int32_t* __restrict__ timer,
                                                                     int mode, uint64_t seed, uint64_t counter, int env_base, float p_record) {
  sigma_poison_lds();
  __shared__ int s_slot[ISB_EPB];                // the ring slot the env's rows go to, -1: none (an env that does not settle, or past the batch)
  __shared__ unsigned s_part[ISB_EPB][ISB_SUB];  // the lanes' shares of the OR over an env's collision block
  const int tid = threadIdx.x, e0 = blockIdx.x * ISB_EPB, N = d.N;
  if (mode == MODE_RESET && blockIdx.x == 0 && tid == 0) { d.words[0] = 0; d.words[1] = 0; }
  if (tid < ISB_EPB) {  // one lane per env reads and writes the env's words: the workgroup's other lanes learn the slot through LDS
    const int b = e0 + tid;
    int slot = -1;
    if (b < d.B && (mode != MODE_SETTLE || isb_settles(timer[b * 4 + 3], d.epi[b], d.pending[b]))) {
      int head = d.head[b], held = d.held[b];
      if (mode != MODE_RECORD) { head = 0; held = 0; d.epi[b] = timer[b * 4 + 3]; d.pending[b] = 0; }
      slot = isb_push(&head, &held, d.S);
      d.head[b] = head; d.held[b] = held;
    }
    s_slot[tid] = slot;
  }
  if (mode == MODE_RECORD) {
    const int e = tid / ISB_SUB, sub = tid - e * ISB_SUB, b = e0 + e, NN = N * N;
    unsigned any = 0u;
    if (b < d.B) {
      const uint8_t* ca = col_agents + (size_t)b * NN;
      if ((NN & 3) == 0) {  // (the env's block then starts on a 4-byte boundary)
        const uint32_t* ca4 = reinterpret_cast<const uint32_t*>(ca);
        for (int q = sub; q < NN / 4; q += ISB_SUB) any |= ca4[q];
      } else {
        for (int q = sub; q < NN; q += ISB_SUB) any |= ca[q];
      }
    }
    s_part[e][sub] = any;
  }
  __syncthreads();
  const int per = 3 * N;  // 16-byte pieces of an entry: 2 N of the state rows, N of the path rows
  for (int it = tid; it < ISB_EPB * per; it += ISB_BLOCK) {
    const int e = it / per, r = it - e * per, slot = s_slot[e];
    if (slot < 0) continue;
    const size_t b = (size_t)(e0 + e), to = b * d.S + slot;
    if (r < 2 * N) d.ring_state[to * N * 2 + r] = state[b * N * 2 + r];
    else d.ring_path[to * N + (r - 2 * N)] = path[b * N + (r - 2 * N)];
  }
  if (mode != MODE_RECORD || tid >= ISB_EPB || e0 + tid >= d.B) return;
  const int b = e0 + tid;
  unsigned any = 0u;
  for (int q = 0; q < ISB_SUB; ++q) any |= s_part[tid][q];
  d.rec[b] = (uint8_t)isb_records(any != 0u, isb_word(seed, counter, (uint32_t)(env_base + b), DRAW_ISB_RECORD), p_record);
  unsigned rq = 0u;
  for (int i = 0; i < N; ++i) rq |= col_flags[((size_t)b * N + i) * 4 + 3];
  d.pending[b] = (uint8_t)(!done[b] && rq != 0u);
}

__global__ void __launch_bounds__(ISB_CHUNK) sigmaenv_isb_record_kernel(Dev d) {
  sigma_poison_lds();
  __shared__ int s_wave[ISB_CHUNK / 64];
  __shared__ int s_list[ISB_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ptr = d.words[0], count = d.words[1], N = d.N;
  // R: the recorders of the whole batch (a kept rank is one of the last `capacity`, which needs R before the first copy)
  int mine = 0;
  for (int b = tid; b < d.B; b += ISB_CHUNK) mine += d.rec[b] != 0;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) mine += __shfl_xor(mine, m);
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  int R = 0;
  for (int w = 0; w < ISB_CHUNK / 64; ++w) R += s_wave[w];
  __syncthreads();
  int base = 0;  // the rank of the chunk's first recorder
  for (int b0 = 0; b0 < d.B; b0 += ISB_CHUNK) {
    const int b = b0 + tid;
    const bool f = b < d.B && d.rec[b] != 0;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < ISB_CHUNK / 64; ++w) { const int c = s_wave[w]; before += w < wave ? c : 0; total += c; }
    if (f) s_list[before + __popcll(bal & ((1ull << lane) - 1ull))] = b;
    __syncthreads();
    const int per = 3 * N;  // 16-byte pieces of an entry: 2 N of the state rows, N of the path rows
    for (int it = tid; it < total * per; it += ISB_CHUNK) {
      const int e = it / per, r = it - e * per, k = base + e;
      if (!isb_rank_kept(k, R, d.capacity)) continue;
      const int eb = s_list[e];
      const size_t src = (size_t)eb * d.S + isb_nth_latest(d.head[eb], d.held[eb], d.S, d.S), dst = (size_t)isb_bank_slot(ptr, k, d.capacity);
      if (r < 2 * N) d.bank_state[dst * N * 2 + r] = d.ring_state[src * N * 2 + r];
      else d.bank_path[dst * N + (r - 2 * N)] = d.ring_path[src * N + (r - 2 * N)];
    }
    __syncthreads();  // (s_wave and s_list are rewritten by the next chunk)
    base += total;
  }
  if (tid == 0) { d.words[0] = isb_ptr_after(ptr, R, d.capacity); d.words[1] = isb_count_after(count, R, d.capacity); }
}

__global__ void __launch_bounds__(ISB_BLOCK) sigmaenv_isb_restart_kernel(Dev d, const uint8_t* __restrict__ done, uint64_t seed, uint64_t counter, int env_base, float p_use, int n_paths,
                                                                         int32_t* __restrict__ e_env, int32_t* __restrict__ e_agent, int4* __restrict__ e_path, float4* __restrict__ e_state) {
  sigma_poison_lds();
  const int k = blockIdx.x * ISB_BLOCK + threadIdx.x;
  if (k >= d.B * d.N) return;
  const int N = d.N, b = k / N, i = k - b * N;
  int count = d.words[1];
  count = count < d.capacity ? count : d.capacity;  // (a loaded count never addresses past the bank)
  bool use = isb_uses(done[b], count, isb_word(seed, counter, (uint32_t)(env_base + b), DRAW_ISB_USE), p_use) != 0;
  int j = 0;
  if (use) {
    j = isb_index(isb_word(seed, counter, (uint32_t)(env_base + b), DRAW_ISB_INDEX), count);
    for (int q = 0; q < N; ++q) use = use && (unsigned)d.bank_path[(size_t)j * N + q].x < (unsigned)n_paths;  // a loaded row outside the path table is never used as an address: the env stays done
  }
  e_env[k] = use ? b : -1;
  e_agent[k] = i;
  if (!use) return;
  e_path[k] = d.bank_path[(size_t)j * N + i];
  e_state[2 * (size_t)k] = d.bank_state[((size_t)j * N + i) * 2];
  e_state[2 * (size_t)k + 1] = d.bank_state[((size_t)j * N + i) * 2 + 1];
}

__global__ void sigmaenv_isb_words_kernel(int32_t* words, int ptr, int count) {
  sigma_poison_lds();
  if (threadIdx.x == 0 && blockIdx.x == 0) { words[0] = ptr; words[1] = count; }
}

static Dev dev_of(const sigmaenv_isb* k) {
  return Dev{(float4*)k->bank_state, (int4*)k->bank_path, k->words, (float4*)k->ring_state, (int4*)k->ring_path, k->held, k->head, k->epi, k->pending, k->rec, k->B, k->N, k->S, k->capacity};
}

}  // namespace isb

static bool isb_owned(sigmaenv* h, const sigmaenv_isb* k, const char* what) {
  if (!k) { h->err = std::string(what) + ": null bank"; return false; }
  if (k->owner != h) { h->err = std::string(what) + ": the bank belongs to another handle"; return false; }
  return true;
}

// sigmaenv_destroy: the handle's banks stay valid for sigmaenv_isb_destroy alone
static void isb_orphan(sigmaenv* h) {
  for (sigmaenv_isb* k : h->isbs) k->owner = nullptr;
  h->isbs.clear();
  h->isb_attached = nullptr;
}

extern "C" void sigmaenv_isb_destroy(sigmaenv_isb* k) {
  if (!k) return;
  if (sigmaenv* h = k->owner) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);  // launches that still read or write its memory
    if (h->isb_attached == k) h->isb_attached = nullptr;
    for (size_t q = 0; q < h->isbs.size(); ++q)
      if (h->isbs[q] == k) { h->isbs.erase(h->isbs.begin() + (long)q); break; }
  }
  if (k->mem) (void)hipFree(k->mem);
  if (k->scratch) (void)hipFree(k->scratch);
  delete k;
}

static int isb_env_launch(sigmaenv* h, sigmaenv_isb* k, int mode, uint64_t seed, uint64_t counter) {
  hipLaunchKernelGGL(isb::sigmaenv_isb_env_kernel, dim3((unsigned)((k->B + ISB_EPB - 1) / ISB_EPB)), dim3(ISB_BLOCK), 0, h->stream, isb::dev_of(k), (const float4*)h->buf.state,
                     (const int4*)h->buf.path, (const uint8_t*)h->buf.col_agents, (const uint8_t*)h->buf.col_flags, (const uint8_t*)h->buf.done, (const int32_t*)h->buf.timer, mode, seed,
                     counter, (int)h->cfg.env_index_base, k->p_record);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_isb_reset(sigmaenv_t* h, sigmaenv_isb* k) {
  if (!h) return SIGMAENV_EINVAL;
  if (!isb_owned(h, k, "isb_reset")) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  return isb_env_launch(h, k, isb::MODE_RESET, 0, 0);
}

extern "C" int sigmaenv_isb_create(sigmaenv_t* h, int32_t capacity, int32_t n_steps_stored, float p_record, float p_use, sigmaenv_isb** out) {
  if (!h || !out) return SIGMAENV_EINVAL;
  *out = nullptr;
  if (capacity < 1 || capacity > ISB_MAX_CAPACITY || n_steps_stored < 1 || n_steps_stored > ISB_MAX_STEPS_STORED || !(p_record >= 0.0f && p_record <= 1.0f) ||
      !(p_use >= 0.0f && p_use <= 1.0f)) {
    h->err = "isb_create: capacity 1 .. 65536, n_steps_stored 1 .. 1024, probabilities in [0, 1]";
    return SIGMAENV_EINVAL;
  }
  HIPCHK(h, hipSetDevice(h->device));
  auto* k = new sigmaenv_isb();
  k->B = h->B; k->N = h->N; k->capacity = capacity; k->S = n_steps_stored; k->p_record = p_record; k->p_use = p_use;
  const size_t B = (size_t)h->B, N = (size_t)h->N, C = (size_t)capacity, S = (size_t)n_steps_stored;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  // every section starts on a 16-byte boundary (the rows are moved 16 bytes at a time)
  const size_t o_bs = 0, o_bp = o_bs + C * N * 32, o_w = o_bp + C * N * 16, o_rs = o_w + 16, o_rp = o_rs + B * S * N * 32, o_held = o_rp + B * S * N * 16, o_head = o_held + up(B * 4),
               o_epi = o_head + up(B * 4), o_pend = o_epi + up(B * 4);
  k->mem_bytes = o_pend + up(B);
  const size_t s_rec = 0, s_env = s_rec + up(B), s_agent = s_env + up(B * N * 4), s_path = s_agent + up(B * N * 4), s_state = s_path + B * N * 16;
  k->scratch_bytes = s_state + B * N * 32;
  hipError_t e = hipMalloc(&k->mem, k->mem_bytes);
  if (e == hipSuccess) e = hipMalloc(&k->scratch, k->scratch_bytes);
  if (e != hipSuccess) {
    h->err = std::string("isb_create: hipMalloc: ") + hipGetErrorString(e);
    sigmaenv_isb_destroy(k);
    return SIGMAENV_ENOMEM;
  }
  char* m = (char*)k->mem;
  k->bank_state = (float*)(m + o_bs); k->bank_path = (int32_t*)(m + o_bp); k->words = (int32_t*)(m + o_w); k->ring_state = (float*)(m + o_rs); k->ring_path = (int32_t*)(m + o_rp);
  k->held = (int32_t*)(m + o_held); k->head = (int32_t*)(m + o_head); k->epi = (int32_t*)(m + o_epi); k->pending = (uint8_t*)(m + o_pend);
  char* sc = (char*)k->scratch;
  k->rec = (uint8_t*)(sc + s_rec); k->e_env = (int32_t*)(sc + s_env); k->e_agent = (int32_t*)(sc + s_agent); k->e_path = (int32_t*)(sc + s_path); k->e_state = (float*)(sc + s_state);
  k->owner = h;
  h->isbs.push_back(k);
  e = hipMemsetAsync(k->mem, 0, k->mem_bytes, h->stream);
#ifdef SIGMAENV_POISON
  if (e == hipSuccess) e = hipMemsetAsync(k->scratch, 0xFF, k->scratch_bytes, h->stream);
#else
  if (e == hipSuccess) e = hipMemsetAsync(k->scratch, 0, k->scratch_bytes, h->stream);
#endif
  if (e != hipSuccess) { h->err = std::string("isb_create: hipMemsetAsync: ") + hipGetErrorString(e); sigmaenv_isb_destroy(k); return SIGMAENV_EHIP; }
  const int rc = sigmaenv_isb_reset(h, k);
  if (rc) { sigmaenv_isb_destroy(k); return rc; }
  *out = k;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_isb_record(sigmaenv_t* h, sigmaenv_isb* k, uint64_t seed, uint64_t counter) {
  if (!h) return SIGMAENV_EINVAL;
  if (!isb_owned(h, k, "isb_record")) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const int rc = isb_env_launch(h, k, isb::MODE_RECORD, seed, counter);
  if (rc) return rc;
  hipLaunchKernelGGL(isb::sigmaenv_isb_record_kernel, dim3(1), dim3(ISB_CHUNK), 0, h->stream, isb::dev_of(k));
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_isb_restart(sigmaenv_t* h, sigmaenv_isb* k, uint64_t seed, uint64_t counter) {
  if (!h) return SIGMAENV_EINVAL;
  if (!isb_owned(h, k, "isb_restart")) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const int n = k->B * k->N;
  hipLaunchKernelGGL(isb::sigmaenv_isb_restart_kernel, dim3((unsigned)((n + ISB_BLOCK - 1) / ISB_BLOCK)), dim3(ISB_BLOCK), 0, h->stream, isb::dev_of(k), (const uint8_t*)h->buf.done, seed, counter,
                     (int)h->cfg.env_index_base, k->p_use, h->n_paths, k->e_env, k->e_agent, (int4*)k->e_path, (float4*)k->e_state);
  HIPCHK(h, hipGetLastError());
  // sigmaenv_reset(full_env = 1) from here on, its entries already on the device: scatter (entries with env index -1 are skipped), derive, fresh observation
  hipLaunchKernelGGL(sigmaenv_reset_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->buf, h->N, n, (const int32_t*)k->e_env, (const int32_t*)k->e_agent,
                     (const int32_t*)k->e_path, (const float*)k->e_state, 1);
  HIPCHK(h, hipGetLastError());
  return launch_derive(h, 1);
}

extern "C" int sigmaenv_isb_settle(sigmaenv_t* h, sigmaenv_isb* k) {
  if (!h) return SIGMAENV_EINVAL;
  if (!isb_owned(h, k, "isb_settle")) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  return isb_env_launch(h, k, isb::MODE_SETTLE, 0, 0);
}

extern "C" int sigmaenv_isb_attach(sigmaenv_t* h, sigmaenv_isb* k) {
  if (!h) return SIGMAENV_EINVAL;
  if (k && !isb_owned(h, k, "isb_attach")) return SIGMAENV_EINVAL;
  h->isb_attached = k;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_isb_get(sigmaenv_t* h, sigmaenv_isb* k, int32_t what, void** dev_ptr, size_t* bytes) {
  if (!h || !dev_ptr || !bytes) return SIGMAENV_EINVAL;
  if (!isb_owned(h, k, "isb_get")) return SIGMAENV_EINVAL;
  const size_t B = (size_t)k->B, N = (size_t)k->N, C = (size_t)k->capacity, S = (size_t)k->S;
  switch (what) {
    case SIGMAENV_ISB_BANK_STATE: *dev_ptr = k->bank_state; *bytes = C * N * 32; break;
    case SIGMAENV_ISB_BANK_PATH: *dev_ptr = k->bank_path; *bytes = C * N * 16; break;
    case SIGMAENV_ISB_WORDS: *dev_ptr = k->words; *bytes = 8; break;
    case SIGMAENV_ISB_RING_STATE: *dev_ptr = k->ring_state; *bytes = B * S * N * 32; break;
    case SIGMAENV_ISB_RING_PATH: *dev_ptr = k->ring_path; *bytes = B * S * N * 16; break;
    case SIGMAENV_ISB_HELD: *dev_ptr = k->held; *bytes = B * 4; break;
    case SIGMAENV_ISB_HEAD: *dev_ptr = k->head; *bytes = B * 4; break;
    case SIGMAENV_ISB_PENDING: *dev_ptr = k->pending; *bytes = B; break;
    case SIGMAENV_ISB_EPISODES: *dev_ptr = k->epi; *bytes = B * 4; break;
    default: h->err = "isb_get: unknown item"; return SIGMAENV_EINVAL;
  }
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_isb_set(sigmaenv_t* h, sigmaenv_isb* k, const float* state_rows, const int32_t* path_rows, int32_t count) {
  if (!h) return SIGMAENV_EINVAL;
  if (!isb_owned(h, k, "isb_set")) return SIGMAENV_EINVAL;
  if (count < 0 || count > k->capacity || (count > 0 && (!state_rows || !path_rows))) { h->err = "isb_set: 0 <= count <= capacity entries, with their state and path rows"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t N = (size_t)k->N;
  if (count > 0) {
    HIPCHK(h, hipMemcpyAsync(k->bank_state, state_rows, (size_t)count * N * 32, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(k->bank_path, path_rows, (size_t)count * N * 16, hipMemcpyDeviceToDevice, h->stream));
  }
  hipLaunchKernelGGL(isb::sigmaenv_isb_words_kernel, dim3(1), dim3(64), 0, h->stream, k->words, (int)(count % k->capacity), (int)count);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}
