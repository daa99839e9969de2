// sigmaenv_eval.inc -- the evaluation of a policy on the device: the reference's four metrics per env from the per-step output buffers (included by sigmaenv.hip after
// sigmaenv_eval.h, which states the arithmetic; the contract is in include/sigmaenv.h, sigmaenv_eval_*).
//
// What it restates: sigmarl/evaluation_base.py:184-217 (_evaluate_model_i) on the frames a caller -- or an attached rollout, between every step and its resets --
// hands it.
//
// Mapping.  One lane per (env, agent slot): the lane group of an env is G = the smallest power of two >= N lanes, a wavefront holds 64 / G whole envs, so the
// butterfly of the header is log2 G cross-lane moves of a double (two 32-bit halves each) inside the wavefront -- no LDS, no barrier, no atomics.  Lane i of a
// group reads agent i's velocity, distance and lanelet byte and ORs the N flag bytes of its col_agents row (whole words when N is a multiple of 4: the row then
// starts on a word); the group's OR is a ballot masked to the group.  Group lane 0 reads, updates and writes the env's five accumulators: memory no other lane
// touches.  A frame is 46 bytes per agent plus N flag bytes: the launch is a few microseconds at 16 x 4096 and bound by its latency, not by bandwidth.

namespace eval {

#define EVL_BLOCK 256

struct Acc {  // the accumulators [B] each, one allocation
  double* sum_speed;
  double* sum_dref;
  uint32_t* n_aa;
  uint32_t* n_al;
  uint32_t* frames;
};

struct Study {  // what a study frame reads and writes besides (sigmaenv_eval.h, "the study of a CBF-filtered policy")
  const float* applied;   // [B,N,2]
  const float* nominal;   // [B,N,2]: the applied action again where no CBF-QP runs (evl_nominal_from_cbf)
  const float* r_goal;    // [B,N] each: rows EVL_REW_GOAL, EVL_REW_AGENTS, EVL_REW_LANE of the reward info
  const float* r_agents;
  const float* r_lane;
  const int32_t* timer;   // [B,4]: an initial frame takes the snapshot of columns 1, 2 from it
  float* carry;           // [B,N,2] (v_prev, a_prev)
  double* sums;           // [EVL_STUDY_SUMS, B]
  uint32_t* n_act;        // [B]
  int32_t* timer0;        // [B,2]
  int initial;
};
struct NoStudy {};

// STUDY = false is the kernel of the plain evaluator: `st` is an empty struct no instruction reads.
template <bool STUDY, class S>
__device__ __forceinline__ void accumulate_frame(const float* __restrict__ state, const float* __restrict__ dist_ref, const uint8_t* __restrict__ col_agents,
                                                 const uint8_t* __restrict__ col_flags, int B, int N, int G, const Acc& acc, float* __restrict__ trace_frame, const S& st) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (EVL_BLOCK >> 6) + (threadIdx.x >> 6);
  const int per_wave = 64 / G;          // whole envs per wavefront
  const int g = lane / G, i = lane - g * G;
  const long long b = wave * per_wave + g;
  const bool on = b < B;                // (no lane leaves early: the cross-lane moves below need the whole wavefront)
  const bool agent = on && i < N;
  const long long a = agent ? b * N + i : 0;  // the agent's row in [B, N, .]
  float x = 0.0f, y = 0.0f, vx = 0.0f, vy = 0.0f, dr = 0.0f;
  uint32_t row = 0, lanelet = 0;
  if (agent) {
    const float* s = state + a * 8;
    x = s[0]; y = s[1]; vx = s[5]; vy = s[6];
    dr = dist_ref[a];
    const uint8_t* ca = col_agents + a * N;
    if ((N & 3) == 0) {  // a * N is a multiple of 4 and the buffer is word aligned (checked on the host)
      const uint32_t* w = reinterpret_cast<const uint32_t*>(ca);
      for (int j = 0; j < (N >> 2); ++j) row |= w[j];
    } else {
      for (int j = 0; j < N; ++j) row |= ca[j];
    }
    row = row != 0;
    lanelet = col_flags[a * 4] != 0;   // byte 0 only: entry / exit / reset request are not collisions
  }
  const float n_i = evl_speed(vx, vy);
  double v_sp = agent ? (double)n_i : 0.0, v_dr = agent ? (double)dr : 0.0;  // padding lanes: +0.0
  for (int m = G >> 1; m > 0; m >>= 1) {  // evl_butterfly: lane ^ m stays inside the group (G is a power of two and the groups are aligned)
    v_sp = v_sp + __shfl_xor(v_sp, m);
    v_dr = v_dr + __shfl_xor(v_dr, m);
  }
  const unsigned long long group = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane - i);
  const uint32_t aa = (__ballot(row != 0) & group) != 0ull;
  const uint32_t al = (__ballot(lanelet != 0) & group) != 0ull;
  if (agent && trace_frame) {
    float* r = trace_frame + a * EVL_TRACE_COLS;
    r[0] = x; r[1] = y; r[2] = vx; r[3] = vy; r[4] = dr; r[5] = n_i; r[6] = (float)row; r[7] = (float)lanelet;
  }
  if constexpr (STUDY) {
    // group lane 0 fetches the env's eight accumulators first, all at once: the loads are in flight while the terms and the butterflies are formed (read one by one
    // between the stores below, each would wait for the store before it -- the compiler cannot tell the rows of `sums` apart -- and an attached rollout finds them cold)
    double old[EVL_STUDY_SUMS] = {};
    uint32_t old_n = 0;
    if (on && i == 0) {
#pragma unroll
      for (int k = 0; k < EVL_STUDY_SUMS; ++k) old[k] = st.sums[(size_t)k * B + b];
      old_n = st.n_act[b];
    }
    float term[EVL_STUDY_SUMS] = {};
    uint32_t act = 0;
    if (agent) {
      const float* ap = st.applied + a * 2;
      const float* nm = st.nominal + a * 2;
      float* cp = st.carry + a * 2;  // (v_prev, a_prev): this lane's own two words
      float carry[2] = {cp[0], cp[1]};
      act = evl_study_terms(st.initial, ap[0], ap[1], nm[0], nm[1], st.r_goal[a], st.r_agents[a], st.r_lane[a], carry, term);
      cp[0] = carry[0]; cp[1] = carry[1];
    }
    double v[EVL_STUDY_SUMS];
#pragma unroll
    for (int k = 0; k < EVL_STUDY_SUMS; ++k) v[k] = agent ? (double)term[k] : 0.0;  // padding lanes: +0.0
    for (int m = G >> 1; m > 0; m >>= 1) {
#pragma unroll
      for (int k = 0; k < EVL_STUDY_SUMS; ++k) v[k] = v[k] + __shfl_xor(v[k], m);
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(act != 0) & group);
    if (on && i == 0) {
#pragma unroll
      for (int k = 0; k < EVL_STUDY_SUMS; ++k) st.sums[(size_t)k * B + b] = evl_add(old[k], v[k]);
      st.n_act[b] = old_n + n;
      if (st.initial) { st.timer0[b * 2] = st.timer[b * 4 + 1]; st.timer0[b * 2 + 1] = st.timer[b * 4 + 2]; }
    }
  }
  if (on && i == 0) {
    acc.sum_speed[b] = evl_add(acc.sum_speed[b], v_sp);
    acc.sum_dref[b] = evl_add(acc.sum_dref[b], v_dr);
    acc.n_aa[b] = acc.n_aa[b] + aa;
    acc.n_al[b] = acc.n_al[b] + al;
    acc.frames[b] = acc.frames[b] + 1u;
  }
}

__global__ void __launch_bounds__(EVL_BLOCK) sigmaenv_eval_accumulate_kernel(const float* __restrict__ state, const float* __restrict__ dist_ref, const uint8_t* __restrict__ col_agents,
                                                                             const uint8_t* __restrict__ col_flags, int B, int N, int G, Acc acc, float* __restrict__ trace_frame) {
  sigma_poison_lds();
  accumulate_frame<false>(state, dist_ref, col_agents, col_flags, B, N, G, acc, trace_frame, NoStudy{});
}

// the study evaluator's instantiation: the same frame, plus the seven sums, the activation count and the carry of sigmaenv_eval.h
__global__ void __launch_bounds__(EVL_BLOCK) sigmaenv_eval_accumulate_study_kernel(const float* __restrict__ state, const float* __restrict__ dist_ref, const uint8_t* __restrict__ col_agents,
                                                                                   const uint8_t* __restrict__ col_flags, int B, int N, int G, Acc acc, float* __restrict__ trace_frame, Study st) {
  sigma_poison_lds();
  accumulate_frame<true>(state, dist_ref, col_agents, col_flags, B, N, G, acc, trace_frame, st);
}

__global__ void __launch_bounds__(EVL_BLOCK) sigmaenv_eval_finish_kernel(Acc acc, int B, int N, float* __restrict__ metrics, uint32_t* __restrict__ counts) {
  sigma_poison_lds();
  const long long b = (long long)blockIdx.x * EVL_BLOCK + threadIdx.x;
  if (b >= B) return;
  const uint32_t n_aa = acc.n_aa[b], n_al = acc.n_al[b], F = acc.frames[b];
  float m[4];
  evl_finish(acc.sum_speed[b], acc.sum_dref[b], n_aa, n_al, F, N, m);
  metrics[b * 4 + 0] = m[0]; metrics[b * 4 + 1] = m[1]; metrics[b * 4 + 2] = m[2]; metrics[b * 4 + 3] = m[3];
  if (counts) { counts[b * 3 + 0] = n_aa; counts[b * 3 + 1] = n_al; counts[b * 3 + 2] = F; }
}

// metrics [B,6], counts [B,4] (optional) of a study evaluator: evl_study_finish with the task counters' differences against the snapshot
__global__ void __launch_bounds__(EVL_BLOCK) sigmaenv_eval_study_finish_kernel(Acc acc, const double* __restrict__ sums, const uint32_t* __restrict__ n_act, const int32_t* __restrict__ timer0,
                                                                               const int32_t* __restrict__ timer, int B, int N, float* __restrict__ metrics, uint32_t* __restrict__ counts) {
  sigma_poison_lds();
  const long long b = (long long)blockIdx.x * EVL_BLOCK + threadIdx.x;
  if (b >= B) return;
  double sum[EVL_STUDY_SUMS];
#pragma unroll
  for (int k = 0; k < EVL_STUDY_SUMS; ++k) sum[k] = sums[(size_t)k * B + b];
  float m[EVL_STUDY_METRICS];
  uint32_t c[EVL_STUDY_COUNTS];
  evl_study_finish(sum, n_act[b], timer[b * 4 + 1] - timer0[b * 2], timer[b * 4 + 2] - timer0[b * 2 + 1], acc.frames[b], N, m, c);
#pragma unroll
  for (int k = 0; k < EVL_STUDY_METRICS; ++k) metrics[b * EVL_STUDY_METRICS + k] = m[k];
  if (counts) {
#pragma unroll
    for (int k = 0; k < EVL_STUDY_COUNTS; ++k) counts[b * EVL_STUDY_COUNTS + k] = c[k];
  }
}

// the snapshot of the task counters (columns 1, 2 of the timer buffer) a reset takes
__global__ void __launch_bounds__(EVL_BLOCK) sigmaenv_eval_study_snapshot_kernel(const int32_t* __restrict__ timer, int B, int32_t* __restrict__ timer0) {
  sigma_poison_lds();
  const long long b = (long long)blockIdx.x * EVL_BLOCK + threadIdx.x;
  if (b >= B) return;
  timer0[b * 2] = timer[b * 4 + 1];
  timer0[b * 2 + 1] = timer[b * 4 + 2];
}

}  // namespace eval

struct sigmaenv_eval {
  sigmaenv* owner = nullptr;  // the handle it was created on (null once that handle is destroyed)
  int B = 0, N = 0, trace_frames = 0;
  uint32_t frames0 = 0;       // test hook (sigmaenv_eval_args_t.debug_frames0): the frame count a reset starts from
  uint64_t frames = 0;        // frames accumulated since the last reset, as the host counts them (every launch adds one to every env)
  void* mem = nullptr;        // the accumulators
  eval::Acc acc{};
  float* trace = nullptr;     // [trace_frames, B, N, 8] or null
  bool study = false;         // sigmaenv_eval_args_t.study: every frame is a study frame
  void* study_mem = nullptr;  // sums f64 [7,B], timer0 i32 [B,2], n_act u32 [B], carry f32 [B,N,2]: one allocation
  double* study_sums = nullptr;
  int32_t* study_timer0 = nullptr;
  uint32_t* study_n_act = nullptr;
  float* study_carry = nullptr;
  size_t study_bytes() const { return (size_t)B * (EVL_STUDY_SUMS * sizeof(double) + 2 * sizeof(int32_t) + sizeof(uint32_t) + (size_t)N * 2 * sizeof(float)); }
};

static bool eval_owned(sigmaenv* h, const sigmaenv_eval* ev, const char* what) {
  if (!ev) { h->err = std::string(what) + ": null evaluator"; return false; }
  if (ev->owner != h) { h->err = std::string(what) + ": the evaluator belongs to another handle"; return false; }
  return true;
}

// sigmaenv_destroy: the handle's evaluators stay valid for sigmaenv_eval_destroy alone
static void eval_orphan(sigmaenv* h) {
  for (sigmaenv_eval* ev : h->evals) ev->owner = nullptr;
  h->evals.clear();
  h->eval_attached = nullptr;
}

extern "C" void sigmaenv_eval_destroy(sigmaenv_eval* ev) {
  if (!ev) return;
  if (sigmaenv* h = ev->owner) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);  // launches that still read or write its memory
    if (h->eval_attached == ev) h->eval_attached = nullptr;
    for (size_t k = 0; k < h->evals.size(); ++k)
      if (h->evals[k] == ev) { h->evals.erase(h->evals.begin() + (long)k); break; }
  }
  if (ev->mem) (void)hipFree(ev->mem);
  if (ev->trace) (void)hipFree(ev->trace);
  if (ev->study_mem) (void)hipFree(ev->study_mem);
  delete ev;
}

extern "C" int sigmaenv_eval_reset(sigmaenv_t* h, sigmaenv_eval* ev) {
  if (!h) return SIGMAENV_EINVAL;
  if (!eval_owned(h, ev, "eval_reset")) return SIGMAENV_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t B = (size_t)ev->B;
  HIPCHK(h, hipMemsetAsync(ev->mem, 0, B * (2 * sizeof(double) + 3 * sizeof(uint32_t)), h->stream));
  if (ev->frames0) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)ev->acc.frames, (int)ev->frames0, B, h->stream));
  if (ev->trace) HIPCHK(h, hipMemsetAsync(ev->trace, 0, (size_t)ev->trace_frames * B * ev->N * EVL_TRACE_COLS * sizeof(float), h->stream));
  if (ev->study) {  // zero sums, count and carry; the task counters as the handle's buffer holds them now
    HIPCHK(h, hipMemsetAsync(ev->study_mem, 0, ev->study_bytes(), h->stream));
    hipLaunchKernelGGL(eval::sigmaenv_eval_study_snapshot_kernel, dim3((unsigned)((h->B + EVL_BLOCK - 1) / EVL_BLOCK)), dim3(EVL_BLOCK), 0, h->stream, (const int32_t*)h->buf.timer, h->B,
                       ev->study_timer0);
    HIPCHK(h, hipGetLastError());
  }
  ev->frames = ev->frames0;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_eval_create(sigmaenv_t* h, const sigmaenv_eval_args_t* args, sigmaenv_eval** out) {
  if (!h || !out) return SIGMAENV_EINVAL;
  *out = nullptr;
  if (!args || args->trace_frames < 0 || args->debug_frames0 < 0 || (args->study != 0 && args->study != 1)) {
    h->err = "eval_create: arguments required, trace_frames >= 0, study 0 or 1";
    return SIGMAENV_EINVAL;
  }
  if ((long long)args->trace_frames * h->B * h->N * EVL_TRACE_COLS >= (1ll << 31)) { h->err = "eval_create: the trace [trace_frames, B, N, 8] must stay below 2^31 floats"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  auto* ev = new sigmaenv_eval();
  ev->B = h->B; ev->N = h->N; ev->trace_frames = args->trace_frames; ev->frames0 = (uint32_t)args->debug_frames0;
  ev->study = args->study != 0;
  const size_t B = (size_t)h->B;
  hipError_t e = hipMalloc(&ev->mem, B * (2 * sizeof(double) + 3 * sizeof(uint32_t)));
  if (e == hipSuccess && ev->trace_frames > 0) e = hipMalloc((void**)&ev->trace, (size_t)ev->trace_frames * B * h->N * EVL_TRACE_COLS * sizeof(float));
  if (e == hipSuccess && ev->study) e = hipMalloc(&ev->study_mem, ev->study_bytes());
  if (e != hipSuccess) {
    h->err = std::string("eval_create: hipMalloc: ") + hipGetErrorString(e);
    sigmaenv_eval_destroy(ev);
    return SIGMAENV_ENOMEM;
  }
  ev->acc.sum_speed = (double*)ev->mem;
  ev->acc.sum_dref = ev->acc.sum_speed + B;
  ev->acc.n_aa = (uint32_t*)(ev->acc.sum_dref + B);
  ev->acc.n_al = ev->acc.n_aa + B;
  ev->acc.frames = ev->acc.n_al + B;
  if (ev->study) {
    ev->study_sums = (double*)ev->study_mem;
    ev->study_timer0 = (int32_t*)(ev->study_sums + EVL_STUDY_SUMS * B);
    ev->study_n_act = (uint32_t*)(ev->study_timer0 + 2 * B);
    ev->study_carry = (float*)(ev->study_n_act + B);
  }
  ev->owner = h;
  h->evals.push_back(ev);
  const int rc = sigmaenv_eval_reset(h, ev);
  if (rc) { sigmaenv_eval_destroy(ev); return rc; }
  *out = ev;
  return SIGMAENV_OK;
}

// every refusal of one more frame, before any launch
static int eval_check_frames(sigmaenv* h, const sigmaenv_eval* ev, uint64_t more, const char* what) {
  if (more >= 1 && evl_full(ev->frames + more - 1, h->N)) {
    h->err = std::string(what) + ": frames * n_agents would reach 2^24 (the counts are reported through floats): finish and reset the evaluator first";
    return SIGMAENV_EINVAL;
  }
  return SIGMAENV_OK;
}

// does the handle's chain run the CBF-QP?  (launch_cbf_then_step asks the same question of the same function.)  The margin rewards win where a caller sets both
// reward flags: the chain then launches sigmaenv_cbf_rewards, no QP writes the nominal buffer, and the applied action stands for the nominal one.
static bool eval_nominal_from_cbf(const sigmaenv* h) {
  const bool qp = (h->cfg.rew_flags & SIGMAENV_REW_CBF_QP) != 0 && (h->cfg.rew_flags & SIGMAENV_REW_CBF) == 0;
  return evl_nominal_from_cbf(h->cbf_seg4 != nullptr, qp) != 0;
}

static int eval_accumulate_impl(sigmaenv* h, sigmaenv_eval* ev, const sigmaenv_eval_src_t* src, const sigmaenv_eval_study_src_t* ssrc) {
  const float* state = src && src->state ? src->state : h->buf.state;
  const float* dist_ref = src && src->dist_ref ? src->dist_ref : h->buf.dist_ref;
  const uint8_t* col_agents = src && src->col_agents ? src->col_agents : h->buf.col_agents;
  const uint8_t* col_flags = src && src->col_flags ? src->col_flags : h->buf.col_flags;
  const void* ptrs[] = {state, dist_ref, col_agents, col_flags};
  for (const void* p : ptrs)
    if ((uintptr_t)p & 3) { h->err = "eval_accumulate: an override that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  eval::Study st{};
  if (ev->study) {
    if (ssrc && (ssrc->initial != 0 && ssrc->initial != 1)) { h->err = "eval_accumulate_study: initial is 0 or 1"; return SIGMAENV_EINVAL; }
    const size_t row = (size_t)h->B * h->N;
    const float* rinfo = ssrc && ssrc->reward_info ? ssrc->reward_info : (const float*)h->buf.reward_info;
    st.applied = ssrc && ssrc->applied ? ssrc->applied : (const float*)h->buf.action;
    // the nominal action: an override; else what the CBF-QP left where the chain runs one; else the applied action of THIS frame (an override included)
    st.nominal = ssrc && ssrc->nominal ? ssrc->nominal : eval_nominal_from_cbf(h) ? (const float*)h->buf.cbf_nominal : st.applied;
    st.r_goal = rinfo + EVL_REW_GOAL * row;
    st.r_agents = rinfo + EVL_REW_AGENTS * row;
    st.r_lane = rinfo + EVL_REW_LANE * row;
    st.timer = ssrc && ssrc->timer ? ssrc->timer : (const int32_t*)h->buf.timer;
    st.carry = ev->study_carry; st.sums = ev->study_sums; st.n_act = ev->study_n_act; st.timer0 = ev->study_timer0;
    st.initial = ssrc ? ssrc->initial : 0;
    const void* sp[] = {st.applied, st.nominal, rinfo, st.timer};
    for (const void* p : sp)
      if ((uintptr_t)p & 3) { h->err = "eval_accumulate_study: an override that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  }
  const int rc = eval_check_frames(h, ev, 1, "eval_accumulate");
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const int G = evl_group(h->N), per_block = (EVL_BLOCK / 64) * (64 / G);
  float* trace_frame = ev->trace && ev->frames - ev->frames0 < (uint64_t)ev->trace_frames ? ev->trace + (size_t)(ev->frames - ev->frames0) * h->B * h->N * EVL_TRACE_COLS : nullptr;
  const dim3 grid((unsigned)((h->B + per_block - 1) / per_block));
  if (ev->study)
    hipLaunchKernelGGL(eval::sigmaenv_eval_accumulate_study_kernel, grid, dim3(EVL_BLOCK), 0, h->stream, state, dist_ref, col_agents, col_flags, h->B, h->N, G, ev->acc, trace_frame, st);
  else
    hipLaunchKernelGGL(eval::sigmaenv_eval_accumulate_kernel, grid, dim3(EVL_BLOCK), 0, h->stream, state, dist_ref, col_agents, col_flags, h->B, h->N, G, ev->acc, trace_frame);
  HIPCHK(h, hipGetLastError());
  ev->frames += 1;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_eval_accumulate(sigmaenv_t* h, sigmaenv_eval* ev, const sigmaenv_eval_src_t* src) {
  if (!h) return SIGMAENV_EINVAL;
  if (!eval_owned(h, ev, "eval_accumulate")) return SIGMAENV_EINVAL;
  return eval_accumulate_impl(h, ev, src, nullptr);  // (a study evaluator: a study frame from the handle's buffers, not an initial one)
}

extern "C" int sigmaenv_eval_accumulate_study(sigmaenv_t* h, sigmaenv_eval* ev, const sigmaenv_eval_src_t* src, const sigmaenv_eval_study_src_t* study_src) {
  if (!h) return SIGMAENV_EINVAL;
  if (!eval_owned(h, ev, "eval_accumulate_study")) return SIGMAENV_EINVAL;
  if (!ev->study) { h->err = "eval_accumulate_study: the evaluator was created without study"; return SIGMAENV_EINVAL; }
  return eval_accumulate_impl(h, ev, src, study_src);
}

extern "C" int sigmaenv_eval_study_finish(sigmaenv_t* h, sigmaenv_eval* ev, float* metrics, uint32_t* counts) {
  if (!h) return SIGMAENV_EINVAL;
  if (!eval_owned(h, ev, "eval_study_finish")) return SIGMAENV_EINVAL;
  if (!ev->study) { h->err = "eval_study_finish: the evaluator was created without study"; return SIGMAENV_EINVAL; }
  if (!metrics || ((uintptr_t)metrics & 3) || ((uintptr_t)counts & 3)) { h->err = "eval_study_finish: metrics is required, every tensor 4-byte aligned"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(eval::sigmaenv_eval_study_finish_kernel, dim3((unsigned)((h->B + EVL_BLOCK - 1) / EVL_BLOCK)), dim3(EVL_BLOCK), 0, h->stream, ev->acc, (const double*)ev->study_sums,
                     (const uint32_t*)ev->study_n_act, (const int32_t*)ev->study_timer0, (const int32_t*)h->buf.timer, h->B, h->N, metrics, counts);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_eval_finish(sigmaenv_t* h, sigmaenv_eval* ev, float* metrics, uint32_t* counts) {
  if (!h) return SIGMAENV_EINVAL;
  if (!eval_owned(h, ev, "eval_finish")) return SIGMAENV_EINVAL;
  if (!metrics || ((uintptr_t)metrics & 3) || ((uintptr_t)counts & 3)) { h->err = "eval_finish: metrics is required, every tensor 4-byte aligned"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(eval::sigmaenv_eval_finish_kernel, dim3((unsigned)((h->B + EVL_BLOCK - 1) / EVL_BLOCK)), dim3(EVL_BLOCK), 0, h->stream, ev->acc, h->B, h->N, metrics, counts);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_eval_attach(sigmaenv_t* h, sigmaenv_eval* ev) {
  if (!h) return SIGMAENV_EINVAL;
  if (ev && !eval_owned(h, ev, "eval_attach")) return SIGMAENV_EINVAL;
  h->eval_attached = ev;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_eval_get(sigmaenv_t* h, sigmaenv_eval* ev, int32_t what, void* host_out) {
  if (!h) return SIGMAENV_EINVAL;
  if (!eval_owned(h, ev, "eval_get")) return SIGMAENV_EINVAL;
  if (!host_out) { h->err = "eval_get: null destination"; return SIGMAENV_EINVAL; }
  const size_t B = (size_t)ev->B;
  const void* src = nullptr;
  size_t bytes = 0;
  if (what == SIGMAENV_EVAL_FRAMES_HOST) { *(uint64_t*)host_out = ev->frames; return SIGMAENV_OK; }
  if (what == SIGMAENV_EVAL_SUM_SPEED) { src = ev->acc.sum_speed; bytes = B * sizeof(double); }
  else if (what == SIGMAENV_EVAL_SUM_DREF) { src = ev->acc.sum_dref; bytes = B * sizeof(double); }
  else if (what == SIGMAENV_EVAL_N_AA) { src = ev->acc.n_aa; bytes = B * sizeof(uint32_t); }
  else if (what == SIGMAENV_EVAL_N_AL) { src = ev->acc.n_al; bytes = B * sizeof(uint32_t); }
  else if (what == SIGMAENV_EVAL_FRAMES) { src = ev->acc.frames; bytes = B * sizeof(uint32_t); }
  else if (what >= SIGMAENV_EVAL_STUDY_SUMS && what <= SIGMAENV_EVAL_STUDY_TIMER0) {
    if (!ev->study) { h->err = "eval_get: the evaluator was created without study"; return SIGMAENV_EINVAL; }
    if (what == SIGMAENV_EVAL_STUDY_SUMS) { src = ev->study_sums; bytes = EVL_STUDY_SUMS * B * sizeof(double); }
    else if (what == SIGMAENV_EVAL_STUDY_N_ACT) { src = ev->study_n_act; bytes = B * sizeof(uint32_t); }
    else if (what == SIGMAENV_EVAL_STUDY_CARRY) { src = ev->study_carry; bytes = B * (size_t)ev->N * 2 * sizeof(float); }
    else { src = ev->study_timer0; bytes = B * 2 * sizeof(int32_t); }
  } else if (what == SIGMAENV_EVAL_TRACE) {
    if (!ev->trace) { h->err = "eval_get: the evaluator was created without a trace"; return SIGMAENV_EINVAL; }
    src = ev->trace; bytes = (size_t)ev->trace_frames * B * ev->N * EVL_TRACE_COLS * sizeof(float);
  } else { h->err = "eval_get: unknown item " + std::to_string(what); return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SIGMAENV_OK;
}
