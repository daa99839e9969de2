// sigmaenv_isb.h -- the challenging initial-state buffer on the device, stated ONCE: the index arithmetic of the per-env history rings and of the bank, and the
// functions that turn a word of the generator into the three decisions (record, use, which entry).  Parameters.is_challenging_initial_state_buffer of the reference:
// the history of states (sigmarl/scenarios/road_traffic.py:702-708, :1226-1240), the recording on an agent-agent collision (:1415-1427 with CircularBuffer /
// InitialStateBuffer, sigmarl/helper_scenario.py:424-508) and the restart of a finished env from a random recording (:857-873, world_state_rt_sim.py:57-71, :162-178).
// In the reference the first USE of a recording raises (`if initial_state:` on an [N, 8] tensor, world_state_rt_sim.py:162): there is no golden; this header is the
// contract, held by the numpy twin tests/isb_check.py (tests/test_isb_check.py compiles this header alone and compares bit for bit).  The kernels of sigmaenv_isb.inc
// call these functions on the device.
//
// Plain C++: no HIP include and, of the library, only sigmaenv_dist.h (the generator's draw table and uniforms, plain C++ as well).  The library compiles it as
// __host__ __device__ __forceinline__; a host program defines SIGMA_HD as `static inline` first and includes this header alone.
//
// An ENTRY of one env: the N rows of SIGMAENV_BUF_STATE (8 fp32 each) and the N rows of SIGMAENV_BUF_PATH (4 int32 each) -- exactly what sigmaenv_reset takes.
//
// The HISTORY: one ring of S = n_steps_stored entries per env with held[b] and head[b].
//   push           writes slot head, then head = (head + 1) mod S, held = min(held + 1, S)                                                        isb_push
//   nth_latest(n)  slot (head - n) mod S when held >= n, else slot 0 (CircularBuffer.get_latest); with n = S: the oldest state held since the ring was last
//                  cleared                                                                                                                        isb_nth_latest
// The BANK: `capacity` entries with the device words ptr and count (CircularBuffer.add).
//
// record (on the frame a step left, before any reset), in this order:
//   1. push the current rows of every env: the collision state itself is the newest entry (road_traffic.py:1240 runs before done())
//   2. collided[b] = any non-zero byte of SIGMAENV_BUF_COL_AGENTS[b]
//   3. env b records iff collided[b] and u > 1.0f - p_record (fp32), u = isb_uniform(rng_u32(seed, counter, env_index_base + b, 0, DRAW_ISB_RECORD))   isb_records
//   4. the R recording envs in ascending b have ranks k = 0 .. R - 1 (isb_ranks); rank k writes nth_latest(S) of its env to bank slot (ptr + k) mod capacity, and only
//      if k >= R - capacity (isb_rank_kept): the result of adding them one after the other, later entries overwriting earlier ones.  Then ptr = (ptr + R) mod capacity,
//      count = min(count + R, capacity)                                                                                                            isb_bank_slot, isb_ptr_after, isb_count_after
//   5. pending[b] = env not done and some SIGMAENV_BUF_COL_FLAGS[b, ., 3] set (a single-agent reset is coming: sigmaenv_auto_reset)
// restart (before sigmaenv_auto_reset): an env with done[b] restarts from the bank iff count >= 1 and u < p_use, u from DRAW_ISB_USE (isb_uses); count includes this
//   step's recordings (the reference's done() records before the resets).  The entry is j = isb_index(word of DRAW_ISB_INDEX, count) in [0, count).
// settle (after sigmaenv_auto_reset): every env whose episodes_reset differs from the bank's copy, and every env with pending[b]: the ring is cleared, the current rows
//   are pushed, the copy refreshed (road_traffic.py:909-923: every reset_world_at, single-agent ones included)                                     isb_settles
// The three draws are keyed by the step's own (seed, counter), env = env_index_base + b, agent 0.
//
// Departures from the reference:
//   (a) the reference keeps (x, y, rot, vx, vy, scenario, path, point) per agent and restores pos / rot / vel only, so speed and steering stay at the previous
//       episode's values; here the whole state row is kept and restored;
//   (b) the reference has ONE ring for the whole batch and a reset of any env clears it for every env; here one ring per env (the two coincide at B = 1; per env
//       is the only reading that means anything at B > 1);
//   (c) the reference draws the record decision once per step for all envs; here once per env;
//   (d) the reference's use of a recording raises (above); here it is sigmaenv_reset(full_env = 1) with the entry's rows.
#ifndef SIGMAENV_ISB_H
#define SIGMAENV_ISB_H
#include <stdint.h>

#include "sigmaenv_dist.h"  // the generator, its draw table and the word conversions: as stand-alone as this header

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define ISB_CHUNK 1024          /* envs per chunk of the record workgroup's walk over the batch (= its threads) */
#define ISB_MAX_CAPACITY 65536  /* bank entries */
#define ISB_MAX_STEPS_STORED 1024

// ---- the ring of one env ---------------------------------------------------------------------------------------------------------------------------------------------
// returns the slot written; head and held advance
SIGMA_HD int isb_push(int* head, int* held, int S) {
  const int slot = *head;
  *head = slot + 1 == S ? 0 : slot + 1;
  *held = *held + 1 < S ? *held + 1 : S;
  return slot;
}
SIGMA_HD int isb_nth_latest(int head, int held, int n, int S) {
  if (held < n) return 0;
  const int d = (head - n) % S;  // head in [0, S), n >= 1: d in (-S, S)
  return d < 0 ? d + S : d;
}

// ---- the bank --------------------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_HD int isb_bank_slot(int ptr, int k, int capacity) { return (int)(((int64_t)ptr + k) % capacity); }
SIGMA_HD int isb_rank_kept(int k, int R, int capacity) { return k >= R - capacity; }
SIGMA_HD int isb_ptr_after(int ptr, int R, int capacity) { return (int)(((int64_t)ptr + R) % capacity); }
SIGMA_HD int isb_count_after(int count, int R, int capacity) { return (int64_t)count + R < capacity ? count + R : capacity; }
// the exclusive ranks of the recording envs in ascending b (the kernel forms them with ballots and a workgroup scan: the same numbers); returns R
static inline int isb_ranks(const uint8_t* records, int B, int* rank) {
  int R = 0;
  for (int b = 0; b < B; ++b) rank[b] = records[b] ? R++ : -1;
  return R;
}

// ---- a word -> a decision --------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_HD float isb_uniform(uint32_t k) { return rng_uniform(k); }  // U[0, 1), exact in fp32
SIGMA_HD uint32_t isb_word(uint64_t seed, uint64_t counter, uint32_t env, uint32_t draw) { return rng_u32(seed, counter, env, 0u, draw); }
SIGMA_HD int isb_records(int collided, uint32_t word, float p_record) { return collided && isb_uniform(word) > 1.0f - p_record; }
SIGMA_HD int isb_uses(int done, int count, uint32_t word, float p_use) { return done && count >= 1 && isb_uniform(word) < p_use; }
SIGMA_HD int isb_index(uint32_t word, int count) { return (int)rng_below(word, (uint32_t)count); }  // [0, count)
SIGMA_HD int isb_settles(int episodes_reset, int episodes_copy, int pending) { return episodes_reset != episodes_copy || pending; }
#endif  // SIGMAENV_ISB_H
