/*
 * sigmaenv.h -- C-ABI of the MI355X-native vectorized multi-agent CAV environment step.
 *
 * The reference (bassamlab/SigmaRL) has no FFI: its boundary for this path is the
 * VMAS plugin surface driven by TorchRL's VmasEnv.  This header defines the C-ABI
 * that sits directly underneath that surface; every entry point cites the reference
 * interface it replaces (paths relative to /root/reference).
 *
 *   sigmaenv_create        <- ScenarioRoadTraffic.make_world            sigmarl/scenarios/road_traffic.py:104-110,112-768
 *                             WorldStateRT._init_stateful_parameters     sigmarl/scenarios/world_state/world_state_rt/world_state_rt.py:119-277
 *                             (+ _extend_map_related_ref_path :279-311, path padding :313-420)
 *   sigmaenv_reset         <- ScenarioRoadTraffic.reset_world_at         sigmarl/scenarios/road_traffic.py:816-923
 *                             WorldStateRTSimulation.reset               .../world_state_rt_sim.py:73-141 (deterministic part:
 *                             the random draws of :215-311 are made by the caller and passed in)
 *                             reset_init_distances_and_short_term_ref_path .../world_state_rt.py:422-576
 *   sigmaenv_step          <- WorldCustom.step                           sigmarl/helper_training.py:797-861
 *                             KinematicBicycleModel.ode/.step            sigmarl/dynamics.py:62-192
 *                             ScenarioRoadTraffic.reward (all agents)    sigmarl/scenarios/road_traffic.py:925-1332
 *                             ScenarioRoadTraffic.observation (all)      :1334-1366  (+ observation_provider_rt.py:345-961)
 *                             ScenarioRoadTraffic.done                   :1368-1487  (flags + reset requests; the host performs the resets)
 *   sigmaenv_observe       <- ScenarioRoadTraffic.observation called again after a reset (VmasEnv reset path)
 *   sigmaenv_auto_reset    <- TorchRL step_and_maybe_reset -> Environment.reset_at -> reset_world_at for done envs, with the
 *                             rejection sampler of world_state_rt_sim.py:215-311 run on device from a counter-based RNG
 *                             (distributional parity only: the reference draws from torch's global generator)
 *   sigmaenv_get           <- the tensors ScenarioRoadTraffic.info exposes   sigmarl/scenarios/road_traffic.py:1489-1635
 *
 * Conventions: return 0 on success, negative SIGMAENV_E* otherwise.  The handle is thread-compatible (the caller
 * serialises calls).  All work is enqueued on the HIP stream given at create; no call synchronises the host except
 * sigmaenv_create / sigmaenv_destroy / sigmaenv_reset (host inputs are copied before it returns).  Output buffers are owned by
 * the library until destroy; pointers returned by sigmaenv_get are DEVICE pointers valid for the handle's lifetime.
 *
 * The CPU oracle (oracle/sigmaenv_oracle.c, test infrastructure) exports the same entry points with the prefix
 * sigmaenv_oracle_ operating on host memory.
 */
#ifndef SIGMAENV_H
#define SIGMAENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIGMAENV_ABI_VERSION 5

/* error codes */
#define SIGMAENV_OK 0
#define SIGMAENV_EINVAL (-22)      /* bad argument / unsupported configuration */
#define SIGMAENV_ENOMEM (-12)
#define SIGMAENV_EHIP (-5)         /* HIP runtime error, see sigmaenv_last_error */
#define SIGMAENV_ENODEV (-19)      /* no usable gfx950 device */

/* distance_type (helper_scenario.py:999-1145) */
#define SIGMAENV_DIST_C2C 0
#define SIGMAENV_DIST_MTV 1

/* rew_flags, decoded from Parameters.rew_method exactly as road_traffic.py:1056-1151 tests the string */
#define SIGMAENV_REW_DISTANCE 1     /* "distance" in rew_method */
#define SIGMAENV_REW_TTC 2          /* "ttc" in rew_method */
#define SIGMAENV_REW_EXACT_SPARSE 4 /* rew_method == "sparse" */
#define SIGMAENV_REW_HAS_SPARSE 8   /* "sparse" in rew_method */
#define SIGMAENV_REW_CBF_QP 32      /* "cbf" in rew_method with Parameters.is_solve_qp == True: the step penalises the deviation of the applied
                                     * action from SIGMAENV_BUF_CBF_NOMINAL, written by sigmaenv_cbf_qp (road_traffic.py:1112-1135) */
#define SIGMAENV_REW_CBF 16         /* "cbf" in rew_method with Parameters.is_solve_qp == False: the step adds the three margin
                                     * channels written by sigmaenv_cbf_rewards (road_traffic.py:1112-1151) */

/* n_points_short_term (config.json:27: 3) is a BUILD constant of the library: it sizes the observation row, the LDS tile layout and the start table, and
 * the kernels unroll over it.  libsigmaenv.so is built for 3; `make NS=k` (1 <= k <= SIGMAENV_MAX_SHORT_TERM) builds libsigmaenv_ns<k>.so for another
 * value from the same sources, and sigmaenv_n_short_term() reports what a loaded library was built for. */
#ifndef SIGMAENV_N_SHORT_TERM
#define SIGMAENV_N_SHORT_TERM 3
#endif
#define SIGMAENV_MAX_SHORT_TERM 8
#define SIGMAENV_MAX_NEARING 4      /* n_nearing_agents_observed <= 4 (default 2) */
#define SIGMAENV_MAX_AGENTS 64
#define SIGMAENV_N_REWARD_INFO 12   /* RewardInfo fields, helper_scenario.py:101-114 */
#define SIGMAENV_CBF_MAX_CIRCLES 4  /* Parameters.n_circles_approximate_vehicle <= 4 (default 3) */

typedef struct sigmaenv_config {
  int32_t abi_version;   /* SIGMAENV_ABI_VERSION */
  int32_t n_envs;        /* VMAS batch_dim (this shard) */
  int32_t n_agents;
  int32_t distance_type; /* SIGMAENV_DIST_* ; Parameters.is_use_mtv_distance */
  int32_t rew_flags;     /* SIGMAENV_REW_* */
  int32_t is_testing_mode;
  int32_t has_entry_exit;/* scenario_type != "cpm_entire": per-agent reset requests for entry/exit leavers (road_traffic.py:1456-1473) */
  int32_t max_steps;     /* Parameters.max_steps */
  int32_t n_nearing;     /* min(n_nearing_agents_observed, n_agents-1) */
  int32_t envs_per_group;   /* envs per workgroup of the step kernel (envs_per_group * n_agents <= 64); 0: chosen by the library
                             * (64 / n_agents, fewer for small batches).  Callers that step several handles concurrently on
                             * different streams -- env shards of one GPU -- pass 64 / n_agents. */
  float dt;
  float length, width, l_f, l_r;                    /* constants.py:628-636 */
  float max_speed, max_steering;                    /* constants.py:637-640 */
  float min_acc, max_acc, min_steering_rate, max_steering_rate;
  float world_x_dim, world_y_dim;                   /* parser.bounds */
  float lane_width;                                 /* SCENARIOS[...]["lane_width"]; normalizers.distance_lanelet = 3*lane_width */
  float reward_progress, reward_reach_goal;         /* road_traffic.py:133-137,217-219 */
  float penalty_near_boundary, penalty_near_other_agents;
  float penalty_collide_with_agents, penalty_collide_with_boundaries;
  float threshold_near_boundary_low, threshold_near_boundary_high;
  float threshold_near_other_agents_low, threshold_near_other_agents_high;
  float ttc_low, ttc_high;
  /* Each low / high pair above feeds decreasing_fcn(type="linear") (helper_scenario.py:960-996): 1 - (clamp(x, low, high) - low) / (high - low).
   * DEGENERATE pair, high == low: the reference divides 0 by 0 there, and so does the library -- the term is NaN for EVERY entry, the proximity
   * channel of SIGMAENV_BUF_REWARD_INFO is NaN, and the step reward, clamped with fmin / fmax (which drop a NaN operand), is -1 for every agent;
   * states, distances and observations are unaffected.  Device and oracle agree word for word (tests/test_constants_host.py,
   * tests/test_gpu_constants.py).  Callers that sweep the thresholds must keep high > low. */
  float penalty_deviate_from_cbf_vel, penalty_deviate_from_cbf_steer; /* road_traffic.py:238-243 (-5/100 each); SIGMAENV_REW_CBF_QP */
  int32_t is_apply_mask;        /* Parameters.is_apply_mask: observed neighbours at or beyond distance_mask_agents are masked (vertices and
                                 * distance := 1, velocity := 0; observation_provider_rt.py:638-749).  The distance criterion is the only live
                                 * one in ego view: the reference computes the agents' lanelets (for the mask by lanelet relation) in its
                                 * bird-view branch only (:537-588), so that mask stays empty (map_manager.py:21,102-118). */
  float distance_mask_agents;   /* thresholds.distance_mask_agents = 5 * length (road_traffic.py:663) */
  int32_t obs_flags;            /* SIGMAENV_OBS_*: non-default observation layout (below); 0 = the reference's config.json defaults */
  float reset_agent_fixed_duration; /* Parameters.reset_agent_fixed_duration [s], 0 = off: every env is also done when t = step * dt (fp32) is a
                                     * non-zero multiple of it (t % duration == 0, road_traffic.py:1388-1397, :1431, :1454) */
  int32_t env_index_base;       /* index of this handle's env 0 in the whole batch (shard_range begin when the batch is sharded over handles / GPUs, else
                                 * 0): every device-side random draw -- reset sampler, observation noise, action sampling -- is keyed on
                                 * (seed, counter, env_index_base + local env, agent, draw), so a sharded batch draws exactly what the unsharded
                                 * batch draws, whatever the number of shards */
  float obs_noise_level;        /* Parameters.obs_noise_level when Parameters.is_obs_noise, else 0 (no noise).  observation_provider_rt.py:613-618:
                                 * `obs + obs_noise_level * rand_like(obs)`, i.e. uniform noise in [0, level) on every element of every observation
                                 * row, drawn at every observation() call.  Here element k of agent i of env b receives level * u with
                                 * u = (rng(obs_noise_seed, episodes_reset(b) * 65537 + timer.step(b), env_index_base + b, i, DRAW_OBS_NOISE + k) >> 8) / 2^24
                                 * (the counter-based generator the reset sampler uses; its draw table: sigmarl_amd/csrc/sigmaenv_dist.h): a pure function of the env's own counters, hence the same in the
                                 * fused / separate / n-step launches and for any sharding.  Applied on the DEVICE to SIGMAENV_BUF_OBS, to the rollout
                                 * record and therefore to what sigmaenv_actor_* / sigmaenv_rollout read. */
  uint32_t obs_noise_seed_lo, obs_noise_seed_hi; /* Parameters.random_seed */
  int32_t n_points_short_term;  /* Parameters.n_points_short_term; 0 = the library's build constant.  A value other than SIGMAENV_N_SHORT_TERM of the loaded
                                 * library is refused (SIGMAENV_EINVAL): load the build for that value (libsigmaenv_ns<k>.so) */
  int32_t reserved[3];          /* must be 0 */
} sigmaenv_config_t;

/* Unpadded reference-path table (output of the map parser, sigmarl/map_manager.py:13-40).  The library builds the padded
 * per-path polylines itself exactly as world_state_rt.py:279-420 does (centre line + 6 extended points + last-point padding;
 * boundaries padded with their last point). */
typedef struct sigmaenv_map {
  int32_t n_paths;
  int32_t stride_points;     /* points per path in the arrays below */
  const float* center;       /* [n_paths, stride_points, 2]  ref_path["center_line"] */
  const float* left;         /* [n_paths, stride_points, 2]  ref_path["left_boundary_shared"] */
  const float* right;        /* [n_paths, stride_points, 2]  ref_path["right_boundary_shared"] */
  const float* yaw;          /* [n_paths, stride_points]     ref_path["center_line_yaw"] */
  const int32_t* n_center;   /* [n_paths] */
  const int32_t* n_left;
  const int32_t* n_right;
  const uint8_t* is_loop;    /* [n_paths] */
} sigmaenv_map_t;

/* buffers readable through sigmaenv_get; shapes with B = n_envs, N = n_agents, K = n_nearing, D = obs_dim */
typedef enum sigmaenv_buf {
  SIGMAENV_BUF_STATE = 0,        /* f32 [B,N,8]  x, y, psi, speed, steering, vx, vy, sideslip                */
  SIGMAENV_BUF_PREV_POS = 1,     /* f32 [B,N,2]  state_buffer.get_latest(1)[..., 0:2]                      */
  SIGMAENV_BUF_VERTICES = 2,     /* f32 [B,N,5,2]                                                           */
  SIGMAENV_BUF_PATH = 3,         /* i32 [B,N,4]  global path index, scenario_id, path_id, point_id        */
  SIGMAENV_BUF_SHORT_TERM = 4,   /* f32 [B,N,3,2]                                                           */
  SIGMAENV_BUF_DIST_REF = 5,     /* f32 [B,N]                                                               */
  SIGMAENV_BUF_DIST_LEFT = 6,    /* f32 [B,N,5]  CG - width/2, then the 4 corners                          */
  SIGMAENV_BUF_DIST_RIGHT = 7,   /* f32 [B,N,5]                                                             */
  SIGMAENV_BUF_DIST_BOUND = 8,   /* f32 [B,N]                                                               */
  SIGMAENV_BUF_CLOSEST = 9,      /* i32 [B,N,3]  closest point on ref path / left / right (already +1)      */
  SIGMAENV_BUF_DIST_AGENTS = 10, /* f32 [B,N,N]                                                             */
  SIGMAENV_BUF_COL_AGENTS = 11,  /* u8  [B,N,N]                                                             */
  SIGMAENV_BUF_COL_FLAGS = 12,   /* u8  [B,N,4]  with_lanelets, with_entry_segments, with_exit_segments, reset_request */
  SIGMAENV_BUF_REWARD = 13,      /* f32 [B,N]                                                               */
  SIGMAENV_BUF_REWARD_INFO = 14, /* f32 [12,B,N] RewardInfo fields in declaration order                     */
  SIGMAENV_BUF_OBS = 15,         /* f32 [B,N,D]                                                             */
  SIGMAENV_BUF_NEARING = 16,     /* i32 [B,N,K]                                                             */
  SIGMAENV_BUF_DONE = 17,        /* u8  [B]                                                                 */
  SIGMAENV_BUF_TIMER = 18,       /* i32 [B,4]    timer.step, num_task_tries, task_success_times, episodes_reset */
  SIGMAENV_BUF_ACTION = 19,      /* f32 [B,N,2]  clamped action (agent.action.u after WorldCustom.step)     */
  SIGMAENV_BUF_CBF_NOMINAL = 20, /* f32 [B,N,2] world_state.nominal_action_{vel,steer} as the CBF-QP leaves them (cbf_qp.py:1315-1379) */
  SIGMAENV_BUF_COUNT = 21
} sigmaenv_buf_t;

typedef struct sigmaenv sigmaenv_t;

/* obs_dim for the default observation flags (config.json:36-45): 1 + 2*3 + 3 + K*(8+2+1) */
int sigmaenv_obs_dim(int32_t n_nearing);

/* Non-default observation flags of Parameters (ego view, partial observation; observation_provider_rt.py:594-925).  Row layout:
 *   [own]     speed | steering (STEERING) | short-term path 2*3 | distance to the centre line (unless NO_DIST_CENTER) | left | right boundary
 *   [other k] vertices 8  (NO_VERTICES: position 2, relative rotation 1, length 1, width 1) | velocity 2 | steering (STEERING) |
 *             distance (unless NO_DIST_AGENTS) | its short-term path 2*3 in the ego frame (REF_OTHERS)
 * normalised as update_state does (:345-536: positions by 10 lengths, rotations / steering by 2 pi, lengths / widths by 10 lengths).
 * With obs_flags != 0 SIGMAENV_BUF_OBS has sigmaenv_obs_dim_full columns; the configured row is assembled INSIDE every kernel that refreshes observations
 * (the fused step incl. its T-step loop, the resets, sigmaenv_observe), and the rollout record (sigmaenv_set_slab, sigmaenv_step_autoreset_n, sigmaenv_rollout*)
 * carries that row: [N * D | N | 1] floats per env with D = sigmaenv_obs_dim_full. */
#define SIGMAENV_OBS_STEERING 1        /* Parameters.is_obs_steering */
#define SIGMAENV_OBS_REF_OTHERS 2      /* Parameters.is_observe_ref_path_other_agents */
#define SIGMAENV_OBS_NO_VERTICES 4     /* Parameters.is_observe_vertices == False */
#define SIGMAENV_OBS_NO_DIST_AGENTS 8  /* Parameters.is_observe_distance_to_agents == False */
#define SIGMAENV_OBS_NO_DIST_CENTER 16 /* Parameters.is_observe_distance_to_center_line == False */
#define SIGMAENV_OBS_BIRD_VIEW 32      /* Parameters.is_ego_view == False (:537-575, :855-884): world-frame positions / vertices / reference points divided by
                                        * (world_x_dim, world_y_dim), velocities as (vx, vy) / max_speed, rotations wrapped / 2 pi; [own] gains position 2 and
                                        * rotation 1 in front, its velocity has both components */
#define SIGMAENV_OBS_BOUNDARY_POINTS 64 /* Parameters.is_observe_distance_to_boundaries == False: instead of the two boundary distances, [own] carries the 5 points
                                        * of each boundary around its closest point (world_state_rt.py:686-724: indices closest - 2 ... closest + 2 with the loop
                                        * rule of get_short_term_reference_path; a negative index addresses the padded polyline from its end, as torch does) */
#define SIGMAENV_OBS_OPPONENT_PAD 128  /* Parameters.is_using_opponent_modeling: the row ends with n_nearing x 2 placeholder columns for the tentative actions of
                                        * the observed neighbours (F.pad, observation_provider_rt.py:606-611), zero before the sensor noise is added;
                                        * sigmaenv_opponent_fill writes the actions into them */
#define SIGMAENV_OBS_FULL 256          /* Parameters.is_partial_observation == False (observation_provider_rt.py:622-800, the `else` branch at :756): every agent observes
                                        * ALL agents in index order instead of its n_nearing nearest -- only with SIGMAENV_OBS_BIRD_VIEW (the ego view raises in the
                                        * reference: its reshape of the per-agent length / width scalars fails).  [own] as in bird view; then, for each of the
                                        * K = n_nearing chunks the reference's reshape(B, n_nearing_agents, -1) cuts every feature tensor into (:790-816), chunk k of:
                                        * vertices [N,4,2] (NO_VERTICES: positions [N,2], rotations [N], lengths [N], widths [N]) | velocities [N,2] | steering [N]
                                        * (STEERING) | the mutual distances [N,N], ALL ZERO in this view (:776-778; unless NO_DIST_AGENTS) | short-term paths
                                        * [N,NS,2] (REF_OTHERS); no mask; SIGMAENV_BUF_NEARING stays zero.  N x (feature width) must be a multiple of K for every
                                        * feature (torch.reshape raises otherwise: SIGMAENV_EINVAL) */
int sigmaenv_obs_dim_ex(int32_t n_nearing, int32_t obs_flags);
/* Row width for ANY flags, SIGMAENV_OBS_FULL included (equals sigmaenv_obs_dim_ex without it); SIGMAENV_EINVAL for a combination the reference raises on. */
int sigmaenv_obs_dim_full(int32_t n_agents, int32_t n_nearing, int32_t obs_flags);
int sigmaenv_n_short_term(void);   /* SIGMAENV_N_SHORT_TERM of this build */
/* First 16 hex digits of the SHA-256 over the library's sources in the order of sigmarl_amd/csrc/Makefile's SRC list, baked in at build time.  The built .so files
 * travel to the GPU box un-rebuilt: sigmarl_amd.capi recomputes the value from the tree and refuses a library that was built from other sources (a stale .so would
 * otherwise be tested silently: VERDICT r5).  "unknown" for a build outside the Makefile. */
const char* sigmaenv_build_id(void);

/* device_id: HIP device ordinal.  hip_stream: hipStream_t to enqueue on (NULL = the device's default stream). */
int sigmaenv_create(const sigmaenv_config_t* cfg, const sigmaenv_map_t* map, int device_id, void* hip_stream,
                    sigmaenv_t** out);
void sigmaenv_destroy(sigmaenv_t* h);
const char* sigmaenv_last_error(const sigmaenv_t* h);

/* Host-chosen resets.  n entries (HOST pointers), entry k resets agent agent_idx[k] of env env_idx[k]:
 *   path_ids[k*4 + {0,1,2,3}] = global path index, scenario_id, path_id, point_id
 *   state8[k*8 + ...]         = x, y, psi, speed, steering, vx, vy, sideslip
 * After applying the entries every touched env gets: initial distances / vertices / short-term path of the reset agents,
 * mutual distances recomputed, collision flags cleared, prev_pos := pos (road_traffic.py:888-923).
 * full_env != 0: additionally timer.step := 0 and the clamped-action buffer of the env is zeroed (world.reset(e)). */
int sigmaenv_reset(sigmaenv_t* h, int32_t n, const int32_t* env_idx, const int32_t* agent_idx, const int32_t* path_ids,
                   const float* state8, int32_t full_env);

/* One fused environment step for all envs.  actions: DEVICE pointer f32 [B,N,2] (v_cmd, delta_cmd), not modified. */
int sigmaenv_step(sigmaenv_t* h, const float* actions);

/* Recompute observations from the current state (observation() called again after resets). */
int sigmaenv_observe(sigmaenv_t* h);

/* Device-side resets.  (1) Every env whose done flag is set: rejection sampling of collision-free starts (bounded retries) on the
 * paths [path_first, path_first + path_count) of the table, then the same deterministic reset as sigmaenv_reset(full_env=1).
 * (2) In every unfinished env, every agent with a pending reset request (SIGMAENV_BUF_COL_FLAGS[...,3]: left through an entry /
 * exit segment, or collided in testing mode -- the per-agent resets ScenarioRoadTraffic.done performs, road_traffic.py:1435-1447,
 * 1456-1473) is re-placed against all other agents, as sigmaenv_reset(full_env=0) would.  Touched envs get a fresh observation.
 * seed/counter select the counter-based random stream. */
int sigmaenv_auto_reset(sigmaenv_t* h, uint64_t seed, uint64_t counter, int32_t path_first, int32_t path_count);

/* scenario_type "cpm_mixed" (_reset_scenario_related_ref_paths, world_state_rt_sim.py:313-358): every finished env draws one of n_lists (<= 4)
 * sub-scenarios with the given probabilities (torch.multinomial(cpm_scenario_probabilities): weights, normalised) -- sub-scenario k + 1 owns the paths
 * [first[k], first[k] + count[k]) -- writes it to SIGMAENV_BUF_PATH[..., 1] of all its agents and places them on that list; a per-agent reset keeps the
 * agent's sub-scenario (:325-328).  Every device-side reset entry point takes the lists instead of one path range when called with
 * path_count = SIGMAENV_SCENARIO_LISTS (path_first is then ignored).  The draw is draw 5000 of agent 0 of the env's (seed, counter) stream. */
#define SIGMAENV_SCENARIO_LISTS (-1)
int sigmaenv_set_scenario_lists(sigmaenv_t* h, int32_t n_lists, const int32_t* first, const int32_t* count, const float* probabilities);

/* sigmaenv_step immediately followed by sigmaenv_auto_reset, in ONE launch: after the record of the step is complete (all
 * buffers, and the rollout slab row with the terminal observation / reward / done flag), the workgroup that still holds the tile
 * in LDS re-places its finished envs / requesting agents.  Bit-identical end state to the two separate calls; what a rollout
 * loop with TorchRL's step_and_maybe_reset semantics needs per step (sigmarl/helper_training.py:687-788).  Note: the terminal
 * observation is only visible in the slab -- SIGMAENV_BUF_OBS holds the post-reset observation when the call returns. */
int sigmaenv_step_autoreset(sigmaenv_t* h, const float* actions, uint64_t seed, uint64_t counter, int32_t path_first, int32_t path_count);

/* sigmaenv_step_autoreset for n handles in one call (env shards of one GPU, each on its own stream): handle k records into
 * slab_ptrs[k] (array may be NULL: record targets unchanged) and steps on actions[k] with seeds[k]. */
int sigmaenv_step_autoreset_many(sigmaenv_t** hs, int32_t n, const float* const* actions, float* const* slab_ptrs, const uint64_t* seeds,
                                 uint64_t counter, int32_t path_first, int32_t path_count);

/* n_steps fused steps of every env in ONE launch -- the reference's rollout loop over a chunk of steps for actions that are already on the
 * device (sigmarl/helper_training.py:687-788: `for t in range(max_steps): policy; env.step; step_mdp`, and TorchRL's step_and_maybe_reset
 * per step).  Step t reads actions + t * action_stride floats ([B, N, 2]; stride 0 repeats one block), draws its resets from
 * (seed, counter0 + t) and records into slab + t * slab_stride floats ([B, N (D + 1) + 1]; slab may be NULL).  End state, record rows and reset
 * draws are bit-identical to n_steps calls of sigmaenv_step_autoreset with sigmaenv_set_slab(slab + t * slab_stride) before call t; the
 * pointer of sigmaenv_set_slab itself is neither used nor changed.  Every wavefront walks its own env tile through the n_steps steps (envs
 * never read each other), so launch ramp / tail and the host's enqueue are paid once per call.  With a "cbf" rew_method (after sigmaenv_cbf_attach; EINVAL
 * without it) the chunk is n_steps x (sigmaenv_cbf_rewards | sigmaenv_cbf_qp on step t's actions, then the fused step -- with the QP's safe action when
 * is_apply_cbf_action / grouping say so) enqueued back to back: CBFQP.update_qp between policy and env.step (helper_training.py:1616-1627), same bits as the
 * per-step calls, the host out of the loop. */
int sigmaenv_step_autoreset_n(sigmaenv_t* h, const float* actions, int32_t n_steps, int64_t action_stride, float* slab, int64_t slab_stride,
                              uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count);

int sigmaenv_get(sigmaenv_t* h, sigmaenv_buf_t which, void** dev_ptr, size_t* bytes);

/* The lanelet tables of the map for the lanelet-relation mask of the BIRD-VIEW observation (sigmarl/map_manager.py:41-118,
 * observation_provider_rt.py:577-665): with SIGMAENV_OBS_BIRD_VIEW and is_apply_mask an observed neighbour is masked when its lanelet is not
 * listed among the neighbouring lanelets of the ego's lanelet (OR the distance criterion).  centers: HOST f32 [n_lanelets, max_points, 2], the
 * centre lines of parser.lanelets_all stacked and ZERO-padded as MapManager.determine_current_lanelet pads them (the padding is a candidate point
 * at the origin there, and here); an agent's lanelet = argmin over lanelets of the minimal squared distance to its points, first index on ties.
 * neighbors: HOST u64 [n_lanelets], bit j of entry i = lanelet j is in parser.neighboring_lanelets_idx[i].  n_lanelets <= 64.  Maps whose parser
 * has no neighbour table (the CPM map) do not call this: the mask by lanelets then masks nobody, as in the reference.  Copied to the device. */
int sigmaenv_set_lanelets(sigmaenv_t* h, int32_t n_lanelets, int32_t max_points, const float* centers, const uint64_t* neighbors);

/* Opponent modelling, the observation half (opponent_modeling, helper_training.py:1117-1137): actions [B,N,2] (device) are the policy's tentative
 * actions; column pair k of the placeholder tail of agent i's row in SIGMAENV_BUF_OBS receives the action of its k-th observed neighbour
 * (nearing_agents_indices[b, i, k], SIGMAENV_BUF_NEARING).  Needs SIGMAENV_OBS_OPPONENT_PAD; the caller runs its policy before and after, as the
 * reference does. */
int sigmaenv_opponent_fill(sigmaenv_t* h, const float* actions);

/* Rollout slab (wire format of the learner-boundary exchange): when dev_ptr != NULL every following sigmaenv_step also writes
 * one contiguous fp32 row per env, [N*D observation | N reward | 1 done], to dev_ptr ([B, N*(D+1)+1]).  The caller rotates the
 * pointer through its rollout buffer; NULL disables the record.  Replaces the per-step tensordict stacking of
 * SyncDataCollectorCustom.rollout (sigmarl/helper_training.py:687-788) for (observation, reward, done). */
int sigmaenv_set_slab(sigmaenv_t* h, void* dev_ptr);
/* Stride (in floats) between the record blocks of consecutive steps of sigmaenv_rollout / sigmaenv_rollout_f32: step t records into
 * slab_base + t * stride.  0 (the default) = B * (N*(D+1)+1), i.e. a [T, B, W] buffer of this handle alone.  A batch that is split over several
 * handles (env shards on their own HIP streams: shard k owns envs [k Bs, (k+1) Bs) of the batch) records into ONE [T, B_total, W] buffer -- the layout
 * SyncDataCollectorCustom.rollout stacks (sigmarl/helper_training.py:687-788) -- by passing slab_base + k * Bs * W and the stride B_total * W, as
 * sigmaenv_step_autoreset_n does through its slab_stride argument.  Returns SIGMAENV_EINVAL for a stride below the handle's own block. */
int sigmaenv_set_rollout_slab_stride(sigmaenv_t* h, int64_t stride_floats);

/* Root-observation record of sigmaenv_rollout / sigmaenv_rollout_f32 / sigmaenv_rollout_f32_ex: base device f32, or NULL (the default) for none.  When set, step t
 * copies SIGMAENV_BUF_OBS ([B, N*D]) to base + t * stride_floats AFTER the policy and BEFORE the step, on the handle's stream: exactly the rows the step's final
 * actor forward read (opponent modelling: with the filled placeholder columns; prioritized propagation: the observation at the start of the step).  This is the
 * "observation" entry of the tensordict SyncDataCollectorCustom.rollout stacks (sigmarl/helper_training.py:687-788) -- the record row of step t - 1 holds it only
 * for envs in which nothing was re-placed at step t - 1.  stride_floats 0 = B * N * D; a stride below that is SIGMAENV_EINVAL; env shards record into ONE
 * [T, B_total, N*D] buffer with base + k * Bs * N * D and the stride B_total * N * D, as sigmaenv_set_rollout_slab_stride does for the slab.  Nothing else of a
 * rollout changes with the record on. */
int sigmaenv_set_rollout_obs_record(sigmaenv_t* h, float* base, int64_t stride_floats);

/* Blocks until everything enqueued on the handle's stream has finished. */
int sigmaenv_sync(sigmaenv_t* h);

/* Average device time (ms) of the last `sigmaenv_step` launches measured with HIP events on the handle's stream
 * since the previous call; n_launches receives the count.  Profiling aid for bench.py. */
int sigmaenv_step_time_ms(sigmaenv_t* h, double* avg_ms, int32_t* n_launches);
/* The same for the other kernels a rollout step can be made of (bench.py names the one with the largest share of GPU time in its roofline):
 * the first call of either function arms the bracketing for all of them. */
#define SIGMAENV_KERNEL_STEP 0        /* sigmaenv_step_wave_kernel (sigmaenv_step / _autoreset / _autoreset_n) */
#define SIGMAENV_KERNEL_CBF_QP 1      /* cbf::sigmaenv_cbf_qp_kernel (sigmaenv_cbf_qp) */
#define SIGMAENV_KERNEL_CBF_MARGIN 2  /* cbf::sigmaenv_cbf_kernel (sigmaenv_cbf_rewards) */
#define SIGMAENV_KERNEL_MLP32 3       /* sigmaenv_mlp32_kernel (sigmaenv_mlp32_forward / sigmaenv_actor_forward_f32) */
#define SIGMAENV_KERNEL_ACTOR_BF16 4  /* sigmaenv_actor_kernel (sigmaenv_actor_forward) */
#define SIGMAENV_KERNEL_COUNT 5
int sigmaenv_kernel_time_ms(sigmaenv_t* h, int32_t kernel_id, double* avg_ms, int32_t* n_launches);

/* What the handle launches (read-only; decided once in sigmaenv_create from the configuration, the device and the diagnostic switches of README.md): the step
 * kernel's tiling -- wave_G envs per wavefront tile, wave_wpb tiles per workgroup, wave_grid workgroups, wave_spec = agents * 256 + envs of a fixed-shape
 * instantiation or 0, wave_lds_bytes of LDS per workgroup -- and the template arguments of the sigmaenv_step_wave_kernel instantiation that sigmaenv_step* launch
 * (kern_*: the very selection the launch uses); whether the map took the shared-reciprocal division and the pruned boundary scan; the tiling of the stand-alone
 * observe / reset kernels (G envs per workgroup of `block` threads, `grid` workgroups, reset_block threads per reset workgroup, smem_bytes of LDS).
 * Lets a test assert the tile shape it means to exercise instead of assuming it. */
typedef struct sigmaenv_launch_shape {
  int32_t wave_G, wave_wpb, wave_grid, wave_spec, wave_lds_bytes;
  int32_t kern_fastdiv, kern_par, kern_sn, kern_sg, kern_var, kern_mtvs; /* <FASTDIV, PAR, SN, SG, VAR, MTVS> */
  int32_t map_fast_div, pruned_scan;
  int32_t G, block, grid, reset_block, smem_bytes;
  int32_t reserved[2];
} sigmaenv_launch_shape_t;
int sigmaenv_launch_shape(const sigmaenv_t* h, sigmaenv_launch_shape_t* out);

/* The pruned scan's create-time neighbour table of ONE polyline, on the host (no device, no handle): from its nch <= 64 chunk boxes (boxes[c] = min x, min y,
 * max x, max y; min > max: a chunk without segments) and the vehicle's length and width, what sigmaenv_create uploads -- rows[c]: 32 bytes = a list of 28 chunk
 * indices, one byte each, without c itself: the chunks within the tight radius of chunk c, then those only within the near radius, then those only within the far
 * radius, each ring ascending; then three counts, the lengths of the tight / near / far prefix of the list, and a pad byte 0.  The bytes past the list's end repeat
 * its last entry.  A count of 255 marks a level with more than 28 neighbours, as every wider level then is (the list stops with the widest level that fits; for a
 * marked level the kernel takes the search over the group boxes) -- and, if masks is not NULL, masks[c][3]: the same three neighbourhoods as bit sets, c's own bit
 * included.  Lets a host test hold the lists to the masks. */
int sigmaenv_neigh_rows(const float* boxes, int32_t nch, float length, float width, uint8_t* rows, uint64_t* masks);

/* The device side of the arithmetic contract's trigonometry (include/sigma_trig_f32.h; torch.sin / cos / tan / atan as called by
 * sigmarl/dynamics.py:103-111,161-168 and helper_scenario.py:795-810), evaluated on arrays: kind 0 sin, 1 cos, 2 tan, 3 atan of
 * in[0..n) -> out[0..n) (device pointers, f32).  Lets the GPU test-suite hold the device functions to the same bits as the host's. */
int sigmaenv_trig_selftest(sigmaenv_t* h, int32_t kind, int32_t n, const float* in, float* out);

/* ---- policy in the loop ------------------------------------------------------------------------------
 * The actor of sigmarl/modules/decision_making_module.py:34-82 (torchrl MultiAgentMLP: Linear(D,256) Tanh Linear(256,256) Tanh
 * Linear(256,256) Tanh Linear(256,4), shared by all agents; NormalParamExtractor "biased_softplus_1.0"; TanhNormal between low and high)
 * as one MFMA kernel (bf16 weights / activations, fp32 accumulate), so that a rollout of T steps runs without the host in the loop. */
typedef struct sigmaenv_actor sigmaenv_actor_t;

/* w_l / b_l: HOST pointers, torch.nn.Linear layout (w_l row-major [out, in], fp32); low / high: action bounds, 2 floats each
 * (VMAS: -/+ u_range = max_speed, max_steering, helper_common.py:382-430).  obs_dim must be 8, 16, 24 or 32 (whole MFMA k-blocks; the
 * reference's default observation is 32 = sigmaenv_obs_dim(2)); other widths: SIGMAENV_EINVAL -- use sigmaenv_mlp32_* (any width). */
int sigmaenv_actor_create(int32_t obs_dim, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                          const float* w4, const float* b4, const float* low, const float* high, sigmaenv_actor_t** out);
void sigmaenv_actor_destroy(sigmaenv_actor_t* a);

/* actions := policy(observation) for every agent row.  obs: device f32 [B*N, obs_dim] or NULL for the handle's SIGMAENV_BUF_OBS;
 * actions: device f32 [B,N,2]; log_prob (optional) device f32 [B,N]; loc_scale (optional) device f32 [B,N,4] = loc0, loc1, scale0,
 * scale1.  deterministic != 0: action = squash(loc).  seed / counter select the counter-based random stream (draws DRAW_ACTOR, + 1 of the draw table,
 * sigmarl_amd/csrc/sigmaenv_dist.h, which states every stream of the generator and the head's arithmetic once).
 * Everywhere in this header the generator takes `seed` with both 32-bit words and `counter` with its LOW 32 bits only: counter and counter + 2^32
 * give the same draws (2^32 + 5 draws what 5 draws), so a stream repeats after 2^32 steps of one seed (tests/policy_head_check.py restates it). */
int sigmaenv_actor_forward(sigmaenv_t* h, sigmaenv_actor_t* a, const float* obs, float* actions, float* log_prob, float* loc_scale, uint64_t seed,
                           uint64_t counter, int32_t deterministic);

/* ---- the reference's networks in the reference's precision ------------------------------------------------------------------------
 * fp32 shared-parameter MLP on the matrix cores (two arithmetic modes, below), Tanh between the layers, hidden width 256:
 *   actor   sigmarl/modules/decision_making_module.py:34-52   dims = {obs_dim, 256, 256, 256, 4}, one row per agent
 *   critic  sigmarl/modules/optimization_module.py:16-32      dims = {n_agents * obs_dim, 256, 256, 256, 1}, one row per env (MAPPO, centralised:
 *           the observations of all agents of the env concatenated -- exactly a row of SIGMAENV_BUF_OBS viewed as [B, N * D]; the one output
 *           is the state value of every agent of the env)
 * weights[l]: torch.nn.Linear layout [dims[l+1], dims[l]] row-major fp32 (host pointers), biases[l]: [dims[l+1]].  2 to 4 layers; dims[0] (the input width)
 * 1 .. 4096, every hidden width 256, dims[n_layers] 1 .. 32; anything else: SIGMAENV_EINVAL.
 * forward: in / out device f32 [rows, dims[0]] / [rows, dims[n_layers]]; `in` must be 16-byte aligned (the rows are read with 16-byte loads).
 * sigmaenv_actor_forward_f32 = this MLP + the distribution head of sigmaenv_actor_forward (same outputs); scratch: device f32 [B * N * 4]. */
typedef struct sigmaenv_mlp32 sigmaenv_mlp32_t;
/* How the products of these fp32 networks are formed.  Both modes accumulate in fp32 and are held to torch.nn (fp32, CPU) within 1e-5 by the test-suite.
 *   EXACT  v_mfma_f32_32x32x2_f32: an fp32 fma chain, one rounding per product -- the fp32 VECTOR rate (157 TF), 1/16 of the half-precision matrix rate
 *   SPLIT  (default) every fp32 operand as hi + lo, two fp16 numbers (22 significant bits, scaled so that lo is a normal number); w x = w_hi x_hi + w_hi x_lo
 *          + w_lo x_hi on v_mfma_f32_32x32x16_f16 with exact products: 3/16 of the matrix time.  Measured against fp64 on K = 256 dot products: 3.6e-7 against
 *          6.4e-7 for the exact chain (tools/mfma_probe/probe_f16_split.hip).  Ranges: |weight| < 255 (else the handle stays EXACT and set_mode(SPLIT)
 *          returns SIGMAENV_EINVAL), |input| < 4094 (an input outside is saturated to +-4094: finite but wrong
 *          outputs), dims[0] <= 592 (a wider network stays EXACT, as above). */
#define SIGMAENV_MLP32_EXACT 0
#define SIGMAENV_MLP32_SPLIT 1
int sigmaenv_mlp32_set_mode(sigmaenv_mlp32_t* m, int32_t mode);
int sigmaenv_mlp32_get_mode(const sigmaenv_mlp32_t* m);
int sigmaenv_mlp32_create(int32_t n_layers, const int32_t* dims, const float* const* weights, const float* const* biases, sigmaenv_mlp32_t** out);
void sigmaenv_mlp32_destroy(sigmaenv_mlp32_t* m);
int sigmaenv_mlp32_forward(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows, float* out);
int sigmaenv_actor_forward_f32(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* obs, float* scratch, const float* low, const float* high, float* actions,
                               float* log_prob, float* loc_scale, uint64_t seed, uint64_t counter, int32_t deterministic);

/* sigmaenv_mlp32_forward on rows that are NOT dense: network row r = t * rows_per_block + b (t < n_blocks, b < rows_per_block) is read from
 * in + t * block_stride + b * row_stride (dims[0] floats; strides in floats, row_stride >= dims[0]); out is dense [n_blocks * rows_per_block, dims[n_layers]].
 * `in` and the rows need 4-byte alignment only.  This is how the critic reads a rollout's records without a staging copy: the observation part of the rows of a
 * [T, B_total, W] slab (row_stride = W = N*(D+1)+1, odd; block_stride = B_total * W) or a root-observation record (sigmaenv_set_rollout_obs_record) -- the
 * `value_network(tensordict)` passes of torchrl's GAE inside _compute_gae (sigmarl/mappo_cavs.py:357-386).  Both arithmetic modes; only the staging of the input
 * tile differs from sigmaenv_mlp32_forward (16-byte loads when base and strides are multiples of 4 floats, realigned 16-byte loads otherwise), so a row's
 * result is bit for bit what sigmaenv_mlp32_forward gives the same row copied to a dense aligned buffer. */
int sigmaenv_mlp32_forward_rows(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                float* out);

/* ---- weights refreshed on the device (sigmaenv_load.inc) ------------------------------------------------------------------------------
 * The learner's new parameters go into an EXISTING network handle without visiting the host: weights_dev / biases_dev are HOST arrays of DEVICE pointers, one per
 * layer (sigmaenv_mlp32: the handle's n_layers; sigmaenv_actor: 4), tensors in torch.nn.Linear layout ([dims[l+1], dims[l]] row-major fp32, [dims[l+1]]) with the
 * dimensions the handle was created with; 4-byte alignment suffices.  `h` supplies the device, the stream and sigmaenv_last_error.  The pack kernels (one launch
 * per layer, one lane per destination slot) are enqueued on h's stream and rewrite the handle's buffers IN PLACE -- every slot, padding included; no allocation,
 * no free, no host copy of a weight -- so launches enqueued on that stream before the call read the old weights, launches enqueued after it the new ones; work on
 * OTHER streams that uses the handle must be ordered against the call by the caller.  The packed words are those sigmaenv_mlp32_create / sigmaenv_actor_create
 * make from the same numbers (the host packers' integer roundings restated on the device): a loaded handle computes bit for bit what a fresh one does.
 * sigmaenv_mlp32_load_device rewrites BOTH forms (exact and split; a network that is exact-only by its input width, dims[0] > 592, only the exact one) and reduces
 * the split form's range predicate (!(|w| < 255): a NaN is outside) into one device word, copies those 4 bytes back on h's stream and waits for them -- the call's
 * only host wait -- and then sets the mode in force: the mode last accepted by sigmaenv_mlp32_set_mode (SPLIT by default) when the weights allow it, else EXACT.
 * A SPLIT network loaded with an out-of-range weight therefore runs EXACT and returns to SPLIT with the next in-range load; sigmaenv_mlp32_get_mode reports the
 * mode in force; sigmaenv_mlp32_set_mode(SPLIT) is refused as before (SIGMAENV_EINVAL) while the weights are outside the range, but remembered for the next load.
 * sigmaenv_actor_load_device rewrites the bf16 weights and the biases; low / high stay.  It does not wait.
 * A null handle, pointer array or tensor, or a tensor that is not 4-byte aligned: SIGMAENV_EINVAL with sigmaenv_last_error set, before any launch. */
int sigmaenv_mlp32_load_device(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* const* weights_dev, const float* const* biases_dev);
int sigmaenv_actor_load_device(sigmaenv_t* h, sigmaenv_actor_t* a, const float* const* weights_dev, const float* const* biases_dev);

/* ---- the fp32 network differentiated (sigmaenv_grad.inc) -------------------------------------------------------------------------------
 * Layers l = 0 .. n - 1 of the handle, z_l = W_l a_l + b_l, a_{l+1} = tanh(z_l) for l < n - 1, a_0 = the input rows.  The rows are addressed as in
 * sigmaenv_mlp32_forward_rows (row r = t * rows_per_block + b at in + t * block_stride + b * row_stride floats, 4-byte alignment suffices; a dense [rows, dims[0]]
 * input is rows_per_block = rows, row_stride = dims[0], n_blocks = 1), so a minibatch of whole time slices of a rollout record is read where it lies.  The weights
 * are the handle's own (what sigmaenv_mlp32_create / sigmaenv_mlp32_load_device put there): forward and gradient cannot disagree about them.  Everything is
 * enqueued on h's stream; nothing waits.
 *   sigmaenv_mlp32_forward_save   out [rows, dims[n]] := the network, bit for bit what sigmaenv_mlp32_forward_rows writes with the handle in EXACT mode -- the
 *       EXACT chain runs whatever mode is in force --, and acts [n - 1][rows][256] := every hidden layer's tanh output as the next layer consumed it
 *       (device f32, 16-byte aligned).
 *   sigmaenv_mlp32_backward_workspace   *n_floats := the floats of `workspace` for `rows` rows (0 for rows = 0).
 *   sigmaenv_mlp32_backward   with g_{n-1} = dout [rows, dims[n]] (device f32):
 *           g_{l-1} = (g_l W_l) (.) (1 - a_l^2)  for l = n - 1 .. 1;     grad_w[l] := g_l^T a_l  ([dims[l+1], dims[l]], torch.nn.Linear layout);     grad_b[l] := sum_rows g_l
 *       grad_w / grad_b: HOST arrays of DEVICE pointers, one per layer, as sigmaenv_mlp32_load_device takes the weights; OVERWRITTEN, not accumulated.  `in` and the
 *       four row arguments, and `acts`, are those of the sigmaenv_mlp32_forward_save call; workspace: device f32, 16-byte aligned; after the call its first
 *       (n - 1) * rows * 256 floats hold g_l, l = 0 .. n - 2, as [n - 1][rows][256] (the rest: the ranges' partial sums).  The gradient with respect to the input is
 *       not computed here (sigmaenv_mlp32_backward_dx, below, computes it).
 * Arithmetic and summation order.  fp32 throughout; every sum is an fma chain (v_mfma_f32_32x32x2_f32: one rounding per term) or a chain of fp32 additions:
 *   g_{l-1}[r, k]  the chain over the features f = 0, 1, .. of g_l[r, f] W_l[f, k] from 0, times fl(1 - a^2) formed with ONE rounding (fma(-a, a, 1)), rounded once more;
 *   grad_w[l][f, k]  the rows are cut into ranges of len = max(256, ceil(rows / 64) rounded up to a multiple of 64) rows: range i = [i len, min(rows, (i + 1) len));
 *       per range the chain over its rows in order from 0, then the ranges' partial sums added in range order;
 *   grad_b[l][f]  per range the chain of additions over its even rows (by offset in the range) and the one over its odd rows, added, then the ranges in order.
 * The partition depends on `rows` alone -- not on the device, the environment or the order in which workgroups arrive -- and no atomics are used: the same inputs give
 * the same bits on every run.  Rows past the end of a tile or a range and padded columns contribute exact zeros.  rows = 0: the gradients are written as zeros and
 * no row is read (in / acts / dout / workspace may be NULL).
 * A null handle, gradient array or tensor, a misaligned pointer, a row_stride below dims[0], negative counts: SIGMAENV_EINVAL with sigmaenv_last_error set, before
 * any launch. */
int sigmaenv_mlp32_forward_save(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                float* out, float* acts);
int sigmaenv_mlp32_backward_workspace(const sigmaenv_mlp32_t* m, int64_t rows, uint64_t* n_floats);
int sigmaenv_mlp32_backward(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                            const float* acts, const float* dout, float* workspace, float* const* grad_w, float* const* grad_b);
/* The same two on a MINIBATCH OF BLOCKS picked by index (a minibatch of frames, sigmarl/mappo_cavs.py:321-340: SamplerWithoutReplacement, or the prioritized buffer,
 * which samples with replacement): index is a device i32 [n_index]; block t of the network's rows is block index[t] of the record, i.e. row r = t * rows_per_block + b
 * lies at in + index[t] * block_stride + b * row_stride.  n_blocks is the record's block count, the bound on the entries; rows = rows_per_block * n_index.  out, acts,
 * dout and the workspace stay dense, in minibatch order; sigmaenv_mlp32_backward_workspace(rows) sizes the workspace.  For the actor a frame is a block of N rows
 * of width D (block_stride = N D), for the critic one row of width N D.  Duplicates in index are legal.  An entry outside [0, n_blocks) is never used as an address:
 * its rows are staged as zeros, exactly like rows beyond the last one (a caller that wants an error checks the range itself, as the Python layer does).
 * Same arithmetic, same summation order and partition as above -- functions of rows and the layer shapes alone, no atomics --, so the results are bit for bit those
 * of the non-indexed call on the same rows gathered dense, and with index = 0, 1, .. those of the non-indexed call on the record.  block_stride >= 0 is required;
 * n_index = 0 is the rows = 0 case.  The index entry is loaded once per row, not per element (forward: by the first 64 lanes of the tile into LDS; dW_0: one load
 * per lane and row). */
int sigmaenv_mlp32_forward_save_indexed(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                        int64_t block_stride, const int32_t* index, int32_t n_index, float* out, float* acts);
int sigmaenv_mlp32_backward_indexed(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                    int64_t block_stride, const int32_t* index, int32_t n_index, const float* acts, const float* dout, float* workspace,
                                    float* const* grad_w, float* const* grad_b);

/* The three calls that read input rows, on PADDED rows: the network's input row is in_dim / seg_dst segments of width seg_dst, the row in memory the same number of
 * segments of width seg_src <= seg_dst; network column a * seg_dst + j is the row's float a * seg_src + j for j < seg_src and 0 for j >= seg_src.  The base critic's
 * next rows under prioritized action propagation: per agent the obs_dim floats of the record's next observation, then 2 n_nearing zeros (the reference's
 * ("next", base_observation) is the env's own output with the placeholder columns zero) -- staged without a padded copy in memory.  row_stride >= the width of the
 * row in memory; otherwise the arguments, the refusals and the orders of the calls without _pad, and bit for bit their results on the rows gathered and padded
 * dense.  seg_src < 1, seg_dst < seg_src or seg_dst not a divisor of in_dim: SIGMAENV_EINVAL. */
int sigmaenv_mlp32_forward_rows_pad(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                    int32_t seg_src, int32_t seg_dst, float* out);
int sigmaenv_mlp32_forward_save_indexed_pad(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                            int64_t block_stride, const int32_t* index, int32_t n_index, int32_t seg_src, int32_t seg_dst, float* out, float* acts);
int sigmaenv_mlp32_backward_indexed_pad(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                        int64_t block_stride, const int32_t* index, int32_t n_index, int32_t seg_src, int32_t seg_dst, const float* acts,
                                        const float* dout, float* workspace, float* const* grad_w, float* const* grad_b);

/* The gradient with respect to the INPUT rows: dx [rows, dims[0]] := g_0 W_0, dx[r, k] the chain over the features f = 0, 1, .., 255 of g_0[r, f] W_0[f, k] from 0
 * (v_mfma_f32_32x32x2_f32: one rounding per term; no factor), g_0 the delta of the first layer as above.  It needs layer 0's weights in the transposed exact form,
 * which a handle holds only when it was asked to:
 *   sigmaenv_mlp32_create_input_grad   sigmaenv_mlp32_create (same arguments, refusals and results) whose handle ALSO holds that form -- dims[0] padded to 32 times 256
 *       floats -- and keeps it current wherever its weights are rewritten (sigmaenv_mlp32_load_device, sigmaenv_optim_step's repack: the same per-slot statement).
 *       Every other entry point treats the two kinds of handle alike; a handle from sigmaenv_mlp32_create allocates, packs and runs what it always did.
 *   sigmaenv_mlp32_input_grad_workspace   *n_floats := (n - 1) * rows * 256, the floats of sigmaenv_mlp32_input_grad's workspace (0 for rows = 0).
 *   sigmaenv_mlp32_input_grad   from acts [n - 1][rows][256] (sigmaenv_mlp32_forward_save's) and dout [rows, dims[n]]: ONE launch -- the delta kernel's instantiation that
 *       ends with the contraction above --; no input row is read and no dW kernel runs.  workspace: device f32, 16-byte aligned; afterwards it holds g_l,
 *       l = 0 .. n - 2, as [n - 1][rows][256].  dx: device f32, dense, 4-byte alignment suffices (rows of an odd width are stored column by column, 16-byte
 *       stores only when dims[0] is a multiple of 4 and dx is 16-byte aligned); OVERWRITTEN; columns >= dims[0] and rows >= rows are never written.
 *   sigmaenv_mlp32_backward_dx   the arguments of sigmaenv_mlp32_backward_indexed_pad, then dx.  index = NULL with n_index = 0 means the record's own blocks
 *       (sigmaenv_mlp32_backward -- NOT the empty minibatch of the _indexed entry points), seg_src = seg_dst = 0 means no padding; padded rows need an index, as
 *       there.  That one delta launch, then the dW and sum kernels of the entry points above: grad_w / grad_b are bit for bit theirs on the same arguments, dx is
 *       bit for bit sigmaenv_mlp32_input_grad's.  The workspace is sigmaenv_mlp32_backward_workspace's.  With padding dx still has dims[0] columns (the network's
 *       input row, padding columns included).
 * No atomics; a function of acts, dout and the weights alone: the same bits every run, whatever the layout the input rows were read from.  rows = 0: nothing is
 * launched for dx, SIGMAENV_OK (backward_dx still writes the gradients as zeros).  A handle without the form: SIGMAENV_EINVAL with sigmaenv_last_error set, as for a
 * null or misaligned pointer, before any launch. */
int sigmaenv_mlp32_create_input_grad(int32_t n_layers, const int32_t* dims, const float* const* weights, const float* const* biases, sigmaenv_mlp32_t** out);
int sigmaenv_mlp32_input_grad_workspace(const sigmaenv_mlp32_t* m, int64_t rows, uint64_t* n_floats);
int sigmaenv_mlp32_input_grad(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* acts, const float* dout, int32_t rows, float* workspace, float* dx);
int sigmaenv_mlp32_backward_dx(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                               const int32_t* index, int32_t n_index, int32_t seg_src, int32_t seg_dst, const float* acts, const float* dout, float* workspace,
                               float* const* grad_w, float* const* grad_b, float* dx);

/* n_steps x (sigmaenv_actor_forward; sigmaenv_step_autoreset) enqueued back to back (SyncDataCollectorCustom.rollout,
 * sigmarl/helper_training.py:687-788, without its per-step Python): actions_buf device f32 [B,N,2] scratch; optional records:
 * slab_base device f32 [n_steps, B, N*(D+1)+1], logp_base device f32 [n_steps, B, N], actions_rec device f32 [n_steps, B, N, 2].
 * Step t uses the random-stream counter counter0 + t for both the policy sample and the resets.  When the handle has SIGMAENV_REW_CBF
 * (or SIGMAENV_REW_CBF_QP) set and sigmaenv_cbf_attach has been called, sigmaenv_cbf_rewards (sigmaenv_cbf_qp) runs on the sampled actions
 * between the two (the order of cbf_constrained_centralized_policy, sigmarl/helper_training.py:1604-1635); with is_apply_cbf_action the
 * env steps with the QP's safe actions. */
int sigmaenv_rollout(sigmaenv_t* h, sigmaenv_actor_t* a, int32_t n_steps, float* actions_buf, float* slab_base, float* logp_base, float* actions_rec,
                     uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count, int32_t deterministic);
/* The same with the actor in the REFERENCE's precision (an fp32 torch MLP, decision_making_module.py:34-82): sigmaenv_actor_forward_f32 in front of
 * every step instead of the bf16 kernel; `m` from sigmaenv_mlp32_create (obs_dim -> 256 -> 256 -> 256 -> 4), low / high HOST pointers (2 floats each),
 * scratch device f32 [B * N * 4].  Step t == sigmaenv_actor_forward_f32(.., seed, counter0 + t, ..) then sigmaenv_step_autoreset(.., seed, counter0 + t, ..)
 * bit for bit.  The policy reads SIGMAENV_BUF_OBS, i.e. the observation incl. the sensor noise when sigmaenv_config_t.obs_noise_level > 0.
 * This runs the PLAIN policy (or the CBF-constrained one, above) only: opponent modelling and prioritized action propagation are sigmaenv_rollout_f32_ex. */
int sigmaenv_rollout_f32(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* low, const float* high, float* scratch, int32_t n_steps, float* actions_buf,
                         float* slab_base, float* logp_base, float* actions_rec, uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count,
                         int32_t deterministic);

/* ---- policy wrappers of the training collector in the device rollout ----------------------------------------------------------------
 * SyncDataCollectorCustom.rollout (sigmarl/helper_training.py:708-740) runs one of four policies per step: the CBF-constrained one (sigmaenv_rollout_f32 after
 * sigmaenv_cbf_attach), opponent modelling, prioritized action propagation, or the plain policy (sigmaenv_rollout_f32).  sigmaenv_rollout_f32_ex adds the two
 * middle ones; with opts == NULL or wrapper == SIGMAENV_WRAP_PLAIN it IS sigmaenv_rollout_f32 (same bits).  The collector's chain is if / elif: a wrapper on a
 * handle with a "cbf" rew_method (SIGMAENV_REW_CBF / SIGMAENV_REW_CBF_QP) is SIGMAENV_EINVAL.
 *
 * SIGMAENV_WRAP_OPPONENT (opponent_modeling, helper_training.py:1071-1142; needs SIGMAENV_OBS_OPPONENT_PAD, `m` takes the handle's obs_dim).  Step t:
 *   tentative forward  sigmaenv_actor_forward_f32 on SIGMAENV_BUF_OBS with seed ^ (1 << 63) (the TENTATIVE key), counter counter0 + t, log-probabilities dropped;
 *   sigmaenv_opponent_fill on its actions;  final forward with (seed, counter0 + t) -- the key of the plain rollout's step t -- into the step's actions /
 *   log-probabilities;  the step.  The reference samples the policy twice on the filled observation (:1139, then the collector at :730) and keeps the second
 *   draw; one draw from the same distribution is made here.  tentative_rec (optional, device f32 [n_steps, B, N, K, 2]): the neighbour actions written into the
 *   placeholder columns at step t (the step rewrites the observation: this is how a trainer recovers the filled observation the reference stores).
 *
 * SIGMAENV_WRAP_PRIORITIZED (prioritized_ap_policy, helper_training.py:1162-1315; `m` takes obs_dim + 2 K inputs: the base observation, SIGMAENV_BUF_OBS padded
 * with 2 K columns as info()["base_observation"] is -- also when the handle has SIGMAENV_OBS_OPPONENT_PAD).  Step t:
 *   1. ranks [B, N] (agent indices, highest priority first) from priority_source:
 *      SIGMAENV_PRIORITY_NET     sigmaenv_priority_forward of priority_net on SIGMAENV_BUF_OBS (the priority observation) with (seed, counter0 + t);
 *      SIGMAENV_PRIORITY_RANDOM  sigmaenv_priority_random with (seed, counter0 + t) (prioritization_method "random");
 *      SIGMAENV_PRIORITY_GIVEN   ranks_given, device i32 [B, N], the same every step (entries outside [0, N) act for nobody).
 *   2. the step's actions are zeroed (combined_action), then N turns: turn k gathers, for every env b, the base observation of agent i = ranks[b, k] with the
 *      current actions of its K observed neighbours (SIGMAENV_BUF_NEARING) in the 2 K padded columns -- zeros for neighbours that have not acted yet -- into a
 *      compact [B, obs_dim + 2 K] buffer, and runs the actor on those B rows only; the head writes agent (b, i)'s action / log-probability and draws with that
 *      row's key, so that the sample is bit for bit what sigmaenv_actor_forward_f32 on all B * N rows with (seed, counter0 + t) gives that row.
 *   3. the step on the combined actions.  The collector calls the policy once more on the turn observations (:743): a re-draw from the same distributions;
 *      the turn draws are kept here.
 *   Records (optional): rank_rec i32 [n_steps, B, N]; score_rec / score_logp_rec f32 [n_steps, B, N] (SIGMAENV_PRIORITY_NET); tentative_rec as above = the
 *   neighbour actions each agent saw at its turn; base_obs_rec f32 [n_steps, B, N, obs_dim + 2 K] = the compact row every agent was evaluated on in its
 *   turn (its SIGMAENV_BUF_OBS row, then the 2 K neighbour-action columns: info()["base_observation"], helper_training.py:1305-1312), written by the turn's gather;
 *   every agent has one turn per step, so every row is written exactly once per step -- unless ranks_given names no agent for it, which leaves the row as it
 *   was; a rank entry outside [0, N) is never an address.
 *   Communication noise (is_communication_noise, :1271-1287): comm_noise_std = (s_v, s_d) != 0, or comm_noise_std_env = a device f32 [B, 2] of per-env pairs,
 *   turns it on (all zero: off).  The agent acting in turn k then sees column q of its 2 K neighbour-action columns as fl32(v + fl32(std_q * z)), z a standard
 *   normal drawn per (env, acting agent, step, column) -- key (seed, counter0 + t, env_index_base + b, i), draws DRAW_COMM_NOISE + 2 q, + 2 q + 1, cosine branch
 *   (csrc/sigmaenv_dist.h) -- whether or not the action sample is deterministic.  The std goes by the column's POSITION as in the reference, which adds
 *   cat([s_v randn(2), s_d randn(2)]) to [a(n0).speed, a(n0).steer, a(n1).speed, a(n1).steer]: std = [s_v, s_v, s_d, s_d].  That 4-vector fits 2 K = 4 columns only,
 *   so n_nearing != 2 is SIGMAENV_EINVAL (raises in the reference as well).  Every column gets its draw, whatever it holds: the zero of a neighbour that has not
 *   acted, the column of a neighbour index that is no agent.  The noisy row is what the actor is evaluated on and what tentative_rec / base_obs_rec hold; the
 *   actions themselves stay clean (combined_action): the step and the later turns read clean values.  A pair of zeros in comm_noise_std_env gives values that
 *   compare equal to the noise-free rollout's.  Noise with another wrapper, a negative or non-finite comm_noise_std: SIGMAENV_EINVAL.
 *   sigmaenv_comm_noise_stds(level, stds4): the four per-column stds of `level` as the reference forms them -- the double products
 *   SIGMAENV_AGENT_MAX_SPEED * level and SIGMAENV_AGENT_MAX_STEERING * level rounded to fp32, by position; (stds4[0], stds4[2]) is comm_noise_std.  A library from
 *   before this entry point reads the two fields as reserved words and runs WITHOUT noise: a binding must refuse noise when the symbol is missing.
 * A first call per handle allocates a workspace (grown when a later call needs more): do not make that first call inside a stream capture. */
#define SIGMAENV_WRAP_PLAIN 0
#define SIGMAENV_WRAP_OPPONENT 1
#define SIGMAENV_WRAP_PRIORITIZED 2
#define SIGMAENV_PRIORITY_NET 0
#define SIGMAENV_PRIORITY_RANDOM 1
#define SIGMAENV_PRIORITY_GIVEN 2
typedef struct sigmaenv_rollout_opts {
  int32_t wrapper;                   /* SIGMAENV_WRAP_* */
  int32_t priority_source;           /* SIGMAENV_PRIORITY_* (SIGMAENV_WRAP_PRIORITIZED) */
  sigmaenv_mlp32_t* priority_net;    /* SIGMAENV_PRIORITY_NET: obs_dim -> 256 -> 256 -> 2 */
  const int32_t* ranks_given;        /* SIGMAENV_PRIORITY_GIVEN: device i32 [B, N] */
  float* tentative_rec;              /* optional device f32 [n_steps, B, N, K, 2] */
  int32_t* rank_rec;                 /* optional device i32 [n_steps, B, N] */
  float* score_rec;                  /* optional device f32 [n_steps, B, N] */
  float* score_logp_rec;             /* optional device f32 [n_steps, B, N] */
  float comm_noise_std[2];           /* communication noise: (s_v, s_d), the stds of columns 0, 1 and of columns 2, 3; zero: none */
  const float* comm_noise_std_env;   /* optional device f32 [B, 2]: a pair per env, in place of comm_noise_std */
  float* base_obs_rec;               /* optional device f32 [n_steps, B, N, obs_dim + 2 K] (SIGMAENV_WRAP_PRIORITIZED) */
} sigmaenv_rollout_opts_t;
int sigmaenv_rollout_f32_ex(sigmaenv_t* h, sigmaenv_mlp32_t* m, const float* low, const float* high, float* scratch, int32_t n_steps, float* actions_buf,
                            float* slab_base, float* logp_base, float* actions_rec, uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count,
                            int32_t deterministic, const sigmaenv_rollout_opts_t* opts);
#define SIGMAENV_AGENT_MAX_SPEED 1.0                              /* AGENTS["max_speed"], sigmarl/constants.py:637-640 */
#define SIGMAENV_AGENT_MAX_STEERING (31 * 3.141592653589793 / 180) /* AGENTS["max_steering"] = 31 * math.pi / 180 */
int sigmaenv_comm_noise_stds(double level, float* stds4);

/* ---- from a rollout's records to a learner's batch -------------------------------------------------------------------------------------
 * sigmaenv_gae: what the trainer computes right after collector.rollout() -- _compute_gae (sigmarl/mappo_cavs.py:357-386: torchrl GAE(gamma, lmbda,
 * value_network = critic, average_gae = False), sigmarl/modules/optimization_module.py:62-67) and, optionally, compute_td_error (sigmarl/helper_training.py:
 * 1029-1068, the priorities of the prioritized replay buffer) -- on the records of n_steps rollout steps of this handle.  torchrl is third-party and absent: its
 * GAE is restated from published behaviour (done = terminated: the scenario has one flag; the critic's one value per env is every agent's).
 *   slab              device f32, the record rows [N*D observation | N reward | 1 done] of step t at slab + t * slab_stride (0: B * (N*(D+1)+1)); reward of agent i
 *                     and done are read IN PLACE at offsets N*D + i and N*(D+1) of the env's row
 *   state_value       device f32 [n_steps, B]: the critic on the root observations (sigmaenv_set_rollout_obs_record);  next_state_value: on the record rows
 *   advantage, value_target   device f32 [n_steps, B, N]
 * Arithmetic contract: fp32, one IEEE operation per operator, no contraction, c = fl32(fl32(gamma) * fl32(lmbda)); backwards over t with A_next = 0 beyond the
 * last step:
 *     nd = 1 - done[t,b];  d = (r[t,b,i] + (gamma * v_next[t,b]) * nd) - v[t,b];  A = d + ((c * nd) * A_next);  advantage = A;  value_target = A + v[t,b]
 * td_priority (optional, device f32 [n_steps, B]): x[t,b] = (sum over i = 0 .. N-1, in that order, of |(r + (td_gamma * v_next) * nd) - v|) / N, then with min / max
 * over THIS HANDLE's [n_steps, B] (an env shard normalises over its own envs): ((x - min) / max(max - min, 1e-3)) * 10 clamped to [1e-3, 10].  The result does not
 * depend on scheduling.  The first call with td_priority allocates two words: do not make it inside a stream capture.  Enqueued on the handle's stream. */
typedef struct sigmaenv_gae_args {
  int32_t n_steps;
  int32_t reserved0;               /* zero */
  const float* slab;
  int64_t slab_stride;             /* floats between the record blocks of consecutive steps; 0: B * (N*(D+1)+1) */
  const float* state_value;
  const float* next_state_value;
  float* advantage;
  float* value_target;
  float* td_priority;              /* optional */
  float gamma, lmbda, td_gamma;
  int32_t reserved[5];             /* zero */
} sigmaenv_gae_args_t;
int sigmaenv_gae(sigmaenv_t* h, const sigmaenv_gae_args_t* a);

/* ---- the episode return of a rollout's records (sigmaenv_episode.inc; the arithmetic: sigmaenv_episode.h) ----------------------------------
 * sigmaenv_episode_return: the RewardSum transform the reference wraps its env in (sigmarl/mappo_cavs.py:178-183: the agents' reward summed into
 * "episode_reward", reset by the env's done flag) and the number every iteration reports and gates its intermediate models on, episode_reward[done].mean()
 * (_log_and_save, :468-478; _save_intermediate_model, :498-515), on the records of n_steps rollout steps of this handle.  torchrl is third-party and absent:
 * RewardSum is restated from its published behaviour, as GAE is.
 *   slab, slab_stride   as in sigmaenv_gae_args_t: the reward of agent i and the done flag are read IN PLACE at offsets N*D + i and N*(D+1) of the env's row; a
 *                       record buffer wider than the handle is addressed by pointing slab at the handle's first env and passing the buffer's stride
 *   carry               device f32 [B, N], in and out: the running return of every agent's open episode on entry (zeros before the first rollout) and on exit
 *   episode_reward      optional device f32 [n_steps, B, N]: the record E
 *   result              device f32 [4]: mean, S, K, 0
 * Element contract: fp32, one IEEE addition per step, no reassociation, forwards over t -- E[t,b,i] = c + r[t,b,i] with c = carry[b,i] at t = 0; after step t
 * c = (done[t,b] != 0) ? 0 : E[t,b,i]; on exit carry[b,i] = the last c.  The frame that finishes an episode carries the whole episode's return, the next frame
 * starts from zero; a per-agent re-placement that does not set the env's done flag resets nothing (nor does it in the reference).  The recurrence is sequential in t
 * on purpose: the record equals the step-by-step fp32 sum bit for bit, which a parallel scan over t would not.
 * Reduction contract: K = the number of (t,b) with done set, result[2] = (float)K (exact: n_steps * B >= 2^24 is refused);  result[1] = S, the fp32 sum of E[t,b,i]
 * over the done frames and all i in the order of sigmaenv_episode.h -- within a frame the chain over i = 0 .. N-1 from 0; per env the chain over its done steps, t
 * ascending, from 0; over the envs one workgroup of 256 lanes: lane l the chain over b = l, l + 256, .. from 0, per wavefront the butterfly v += v[lane ^ m], m = 32,
 * 16, .., 1, then ((w0 + w1) + w2) + w3 (the longest chain: N + n_steps + ceil(B / 256) + 9 additions);  result[0] = S / (K * N) with K * N formed in fp32 and one
 * division, NaN when K = 0 (the reference's mean of an empty selection is NaN too);  result[3] = 0.  No atomics: a function of the inputs and (n_steps, B, N)
 * alone, whatever the scheduling or the launch shape.  Two launches on the handle's stream; nothing waits.  The first call allocates 2 B words: do not make it
 * inside a stream capture.
 * n_steps < 1, n_steps * B >= 2^24, a null slab, carry or result, a misaligned tensor, a stride below the handle's block: SIGMAENV_EINVAL with sigmaenv_last_error
 * set, before any launch. */
typedef struct sigmaenv_episode_args {
  int32_t n_steps;
  int32_t reserved0;               /* zero */
  const float* slab;
  int64_t slab_stride;             /* floats between the record blocks of consecutive steps; 0: B * (N*(D+1)+1) */
  float* carry;                    /* device f32 [B, N], in and out */
  float* episode_reward;           /* optional device f32 [n_steps, B, N] */
  float* result;                   /* device f32 [4] */
  int32_t reserved[6];             /* zero */
} sigmaenv_episode_args_t;
int sigmaenv_episode_return(sigmaenv_t* h, const sigmaenv_episode_args_t* a);

/* ---- the evaluation of a policy (sigmaenv_eval.inc; the arithmetic: sigmaenv_eval.h) ----------------------------------------------------------
 * What the reference reduces a testing rollout to (sigmarl/evaluation_base.py:184-217, _evaluate_model_i): four numbers per env -- the average speed
 * velocities.norm(dim=-1).mean(dim=(-2, -1)) (:205-207), the agent-agent collision rate is_collision_with_agents.squeeze(-1).any(dim=-1).sum(dim=-1) / num_steps
 * (:208-210), the agent-lanelet collision rate (:211-214) and the mean centre-line deviation distance_ref.squeeze(-1).mean(dim=(-2, -1)) (:215-217) -- accumulated
 * frame by frame from the per-step output buffers, on the device.  A rollout record row holds none of the inputs, and the fused step + auto-reset launch has
 * cleared the collision flags by the time a call returns: an evaluator is therefore either handed its frames (sigmaenv_eval_accumulate) or attached to the
 * handle's rollouts (sigmaenv_eval_attach), which then run every step as sigmaenv_step -> sigmaenv_eval_accumulate -> sigmaenv_auto_reset.
 *
 * A frame of env b: SIGMAENV_BUF_STATE[b,i,5:7] = (vx, vy) (info["vel"]); SIGMAENV_BUF_DIST_REF[b,i] (info["distance_ref"]); SIGMAENV_BUF_COL_AGENTS[b,i,j];
 * byte 0 of SIGMAENV_BUF_COL_FLAGS[b,i,.] (with_lanelets; bytes 1 .. 3 are never counted) -- as the buffers stand when the launch runs, no other source.
 * Element contract: n_i = sqrtf(vx * vx + vy * vy), two products, one addition, one correctly rounded square root, each fp32, no contraction;
 * aa = OR over i, j of col_agents[b,i,j]; al = OR over i of col_flags[b,i,0].
 * Reduction contract: the frame's sums of (double)n_i and of (double)dist_ref_i over the agents in fp64 in a butterfly over G = the smallest power of two >= N
 * lanes -- lane i holds agent i's term, lanes N .. G-1 hold +0.0, v += v[lane ^ m] for m = G/2, .., 1 --; per env sum_speed = sum_speed + frame_sum and sum_dref
 * likewise, ONE fp64 addition per frame in frame order; n_aa += aa, n_al += al, frames += 1 in uint32.  No atomics: a function of the inputs and (N, B, frames)
 * alone, whatever the scheduling or the launch shape.
 * sigmaenv_eval_finish: metrics f32 [B, 4], with F = frames:  [0] = (float)(sum_speed / (double)(F * N));  [1] = (float)n_aa / (float)F;  [2] = (float)n_al / (float)F;
 * [3] = (float)(sum_dref / (double)(F * N)).  F * N < 2^24 always holds (below), so both rates are one fp32 division of two exactly represented integers: bit for bit
 * the count / num_steps of :208-214.  F = 0: NaN in all four.  counts (optional) u32 [B, 3] = n_aa, n_al, frames.  The accumulators are left as they are.
 *
 * sigmaenv_eval_create: an evaluator of THIS handle (its B and N); args->trace_frames > 0 also allocates a device trace f32 [trace_frames, B, N, 8] with the rows
 *   x, y, vx, vy, dist_ref, n_i, col_agents-any-j (0/1), col_lanelet (0/1) -- the out_td entries :191-199 reads -- of the first trace_frames frames after a reset;
 *   later frames are accumulated but not traced.  args->debug_frames0 is a test hook and zero otherwise: the frame count every reset starts from (sums and counts
 *   start from zero all the same).  Allocates: do not call inside a stream capture.
 * sigmaenv_eval_reset: zero accumulators (and trace), enqueued on the handle's stream.  sigmaenv_eval_create ends with one.
 * sigmaenv_eval_accumulate: ONE launch, one frame for every env.  src NULL: the handle's buffers; otherwise each non-null pointer of src replaces the handle's buffer
 *   of that name, in the handle's own layout ([B,N,8] f32, [B,N] f32, [B,N,N] u8, [B,N,4] u8), 4-byte aligned.  Takes no position on WHICH moments are frames.
 * sigmaenv_eval_finish: ONE launch.  Nothing above waits on the host.
 * sigmaenv_eval_attach(h, ev) / (h, NULL): while an evaluator is attached, every step of sigmaenv_rollout, sigmaenv_rollout_f32 and sigmaenv_rollout_f32_ex (every
 *   wrapper, and the CBF chain: the step then takes the chain's own action, the QP's safe action where the chain uses one) runs as sigmaenv_step ->
 *   sigmaenv_eval_accumulate -> sigmaenv_auto_reset with the record row block, the (seed, counter0 + t) keys and the path range of the fused launch it replaces: end
 *   state, slab, log-probabilities, action record and observation record are the fused rollout's, bit for bit (sigmaenv_step_autoreset promises it).  The frame of
 *   step t is the step's outcome BEFORE the re-placements of testing mode (road_traffic.py:1435-1447) and reset_collisions clear it.  With nothing attached the
 *   rollouts are unchanged.  Direct calls of sigmaenv_step_autoreset, sigmaenv_step_autoreset_many and sigmaenv_step_autoreset_n are NOT affected by an attachment.
 * sigmaenv_eval_get: the one call that waits (it synchronises the handle's stream): copies an item to HOST memory, for inspection -- SIGMAENV_EVAL_SUM_SPEED /
 *   _SUM_DREF f64 [B]; _N_AA / _N_AL / _FRAMES u32 [B]; _TRACE f32 [trace_frames, B, N, 8]; _FRAMES_HOST one u64, the frames since the last reset as the host counts
 *   them (no wait).
 * sigmaenv_eval_destroy: waits for the handle's stream, detaches, frees.  An evaluator whose handle was destroyed first can only be destroyed.
 * Refused with SIGMAENV_EINVAL and sigmaenv_last_error set, before any launch: a null handle (no message), a null evaluator, an evaluator of another handle, an
 * override that is not 4-byte aligned, a frame with (frames + 1) * N >= 2^24 (an attached rollout: (frames + n_steps) * N, before its first launch). */
typedef struct sigmaenv_eval sigmaenv_eval_t;
typedef struct sigmaenv_eval_args {
  int32_t trace_frames;            /* 0: no trace */
  int32_t debug_frames0;           /* test hook, zero otherwise: the frame count a reset starts from */
  int32_t study;                   /* 1: a study evaluator (below); 0 (what a zeroed reserved word was): the four metrics alone */
  int32_t reserved[5];             /* zero */
} sigmaenv_eval_args_t;
typedef struct sigmaenv_eval_src {
  const float* state;              /* optional device f32 [B, N, 8] */
  const float* dist_ref;           /* optional device f32 [B, N] */
  const uint8_t* col_agents;       /* optional device u8 [B, N, N] */
  const uint8_t* col_flags;        /* optional device u8 [B, N, 4] */
  int32_t reserved[4];             /* zero */
} sigmaenv_eval_src_t;
#define SIGMAENV_EVAL_SUM_SPEED 0
#define SIGMAENV_EVAL_SUM_DREF 1
#define SIGMAENV_EVAL_N_AA 2
#define SIGMAENV_EVAL_N_AL 3
#define SIGMAENV_EVAL_FRAMES 4
#define SIGMAENV_EVAL_TRACE 5
#define SIGMAENV_EVAL_FRAMES_HOST 6
#define SIGMAENV_EVAL_STUDY_SUMS 7    /* f64 [7, B]: event, a^2, j^2, |dv|, |ds|, |av|, |as| */
#define SIGMAENV_EVAL_STUDY_N_ACT 8   /* u32 [B] */
#define SIGMAENV_EVAL_STUDY_CARRY 9   /* f32 [B, N, 2]: v_prev, a_prev */
#define SIGMAENV_EVAL_STUDY_TIMER0 10 /* i32 [B, 2]: the snapshot of num_task_tries, task_success_times */
int sigmaenv_eval_create(sigmaenv_t* h, const sigmaenv_eval_args_t* args, sigmaenv_eval_t** out);
void sigmaenv_eval_destroy(sigmaenv_eval_t* ev);
int sigmaenv_eval_reset(sigmaenv_t* h, sigmaenv_eval_t* ev);
int sigmaenv_eval_accumulate(sigmaenv_t* h, sigmaenv_eval_t* ev, const sigmaenv_eval_src_t* src);
int sigmaenv_eval_finish(sigmaenv_t* h, sigmaenv_eval_t* ev, float* metrics, uint32_t* counts);
int sigmaenv_eval_attach(sigmaenv_t* h, sigmaenv_eval_t* ev);
int sigmaenv_eval_get(sigmaenv_t* h, sigmaenv_eval_t* ev, int32_t what, void* host_out);

/* ---- the study of a CBF-filtered policy: six more metrics per env (sigmaenv_eval_args_t.study = 1; the arithmetic: sigmaenv_eval.h, second half) ------------
 * What sigmarl/evaluation_itsc26.py reduces a testing rollout to: compute_total_reward (:926-992), compute_cbf_activation_percentage (:995-1035) and the task
 * counters num_task_tries / task_success_times (:883-898, metric_task_success_rate :1450-1458).  The reference runs one env per process; here every env of the
 * batch is such a run.  An evaluator created with study = 0 is what it was: nothing below applies to it, and its kernel is unchanged.
 *
 * A study evaluator takes, with EVERY frame (sigmaenv_eval_accumulate, an attached rollout's step, sigmaenv_eval_accumulate_study), besides the four inputs above:
 * (av, as) = SIGMAENV_BUF_ACTION[b,i,:], the applied action; (nv, ns) = the nominal action: SIGMAENV_BUF_CBF_NOMINAL[b,i,:] when the handle's chain runs the
 * CBF-QP (SIGMAENV_REW_CBF_QP without SIGMAENV_REW_CBF, and sigmaenv_cbf_attach: the very condition under which a rollout step launches sigmaenv_cbf_qp; with both
 * flags set the chain runs the margin rewards and no QP), otherwise the applied action of the frame itself.  This is a fact of the HANDLE; a caller who reads the
 * nominal action from its own configuration instead (sigmarl_amd/scenario.py does, from its Parameters) can disagree with it, e.g. before sigmaenv_cbf_attach; rows 1 (rew_reach_goal), 7 (rew_collide_other_agents), 8 (rew_collide_lane) of SIGMAENV_BUF_REWARD_INFO; and a carry f32 [B,N,2] = (v_prev, a_prev).
 * Element contract, every operator one fp32 IEEE operation, no contraction:  e = (r1 + r7) + r8;  a = (av - v_prev) / fl32(0.1);  j = (a - a_prev) / fl32(0.1)  (0.1 is
 * the reference's constant, not Parameters.dt);  then v_prev = av, a_prev = a;  terms q q with q = |a| / 3.0f, q q with q = |j| / 20.0f, |av - nv|, |as - ns|, |av|, |as|;
 * activated = |av - nv| > fl32(1e-9) || |as - ns| > fl32(1e-9).  An INITIAL frame (study_src->initial = 1: the state after the reset) takes av = as = nv = ns = e = 0
 * whatever the buffers hold, a = j = 0, leaves the carry zero, and retakes the snapshot of the task counters from columns 1, 2 of the timer it is given.  A
 * re-placement of testing mode does not touch the carry.  Reduction contract: the seven sums over the agents in the butterfly above, ONE fp64 addition per frame
 * into seven accumulators; n_act += the activated agents of the frame (the popcount of the group's ballot), uint32.  No atomics.
 * sigmaenv_eval_study_finish: ONE launch.  metrics f32 [B,6], M = F N, m_x = (float)(sum_x / (double)M):  [1] event = (float)sum_e;  [2] comfort = (-0.2f m_a2) + (-0.2f m_j2);
 *   [0] total = event + comfort;  [3] degree = 100.0f (0.5f (m_dv / (m_av + 1e-9f) + m_ds / (m_as + 1e-9f)));  [4] rate = (float)((double)(100 n_act) / (double)M);
 *   [5] success rate = (float)(100.0 success / tries), NaN when tries <= 0, with tries / success = SIGMAENV_BUF_TIMER[b,1] / [b,2] AS THEY STAND WHEN THE LAUNCH RUNS
 *   minus the snapshot.  counts (optional) u32 [B,4] = n_act, tries, success, frames.  The accumulators are left as they are; sigmaenv_eval_finish still gives the four.
 * sigmaenv_eval_reset on a study evaluator also zeroes sums, count and carry and takes the snapshot from SIGMAENV_BUF_TIMER, on the stream (one more small launch).
 * sigmaenv_eval_accumulate_study: sigmaenv_eval_accumulate with study_src (NULL: no override, not initial): each non-null pointer replaces the handle's buffer of
 *   that name in its layout (applied, nominal f32 [B,N,2]; reward_info f32 [12,B,N], rows 1, 7, 8 read; timer i32 [B,4], read by an initial frame only), 4-byte
 *   aligned.  Without a nominal override and without the QP in the chain, the nominal action is the frame's applied action, an override included.
 * sigmaenv_eval_get: _STUDY_SUMS f64 [7,B] (event, a^2, j^2, |dv|, |ds|, |av|, |as|), _STUDY_N_ACT u32 [B], _STUDY_CARRY f32 [B,N,2], _STUDY_TIMER0 i32 [B,2].
 * Refused with SIGMAENV_EINVAL before any launch, besides the refusals above: the three study calls / items on an evaluator created without study; initial not 0 / 1. */
typedef struct sigmaenv_eval_study_src {
  const float* applied;            /* optional device f32 [B, N, 2] */
  const float* nominal;            /* optional device f32 [B, N, 2] */
  const float* reward_info;        /* optional device f32 [12, B, N] */
  const int32_t* timer;            /* optional device i32 [B, 4] */
  int32_t initial;                 /* 1: the frame after the reset */
  int32_t reserved[3];             /* zero */
} sigmaenv_eval_study_src_t;
int sigmaenv_eval_accumulate_study(sigmaenv_t* h, sigmaenv_eval_t* ev, const sigmaenv_eval_src_t* src, const sigmaenv_eval_study_src_t* study_src);
int sigmaenv_eval_study_finish(sigmaenv_t* h, sigmaenv_eval_t* ev, float* metrics, uint32_t* counts);

/* ---- the clip-PPO loss head of a minibatch update (sigmaenv_ppo.inc) ---------------------------------------------------------------------
 * sigmaenv_ppo_head: torchrl's ClipPPOLoss as sigmarl/modules/optimization_module.py:44-66 configures it (clip_epsilon, entropy_coeff = entropy_eps,
 * normalize_advantage = False, the default smooth-L1 critic loss, samples_mc_entropy = 1) for one minibatch of frames (sigmarl/mappo_cavs.py:389-407, _train_epoch /
 * _train_on_batch): from the networks' outputs of the minibatch and the learner's records, read through index, to the three loss terms and the gradients of their
 * sum with respect to those outputs -- the dout of sigmaenv_mlp32_backward_indexed.  torchrl is third-party and absent: the formulas below are the specification
 * (restated from its published behaviour, as actor_distribution is).  N = the handle's agents, M = n_index, F = n_frames; slot m, frame f = index[m], agent n,
 * action dimension d in {0, 1}, o = out[m, n, 0:4]:
 *   parameters     loc_d = o[d];  sigma_d = max(softplus(o[2 + d] + ln(e^0.99 - 1)) + 0.01, 1e-4);  h_d = (high_d - low_d) / 2      (actor_distribution's)
 *   log-probability of the recorded action a = action[f, n]   (the replay buffer has dropped the distribution's cache: the inverse transform)
 *                  y_d = clamp((a_d - low_d) / h_d - 1, +-(1 - 1e-6));   x_d = atanh(y_d) = 0.5 (log1p(y_d) - log1p(-y_d));
 *                  logp = sum_d [ -(x_d - loc_d)^2 / (2 sigma_d^2) - log sigma_d - log sqrt(2 pi) - 2 (log 2 - x_d - softplus(-2 x_d)) - log h_d ]
 *   objective      lw = logp - sample_log_prob[f, n];  A = advantage[f, n];  g1 = exp(lw) A;  g2 = exp(clamp(lw, log1p(-eps), log1p(eps))) A;
 *                  loss_objective = -mean_{m, n} min(g1, g2);  on a tie the unclamped branch carries the gradient
 *   entropy bonus  TanhNormal has no closed-form entropy: one reparameterised sample.  (z_0, z_1) by Box-Muller (z_0 the cosine branch) from the generator keyed
 *                  (seed, counter, env = f, agent = n), draws DRAW_ENTROPY, + 1 (the draw table of sigmaenv_dist.h);  x'_d = loc_d + sigma_d z_d;
 *                  logp' = sum_d [ -z_d^2 / 2 - log sigma_d - log sqrt(2 pi) - 2 (log 2 - x'_d - softplus(-2 x'_d)) - log h_d ]   (never clamped);
 *                  entropy = -mean logp';  loss_entropy = -entropy_coeff entropy;  the gradient flows through x' into loc and sigma
 *   critic         v = value[m] (the centralised critic's one value per frame is every agent's);  e = v - value_target[f, n];
 *                  smooth-L1, beta = 1: 0.5 e^2 if |e| < 1 else |e| - 0.5;  loss_critic = critic_coeff mean_{m, n}
 *   outputs        dout_actor[m, n, 0:4] = d(loss_objective + loss_entropy) / d o, with d sigma / d raw = sigmoid(raw + ln(e^0.99 - 1)), 0 where the 1e-4 floor acts;
 *                  dout_critic[m] = sum_n d loss_critic / d v;
 *                  result[0 .. 5] = loss_objective, loss_entropy, loss_critic, entropy, clip_fraction = mean[clamp(lw) != lw], kl_approx = mean(-lw); [6], [7] = 0
 * Tensors (device f32 unless said): index i32 [M]; out [M, N, 4] and dout_actor [M, N, 4], 16-byte aligned; value, dout_critic [M]; action [F, N, 2], 8-byte
 * aligned; sample_log_prob, advantage, value_target [F, N]; result [8]; workspace [SIGMAENV_PPO_SUMS * ceil(M N / 256)].  The records are read in place; duplicates
 * in index are legal; an entry outside [0, F) is never used as an address (its rows give zero gradients and add zeros to the sums -- the means still divide by M N).
 * Arithmetic: fp32, one IEEE operation per operator, no contraction, denormals kept; log1p(+-eps), 1 / (M N), entropy_coeff / (M N) and critic_coeff / (M N) are
 * rounded once, on the host.  Summation order: one lane per (m, n) row r = m N + n, workgroups of 256 rows.  dout_critic[m]: the chain over n = 0, 1, .. from 0.
 * Each mean: per wavefront of 64 consecutive rows the butterfly v += v[lane ^ s], s = 32, 16, .., 1; per workgroup ((w0 + w1) + w2) + w3 over its wavefronts;
 * then one wavefront: lane k the chain over the workgroups k, k + 64, .. from 0, and the same butterfly.  A function of (M, N) alone, no atomics: the same inputs
 * give the same bits on every run.  Two launches on the handle's stream; nothing waits.
 * M < 1, F < 1, a null or misaligned tensor, clip_epsilon outside (0, 1), high <= low: SIGMAENV_EINVAL with sigmaenv_last_error set, before any launch. */
#define SIGMAENV_PPO_SUMS 5
typedef struct sigmaenv_ppo_head_args {
  int32_t n_index;                 /* M */
  int32_t n_frames;                /* F */
  const int32_t* index;
  const float* out;
  const float* value;
  const float* action;
  const float* sample_log_prob;
  const float* advantage;
  const float* value_target;
  float* dout_actor;
  float* dout_critic;
  float* result;
  float* workspace;
  float low[2], high[2];
  float clip_epsilon, entropy_coeff, critic_coeff;
  int32_t reserved0;               /* zero */
  uint64_t seed, counter;
  int32_t reserved[4];             /* zero */
} sigmaenv_ppo_head_args_t;
int sigmaenv_ppo_head(sigmaenv_t* h, const sigmaenv_ppo_head_args_t* a);

/* sigmaenv_ppo_head_1d: the same loss for the priority module (sigmarl/modules/priority_module.py:93-126: a second ClipPPOLoss over the priority actor, a 1-D
 * TanhNormal on [-1, 1], and its own centralised critic).  Everything above holds in one dimension with the trivial bounds; what differs:
 *   shapes         out, dout_actor [M, N, 2] = (loc, raw scale), 8-byte aligned; the recorded score s = scores[f, n] and score_log_prob [F, N] take the place of
 *                  action and sample_log_prob; advantage, value_target [F, N] and value [M] are the PRIORITY critic's
 *   log-prob       torchrl applies no affine map on [-1, 1]: y = clamp(s, +-(1 - 1e-6)) -- not (s + 1) / 1 - 1, which rounds --, x = atanh(y) as above, and
 *                  logp = -(x - loc)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi) - 2 (log 2 - x - softplus(-2 x)): no - log h term
 *                  (sigmaenv_priority_head_kernel's expressions, sigmaenv_dist.h)
 *   entropy draw   z = the cosine branch of a normal pair (cosf, as the priority head draws its score) keyed (seed, counter, env = f, agent = n), draws
 *                  DRAW_PRIORITY_ENTROPY, + 1: both heads can run on one (seed, counter) without sharing a draw
 *   outputs        dout_actor[m, n, 0:2] = d(loss_objective + loss_entropy) / d (loc, raw);  dout_critic, result, the workspace, the order of every sum, the
 *                  treatment of index entries outside [0, F) and the refusals: as above (no bounds to refuse). */
typedef struct sigmaenv_ppo_head_1d_args {
  int32_t n_index;                 /* M */
  int32_t n_frames;                /* F */
  const int32_t* index;
  const float* out;
  const float* value;
  const float* scores;
  const float* score_log_prob;
  const float* advantage;
  const float* value_target;
  float* dout_actor;
  float* dout_critic;
  float* result;
  float* workspace;
  float clip_epsilon, entropy_coeff, critic_coeff;
  int32_t reserved0;               /* zero */
  uint64_t seed, counter;
  int32_t reserved[4];             /* zero */
} sigmaenv_ppo_head_1d_args_t;
int sigmaenv_ppo_head_1d(sigmaenv_t* h, const sigmaenv_ppo_head_1d_args_t* a);

/* ---- the optimiser step of a minibatch update (sigmaenv_optim.inc; the arithmetic: sigmaenv_optim.h) ---------------------------------------
 * sigmaenv_optim_step: the last three lines of _train_on_batch (sigmarl/mappo_cavs.py:421-426) -- torch.nn.utils.clip_grad_norm_(loss_module.parameters(),
 * max_grad_norm) (norm_type = 2, error_if_nonfinite = False: ONE norm over actor and critic together), optim.step() of the torch.optim.Adam of
 * sigmarl/modules/optimization_module.py:69 (weight_decay = 0, amsgrad = False, maximize = False) and, in place of optim.zero_grad() followed by a load, the repack
 * of every given network's weight forms -- for 1 .. 4 networks (SIGMAENV_OPTIM_MAX_NETS) of together at most 32 tensors (SIGMAENV_OPTIM_MAX_TENSORS), three launches on
 * h's stream; nothing waits.  Per network: the sigmaenv_mlp32 handle, optionally the sigmaenv_actor handle of the same network (its bf16 form is then rewritten too;
 * the fp32 handle must then be obs_dim -> 256 -> 256 -> 256 -> 4 with the actor's obs_dim), and eight HOST arrays of DEVICE pointers, one entry per layer as
 * sigmaenv_mlp32_load_device takes the weights: the parameters (weights / biases, torch.nn.Linear layout, contiguous), their gradients, exp_avg and exp_avg_sq, all
 * of the parameters' shapes; 4-byte alignment suffices (no access is wider).  The tensors are taken in the order given: per network, per layer, weight then bias.
 *   norm      every tensor is cut into chunks of 1024 consecutive elements (the last chunk of a tensor may be short), one workgroup of 256 lanes per chunk: lane t the
 *             chain s = 0; s += g[i]^2 over the chunk's elements i = t, t + 256, ..; per wavefront of 64 consecutive lanes the butterfly v += v[lane ^ s], s = 32, 16,
 *             .., 1; ((w0 + w1) + w2) + w3 over the four wavefronts -> workspace[c], c the chunk's number in that sequence.  The P partials are added the same way
 *             once more: lane t the chain over c = t, t + 256, .., the butterfly, the four wavefronts.  total_norm = sqrt(sum);
 *             clip_coef = min(1, max_grad_norm / (total_norm + 1e-6)).  A non-finite gradient: clip_coef is NaN and every parameter becomes NaN (torch's behaviour).
 *   Adam      g' = g clip_coef;  m = m + (g' - m) fl(1 - beta1);  v = fl(beta2) v + (fl(1 - beta2) g') g';  p = p - step_size (m / (sqrt(v) / sqrt_bc2 + fl(eps)))
 *             with step_size = fl(lr / (1 - beta1^t)) and sqrt_bc2 = fl(sqrt(1 - beta2^t)) formed in double on the host and rounded once; p, m, v are updated in
 *             place, the gradients are read, never written.  fp32, one IEEE operation per operator, correctly rounded division and square root, no contraction.
 *   result    device f32 [2] := total_norm, clip_coef.
 *   repack    every form the handles hold -- exact fragments, their transposes, the split pairs, both bias vectors, the bf16 form -- by the per-slot functions
 *             sigmaenv_mlp32_create / sigmaenv_actor_create / *_load_device run (sigmaenv_pack.h), read from the updated parameters themselves: the handles then hold
 *             word for word what *_create makes from those numbers.  The split form's range predicate is reduced into each network's own device word.
 * No atomics in any sum; the shape of every sum is a function of the tensors' element counts alone: the same inputs give the same bits on every run.
 * workspace: device f32 [P] (sigmaenv_optim_workspace: *n_floats := P, the chunks of all tensors; it reads the handles' shapes only).
 * The deferred mode.  The range word decides between SPLIT and EXACT for the next forward, and reading it is a host wait -- which sigmaenv_mlp32_load_device pays on
 * every call.  The training loop never needs the answer: sigmaenv_mlp32_forward_save runs the EXACT chain whatever mode is in force.  So the step does not wait: it
 * leaves every given sigmaenv_mlp32 with EXACT in force -- always correct, the exact form is valid for every weight --, sigmaenv_mlp32_get_mode reports EXACT, and
 * sigmaenv_mlp32_set_mode(SPLIT) is refused but remembered, as it is for a handle outside the range.  sigmaenv_mlp32_resolve_mode(h, m) copies m's range word back on
 * h's stream and waits for it -- the only host wait of the device route, needed once, before the next rollout (after the last minibatch of
 * sigmarl/mappo_cavs.py:421-426's loop) -- and then sets the mode in force exactly as sigmaenv_mlp32_load_device would have: the mode last accepted or remembered by
 * set_mode when the weights allow it, else EXACT.  On a handle that no step has touched it re-derives the mode from the weights the handle holds.
 * More than 4 networks or 32 tensors, a null handle, pointer array or tensor, a tensor that is not 4-byte aligned, an actor handle of another shape, t < 1, a beta
 * outside [0, 1), or eps, lr or max_grad_norm negative or not finite: SIGMAENV_EINVAL with sigmaenv_last_error set, before any launch. */
#define SIGMAENV_OPTIM_MAX_NETS 4
#define SIGMAENV_OPTIM_MAX_TENSORS 32
typedef struct sigmaenv_optim_net {
  sigmaenv_mlp32_t* mlp32;
  sigmaenv_actor_t* actor;           /* optional (NULL): the bf16 handle of the same network */
  float* const* weights;             /* [n_layers] device pointers, updated in place */
  float* const* biases;
  const float* const* grad_weights;  /* read */
  const float* const* grad_biases;
  float* const* exp_avg_weights;     /* updated in place */
  float* const* exp_avg_biases;
  float* const* exp_avg_sq_weights;
  float* const* exp_avg_sq_biases;
} sigmaenv_optim_net_t;
typedef struct sigmaenv_optim_args {
  int32_t n_networks;
  int32_t reserved0;                 /* zero */
  sigmaenv_optim_net_t net[SIGMAENV_OPTIM_MAX_NETS];
  double lr, beta1, beta2, eps, max_grad_norm;
  int64_t t;                         /* the step count of THIS step: 1 for the first */
  float* workspace;
  float* result;
  int32_t reserved[4];               /* zero */
} sigmaenv_optim_args_t;
int sigmaenv_optim_workspace(sigmaenv_t* h, const sigmaenv_optim_args_t* a, uint64_t* n_floats);
int sigmaenv_optim_step(sigmaenv_t* h, const sigmaenv_optim_args_t* a);
int sigmaenv_mlp32_resolve_mode(sigmaenv_t* h, sigmaenv_mlp32_t* m);

/* ---- the prioritized replay buffer (sigmaenv_prb.inc; the arithmetic: sigmaenv_prb.h) -----------------------------------------------------
 * Parameters.is_prb: torchrl's TensorDictPrioritizedReplayBuffer(alpha = 0.7, beta = 0.6, priority_key = "td_error") sized frames_per_batch and overwritten whole
 * by extend every iteration (sigmarl/mappo_cavs.py:321-332), its sample() before every minibatch (:397-407) and _update_priorities_after_training behind every
 * optimiser step (:431-456), as a device object.  torchrl is third-party and absent: the formulas below are the specification, restated from the published
 * behaviour of torchrl 0.9.0.  F = capacity, len <= F the filled length, q[f] the stored priority of frame f, M = n_index.
 *   create    allocates everything the other calls use -- the leaves, the levels, the words total / q_min, the refresh workspace --: none of them allocates, frees
 *             or waits on the host (sigmaenv_prb_get excepted).  alpha, beta, eps are rounded to fp32 once.  destroy frees the object (not h).
 *   extend    REPLACES the content: len = n, q[f] = powf(td[f] + eps, alpha) for f < n (td: device f32 [n], the td_priority of sigmaenv_gae); no ring cursor.  Leaves
 *             in [len, F) count as 0 for the sums and +inf for the minimum.  Then every level is rebuilt.
 *   the hierarchy   fan-out 256: level 0 = the leaves, level k + 1 = one (sum, min) per 256 entries of level k until a level has <= 256 entries; total / q_min =
 *             the sum / min of the one node over the top level.  A node's sum: lane l of 64 the chain ((e_{4l} + e_{4l+1}) + e_{4l+2}) + e_{4l+3}, then the
 *             inclusive scan over the lanes I_l = I_l + I_{l-d} (l >= d), d = 1, 2, .., 32; the sum is I_63.  The order of every operation: sigmaenv_prb.h.
 *   sample    with replacement, proportional to q.  Slot m: u_m = ((k >> 8) + 0.5) 2^-24 of the generator's word k keyed (seed, counter, env = m, agent = 0), draw
 *             DRAW_REPLAY (the draw table of sigmaenv_dist.h);  mass_m = u_m total;  index_out[m] = the lower-bound scan of the prefix sums -- the first f with
 *             mass < q[0] + .. + q[f], clamped to len - 1 -- found by descending the levels: at a node the smallest child j with r < S_j (the children's
 *             inclusive prefixes), then r - S_{j-1} below; if no child qualifies (rounding, u = 1, a NaN) the last child below len.  The index is always in
 *             [0, len).  weight_out[m] = powf(q[index] / q_min, -beta) (<= 1; exactly 1 at a minimal leaf).  total and q_min are read on the device.
 *             ClipPPOLoss of torchrl 0.9.0 does not read "_weight": the weights are an output and sigmaenv_ppo_head does not take them.
 *   refresh   slot m, frame f = index[m]: with v = state_value[m], v' = next_state_value[m] (the critic after the step, on observation[f] and on the record row's
 *             observation part), reward and done read IN PLACE from row f of slab [F, W] (W = N*(D+1)+1, offsets N*D + i and N*(D+1), contiguous frames):
 *             x_m = (sum over i = 0 .. N-1, in that order, of |(r[f,i] + (td_gamma * v') * nd) - v|) / N, nd = 1 - done[f] -- sigmaenv_gae's td_priority expression;
 *             min / max over the M slots OF THIS MINIBATCH (ordered partials, no atomics);  td_m = clamp(((x_m - min) / max(max - min, 1e-3)) * 10, 1e-3, 10);
 *             q[f] = powf(td_m + eps, alpha) (duplicate slots of a frame write the same bits);  td_out (optional, device f32 [M]) := td_m;  then every level is
 *             rebuilt in full: after refresh every level equals bit for bit what extend builds from the same leaves.  An index entry outside [0, len) is never
 *             used as an address: its slot takes no part in min / max and writes nothing (td_out[m] included).  M <= max(F, 65536).
 *   get       copies to the HOST and waits (tests, inspection, checkpoints): SIGMAENV_PRB_LEAVES f32 [len], _TOTAL / _QMIN f32 [1], _LEN / _N_LEVELS i32 [1] (levels,
 *             the leaves included), _LEVEL_SUM + k / _LEVEL_MIN + k f32 [n_k] for k = 1 .. n_levels - 1 (n_0 = F, n_{k+1} = ceil(n_k / 256)).
 * fp32, one IEEE operation per operator, no contraction; powf is the device's (OCML): the two powers are the only operations a host twin cannot reproduce to the
 * bit.  No atomics: the same inputs give the same bits on every run.  Everything is enqueued on h's stream.
 * A null handle, a null or misaligned tensor, M < 1, n < 1 or n > capacity, capacity outside [1, 2^30], alpha outside [0, 1], beta < 0, eps < 0, td_gamma outside
 * [0, 1], sample / refresh on an empty buffer: SIGMAENV_EINVAL with sigmaenv_last_error set, before any launch. */
#define SIGMAENV_PRB_LEAVES 0
#define SIGMAENV_PRB_TOTAL 1
#define SIGMAENV_PRB_QMIN 2
#define SIGMAENV_PRB_LEN 3
#define SIGMAENV_PRB_N_LEVELS 4
#define SIGMAENV_PRB_LEVEL_SUM 16
#define SIGMAENV_PRB_LEVEL_MIN 32
typedef struct sigmaenv_prb sigmaenv_prb_t;
typedef struct sigmaenv_prb_refresh_args {
  int32_t n_index;                 /* M */
  int32_t reserved0;               /* zero */
  const int32_t* index;            /* device i32 [M] */
  const float* state_value;        /* device f32 [M] */
  const float* next_state_value;   /* device f32 [M] */
  const float* slab;               /* device f32 [>= len, W] */
  float* td_out;                   /* optional device f32 [M] */
  float td_gamma;
  int32_t reserved[5];             /* zero */
} sigmaenv_prb_refresh_args_t;
int sigmaenv_prb_create(sigmaenv_t* h, int64_t capacity, double alpha, double beta, double eps, sigmaenv_prb_t** out);
void sigmaenv_prb_destroy(sigmaenv_prb_t* b);
int sigmaenv_prb_extend(sigmaenv_t* h, sigmaenv_prb_t* b, const float* td, int64_t n);
int sigmaenv_prb_sample(sigmaenv_t* h, sigmaenv_prb_t* b, int32_t n_index, uint64_t seed, uint64_t counter, int32_t* index_out, float* weight_out);
int sigmaenv_prb_refresh(sigmaenv_t* h, sigmaenv_prb_t* b, const sigmaenv_prb_refresh_args_t* a);
int sigmaenv_prb_get(sigmaenv_t* h, sigmaenv_prb_t* b, int32_t what, void* host_out);

/* The priority module (sigmarl/modules/priority_module.py).  sigmaenv_priority_forward: priority_net (MultiAgentMLP depth 2: obs_dim -> 256 -> 256 -> 2, Tanh,
 * :34-51) on `obs` (device f32 [B * N, obs_dim], or NULL for SIGMAENV_BUF_OBS), NormalParamExtractor ("biased_softplus_1.0", as the actor's) and a 1-D
 * TanhNormal on [-1, 1] (:52-66): score = clamp(tanh(loc + scale z), -1 + 1e-6, 1 - 1e-6), z from draws DRAW_PRIORITY, + 1 of (seed, counter, env, agent) (0 when
 * deterministic), log_prob = Normal(loc, scale).log_prob(x) - log(1 - tanh(x)^2).  scores / log_prob (optional) device f32 [B, N]; ranks (optional) device
 * i32 [B, N] = sigmaenv_priority_rank of the scores.  scratch: device f32 [B * N * 2].
 * sigmaenv_priority_rank (rank_agents, :118-135): ranks[b, :] = the agents of env b by descending score.  torch.argsort is not stable: here ties go to the
 * LOWER agent index first (a stable descending sort); a NaN score ranks below every number.
 * sigmaenv_priority_random (:147-153, prioritization_method "random"): ranks[b, :] = a uniform permutation of 0 .. N - 1 per env (inside-out Fisher-Yates on
 * draw DRAW_SHUFFLE of (seed, counter, env, agent = i): position i draws j in [0, i]). */
int sigmaenv_priority_forward(sigmaenv_t* h, sigmaenv_mlp32_t* priority_net, const float* obs, float* scratch, float* scores, float* log_prob, int32_t* ranks,
                              uint64_t seed, uint64_t counter, int32_t deterministic);
int sigmaenv_priority_rank(sigmaenv_t* h, const float* scores, int32_t* ranks);
int sigmaenv_priority_random(sigmaenv_t* h, uint64_t seed, uint64_t counter, int32_t* ranks);

/* ---- QP-free CBF margin reward ---------------------------------------------------------------------------
 * CBFQP.update_qp with Parameters.is_solve_qp == False (sigmarl/cbf_qp.py:2534-2560): the nominal CBF constraint margins of every
 * env (compute_nominal_cbf_constraint_margins :2562-2760 -- lane margins from the pseudo distance to both boundaries and its
 * finite-difference gradient / Hessian, sigmarl/pseudo_distance.py:69-242 + cbf_qp.py:575-665; pair margins between the covering
 * circles of every two vehicles :2688-2754; second-order Taylor CBF coefficients :2283-2489) and the three reward channels derived
 * from them (compute_cbf_violation_rewards_from_margins :2762-2804), for all envs in one launch instead of one Python object per
 * env (helper_training.py:1620-1627).  Nominal controllers "rl" (:2605-2615, the policy's action) and "clf" (:2616-2628, a P controller
 * towards the third short-term reference point); no observation noise. */
typedef struct sigmaenv_cbf_config {
  int32_t n_circles;        /* Parameters.n_circles_approximate_vehicle, 1..SIGMAENV_CBF_MAX_CIRCLES */
  int32_t nominal;          /* Parameters.nom_controller_type: 0 = "rl" (cbf_qp.py:2605-2615), 1 = "clf" (:2616-2628) */
  double dt_taylor;         /* cbf_qp.py:370-371: 2 * Parameters.dt */
  double lambda_ttcbf;      /* :404 (0.5) */
  double h_nom;             /* Parameters.h_nom */
  double fd_step;           /* :372-373 (0.02), finite-difference stencil of the pseudo distance */
  double safety_buffer;     /* :403 (0) */
  double circle_radius;     /* RectangleCircleApproximation.radius, sigmarl/rectangle_approximation.py:45-56 */
  double circle_x[SIGMAENV_CBF_MAX_CIRCLES]; /* centres along the length axis (y = 0), :58-70 */
  double l_r, l_wb;         /* constants.py:634-635 (compute_dstate_2nd_time, cbf_qp.py:667-695) */
  float min_speed, min_steering; /* constants.py:637-640; the maxima, acceleration and steering-rate limits come from the env config */
  double steering_rate_max;       /* constants.py:645-646 in double (pi / 2; the minimum is its negative): the QP's box and the "clf" controller's clip are float64 in the reference */
  double k_clf_speed, k_clf_heading, ref_speed; /* "clf" nominal controller, cbf_qp.py:408-417 (defaults 1, 1, 1 m/s) */
  /* centralized CBF-QP (sigmaenv_cbf_qp), cbf_qp.py:409-433, 914-927 */
  double qp_w_acc, qp_w_steer;   /* nom_weight = diag(10, 1): tracking cost sum ((u - u_nom) @ nom_weight)^2 */
  double qp_w_lane, qp_w_pair;   /* lane_slack_weight, pair_slack_weight (1e9) */
  double qp_w_clf;               /* w_clf_relax (1) */
  double qp_w_lambda;            /* lambda_weight (1e3) when Parameters.adaptive_lambda, else 0 (:924-927) */
  double lam_clf;                /* lam_clf (2) */
  int32_t is_apply_cbf_action;   /* Parameters.is_apply_cbf_action: which action SIGMAENV_BUF_CBF_NOMINAL receives (below) */
  /* grouped CBF-QPs (Parameters.is_grouping_agents, cbf_qp.py:1562-2281): sigmaenv_cbf_qp then solves, per env, the ceil(N / max_group_size)
   * group problems of build_grouped_cbf_qps instead of the centralized one (below) */
  int32_t is_grouping;           /* Parameters.is_grouping_agents */
  int32_t max_group_size;        /* Parameters.max_group_size (m): capacity of a group */
  int32_t reserved4;
  double observation_range;      /* Parameters.observation_range: cross-group rows only against external vehicles within this distance (:2094-2109) */
  double rs;                     /* Parameters.rs: share of a cross-group row's h a vehicle takes on (rs * h * lambda, :1751-1757) */
  double qp_w_cross;             /* cross_slack_weight (1e9, :428-430) */
  double qp_w_lambda_cross;      /* lambda_weight (1e3): the cross-group lambdas are always penalised (:1789-1791) */
} sigmaenv_cbf_config_t;

/* seg_left / seg_right: HOST pointers f32 [n_paths, seg_stride, 5] = per boundary segment (cos, sin, m_b, m_t, length): the
 * map-only part of PseudoDistance.get_pseudo_distance (pseudo_distance.py:43-56,94-103,174-177), for the paths of the map the
 * handle was created with.  Copied to the device. */
int sigmaenv_cbf_attach(sigmaenv_t* h, const sigmaenv_cbf_config_t* cfg, const float* seg_left, const float* seg_right, int32_t seg_stride);

/* actions: DEVICE f32 [B,N,2], the policy's action (target speed, target steering) the step is about to receive.  Writes rows 5
 * (rew_near_left_lane), 6 (rew_near_right_lane) and 4 (rew_near_other_agents) of SIGMAENV_BUF_REWARD_INFO, which the next
 * sigmaenv_step adds to the reward when SIGMAENV_REW_CBF is set.  margins: optional DEVICE f64 buffer receiving
 * lane_left [B,N,C], lane_right [B,N,C], pair [B,N,N,C,C] (entries with i < j), back to back; NULL to skip. */
int sigmaenv_cbf_rewards(sigmaenv_t* h, const float* actions, double* margins);

/* Test hook.  centers: DEVICE f32 [B,N,C,2] (C = n_circles) or NULL.  While set, sigmaenv_cbf_rewards / sigmaenv_cbf_qp take the covering-circle centres from it
 * instead of computing them (get_circle_centers, sigmarl/cbf_qp.py:527-573).  The reference rounds the pseudo distance to fp16 and differentiates it numerically, so a
 * 1-ulp difference of a float32 centre (torch's closed cos / sin against this library's correctly rounded ones) can flip an fp16 rounding; the parity tests inject the
 * centres the reference itself computed (recorded in the CBF goldens) and then hold every CBF quantity to 2e-6 without exceptions. */
int sigmaenv_cbf_inject_centers(sigmaenv_t* h, const float* centers);

/* The centralized CBF-QP safety filter of every env (CBFQP.update_centralized_cbf_qp with Parameters.is_solve_qp,
 * sigmarl/cbf_qp.py:733-1019 problem, :1019-1400 data + solve): per env
 *     min  sum_i |(u_i - u_nom_i) W|^2 + w_lane |s_lane|^2 + w_pair |s_pair|^2 + w_clf (|s_head|^2 + |s_speed|^2) [+ w_lambda |lambda|^2]
 *     s.t. a_min <= u_i0 <= a_max, rate_min <= u_i1 <= rate_max, s >= 0, 0 <= lambda <= 1,
 *          lane (i, c, side):      A u_i + b0 + h lambda >= -s          (ttcbf_lane_affine_coeffs, adaptive branch :2341-2369)
 *          pair (i < j, ci, cj):   A_i u_i + A_j u_j + b0 + h lambda >= -s   (ttcbf_pair_affine_coeffs :2406-2447)
 *          CLF (i):  -e_head u_i1 + lam_clf e_head^2 / 2 <= s_head,  -e_speed u_i0 + lam_clf e_speed^2 / 2 <= s_speed   ("clf" only)
 * with the data of sigmaenv_cbf_rewards.  The reference hands the problem to cvxpy / OSQP (eps 1e-5, polished); here every slack
 * and lambda is eliminated in closed form (each appears in one constraint) and the remaining strictly convex, piecewise quadratic
 * problem in the 2N controls is solved to machine precision by a projected Newton method -- the same minimiser, not the same
 * iterates.  actions: DEVICE f32 [B,N,2] policy actions.  actions_safe: DEVICE f32 [B,N,2] = u_to_rl_action(u*, v, steering)
 * (:499-525): what the reference writes into the action tensor when is_apply_cbf_action, and into
 * world_state.nominal_action_{vel,steer} otherwise.  u_opt (optional): DEVICE f64 [B,N,2] the minimiser (acceleration, steering
 * rate).  info (optional): DEVICE i32 [B,2] = Newton iterations, converged flag.  SIGMAENV_BUF_CBF_NOMINAL receives what the reference
 * leaves in world_state.nominal_action_*: the safe action when is_apply_cbf_action == 0 (the caller then steps with the policy's action,
 * :1343-1379), the clamped policy action when it is 1 (the caller steps with actions_safe, :1262-1283, 1315-1325); with
 * SIGMAENV_REW_CBF_QP the next step penalises the distance between the two (road_traffic.py:1117-1135).  n_agents <= 64 (SIGMAENV_EINVAL
 * beyond: the 2N x 2N Hessian is kept in LDS).  Repeated launches on the same state return the same bits. */
int sigmaenv_cbf_qp(sigmaenv_t* h, const float* actions, float* actions_safe, double* u_opt, int32_t* info);

/* Grouped mode (cfg.is_grouping): per env the vehicles are partitioned ONCE into K = ceil(N / m) groups by group_agents_k_nearest
 * (cbf_qp.py:193-310: farthest-point seeds, then every vehicle joins the nearest group with room; members sorted, groups ordered by their
 * first member) from the positions at the first sigmaenv_cbf_qp call, and kept for the rest of the run (use_fixed_groups, :1897-1909).  Each
 * group problem (:1562-1856) has the lane rows of its members, the pair rows of its member pairs, and per member i and external vehicle j
 * within observation_range the ONE-SIDED rows  A_i u_i + b0 / 2 + rs h lambda >= -s  (ttcbf_pair_affine_coeffs_cross :2491-2532; slack
 * weight qp_w_cross, lambda always penalised).  The group problems share no variable, so sigmaenv_cbf_qp solves them as one block-separable
 * problem in the 2N controls: the same minimisers.  As in the reference the safe action always replaces the action
 * (actions_safe) and SIGMAENV_BUF_CBF_NOMINAL receives the clamped policy action ("rl", :2254-2260) or U_nom ("clf", :2262-2268).
 * Requires is_solve_qp semantics (the reference's grouped update raises otherwise: its coefficient builders receive lam = None).
 * sigmaenv_cbf_regroup: forget the groups (the next sigmaenv_cbf_qp call forms them again: what constructing new CBFQP objects does).
 * sigmaenv_cbf_get_groups: HOST i32 [B,N] group index of every vehicle (SIGMAENV_EINVAL before the first grouped call). */
int sigmaenv_cbf_regroup(sigmaenv_t* h);
int sigmaenv_cbf_get_groups(sigmaenv_t* h, int32_t* groups_host);

/* ---- the challenging initial-state buffer (sigmaenv_isb.inc; the index arithmetic and the decisions: sigmarl_amd/csrc/sigmaenv_isb.h) ---------------------
 * Parameters.is_challenging_initial_state_buffer: a per-step history of the states (sigmarl/scenarios/road_traffic.py:702-708, :1226-1240), on an agent-agent
 * collision the state n_steps_stored steps back goes into a circular bank (:1415-1427; CircularBuffer / InitialStateBuffer, sigmarl/helper_scenario.py:424-508), and
 * a finished env restarts from a random bank entry with probability probability_use_recording (:857-873, world_state_rt_sim.py:57-71, :162-178).  In the reference
 * the first use of a recording raises (`if initial_state:` on an [N, 8] tensor, world_state_rt_sim.py:162), so no golden exists: sigmaenv_isb.h is the specification
 * -- rings, ranks, bank slots, the three draws DRAW_ISB_RECORD / _USE / _INDEX keyed (seed, counter, env_index_base + b, agent 0) -- and lists the four departures
 * (the whole state row is kept and restored; one ring per env; one record draw per env; the restart is sigmaenv_reset(full_env = 1)).
 * An entry of one env: its N rows of SIGMAENV_BUF_STATE and its N rows of SIGMAENV_BUF_PATH.  Everything is enqueued on the handle's stream; record, restart and
 * settle never wait on the host, and no state, index or probability visits it.
 *
 * sigmaenv_isb_create   <- InitialStateBuffer / StateBuffer construction, road_traffic.py:702-708 (capacity 100, probability_record 1.0, probability_use_recording 0.2
 *                          there; n_steps_stored from Parameters).  A bank of THIS handle (its B and N): capacity 1 .. 65536 entries, a ring of n_steps_stored
 *                          (1 .. 1024) entries per env.  Allocates (do not call inside a stream capture) and ends with a sigmaenv_isb_reset.
 * sigmaenv_isb_destroy  the bank; a bank outlives its handle only for this call.
 * sigmaenv_isb_reset    <- CircularBuffer.reset (helper_scenario.py:465-469) + the first state_buffer.add: empties the bank (ptr = count = 0) and every ring, then
 *                          pushes every env's current rows and takes the envs' episodes_reset as the bank's copy.
 * sigmaenv_isb_record   <- state_buffer.add (road_traffic.py:1226-1240) and the recording of done() (:1415-1427).  Runs on the frame a step left, before any reset:
 *                          push, collided[b] = any byte of SIGMAENV_BUF_COL_AGENTS[b], the record draw, the ordered write of nth_latest(n_steps_stored) of the R
 *                          recording envs into the bank (the last `capacity` of them survive), ptr / count, pending[b] = env not done and a reset request
 *                          (SIGMAENV_BUF_COL_FLAGS[b, ., 3]) set.  Two launches: one lane per env, then ONE workgroup that ranks the recorders.
 * sigmaenv_isb_restart  <- reset_world_at's use of a recording (:857-873, world_state_rt_sim.py:57-71, :162-178).  Runs before sigmaenv_auto_reset: an env with
 *                          done[b] restarts from entry j of the bank iff count >= 1 and u < p_use (count includes this step's recordings); the restart is
 *                          sigmaenv_reset(full_env = 1) with the entry's N (path, state) rows, the entries staying on the device (step counter 0, episodes_reset + 1,
 *                          done cleared, derived state, mutual distances, collision flags, prev_pos), followed by a fresh observation of the env.  Envs not chosen
 *                          stay done for sigmaenv_auto_reset, whose draws are keyed per env and so do not move.  A loaded entry whose path index lies outside the
 *                          path table is never used: its env stays done.
 * sigmaenv_isb_settle   <- state_buffer.reset + add at the end of every reset_world_at (:909-923, single-agent resets included).  Runs after sigmaenv_auto_reset:
 *                          every env whose episodes_reset differs from the bank's copy, and every env with pending[b], has its ring cleared and its current rows
 *                          pushed; the copy is refreshed.
 * sigmaenv_isb_attach(h, bank) / (h, NULL): while a bank is attached, every step of sigmaenv_rollout, sigmaenv_rollout_f32 and sigmaenv_rollout_f32_ex (every wrapper,
 *                          and the CBF chain) runs as sigmaenv_step -> (sigmaenv_eval_accumulate, if an evaluator is attached as well) -> sigmaenv_isb_record ->
 *                          sigmaenv_isb_restart -> sigmaenv_auto_reset -> sigmaenv_isb_settle with the action, the record row block, the (seed, counter0 + t) keys
 *                          and the path range of the fused launch it replaces (a rollout with path_count 0 -- no device-side resets -- only records).  With
 *                          p_use = 0 the rollout is the unattached one, bit for bit.  With nothing attached the rollouts are unchanged.  Direct calls of
 *                          sigmaenv_step_autoreset, sigmaenv_step_autoreset_many and sigmaenv_step_autoreset_n never consult a bank.
 * sigmaenv_isb_get      DEVICE pointers into the bank, for tests and checkpoints (no wait, no copy): see SIGMAENV_ISB_*.
 * sigmaenv_isb_set      loads the first `count` (0 .. capacity) entries from DEVICE tensors state_rows f32 [count, N, 8] and path_rows i32 [count, N, 4] -- a saved
 *                          bank, or a hand-made scenario set -- and sets count and ptr = count mod capacity.  The rings are left as they are. */
typedef struct sigmaenv_isb sigmaenv_isb_t;
#define SIGMAENV_ISB_BANK_STATE 0 /* f32 [capacity, N, 8] */
#define SIGMAENV_ISB_BANK_PATH 1  /* i32 [capacity, N, 4] */
#define SIGMAENV_ISB_WORDS 2      /* i32 [2]: ptr, count */
#define SIGMAENV_ISB_RING_STATE 3 /* f32 [B, n_steps_stored, N, 8] */
#define SIGMAENV_ISB_RING_PATH 4  /* i32 [B, n_steps_stored, N, 4] */
#define SIGMAENV_ISB_HELD 5       /* i32 [B] */
#define SIGMAENV_ISB_HEAD 6       /* i32 [B] */
#define SIGMAENV_ISB_PENDING 7    /* u8  [B] */
#define SIGMAENV_ISB_EPISODES 8   /* i32 [B]: the bank's copy of the envs' episodes_reset (sigmaenv_isb_settle compares against it); with ids 0 .. 7 every word a
                                   * checkpoint of the bank holds */
#define SIGMAENV_ISB_CHUNK 1024   /* envs per chunk of sigmaenv_isb_record's ranking workgroup (ISB_CHUNK of sigmaenv_isb.h) */
int sigmaenv_isb_create(sigmaenv_t* h, int32_t capacity, int32_t n_steps_stored, float p_record, float p_use, sigmaenv_isb_t** out);
void sigmaenv_isb_destroy(sigmaenv_isb_t* bank);
int sigmaenv_isb_reset(sigmaenv_t* h, sigmaenv_isb_t* bank);
int sigmaenv_isb_record(sigmaenv_t* h, sigmaenv_isb_t* bank, uint64_t seed, uint64_t counter);
int sigmaenv_isb_restart(sigmaenv_t* h, sigmaenv_isb_t* bank, uint64_t seed, uint64_t counter);
int sigmaenv_isb_settle(sigmaenv_t* h, sigmaenv_isb_t* bank);
int sigmaenv_isb_attach(sigmaenv_t* h, sigmaenv_isb_t* bank);
int sigmaenv_isb_get(sigmaenv_t* h, sigmaenv_isb_t* bank, int32_t what, void** dev_ptr, size_t* bytes);
int sigmaenv_isb_set(sigmaenv_t* h, sigmaenv_isb_t* bank, const float* state_rows, const int32_t* path_rows, int32_t count);

/* ---- Snapshot and restore of a handle's state (sigmarl_amd/csrc/sigmaenv_snapshot.h, sigmaenv_snapshot.inc) --------------------------------------------------------
 * The reference resumes a training run from the policy's and the critic's weights alone (is_load_model / is_continue_train, sigmarl/mappo_cavs.py:100-105, :219-306):
 * the envs start afresh.  Here every draw is a function of (seed, counter, env, agent, draw id) and no kernel uses atomics, so a handle whose buffers are put back
 * continues bit for bit.  The STATE of a handle is every device buffer whose content at the start of a call can change a later result -- the 21 SIGMAENV_BUF_*,
 * reset_mask, reset_full, fresh (SIGMAENV_OBS_BOUNDARY_POINTS), cbf_groups (CBF tables attached with is_grouping) -- and two host words (the count of stand-alone
 * sigmaenv_observe calls, the validity of the CBF groups).  sigmaenv_snapshot.h is the one statement of the segment table (id, element size, bytes per env, outer
 * blocks and their stride, offset in the blob; offsets are multiples of 16; a total) and lists what is deliberately not state: scratch, staging, workspaces, timing
 * pools and the caller's settings (slab pointer and strides, observation record, attached evaluator or bank, lanelet and scenario lists).
 *
 * sigmaenv_state_layout   fills the host header of the handle as it stands: magic, layout version, the seven quantities the layout is a function of (n_envs, n_agents,
 *                         n_nearing, obs_dim, n_short_term, obs_flags, cbf: 0 none / 1 tables attached / 2 attached with groups), total_bytes and the two host words.
 *                         No build id: a blob outlives a rebuild that leaves the layout alone.  Launches nothing, waits for nothing.
 * sigmaenv_state_save     packs every segment into dev_blob (DEVICE, 16-byte aligned, bytes == total_bytes) in ONE launch on the handle's stream; no host wait.  Every
 *                         byte of the blob is written (the padding between segments with zeros): equal states give equal blobs.  The
 *                         host words of that moment are the ones sigmaenv_state_layout returns when called next to it.
 * sigmaenv_state_restore  the inverse.  env_mask == NULL: every env, and the handle takes over the header's host words.  Otherwise env_mask is a DEVICE u8 [n_envs]:
 *                         only envs with a non-zero byte are written, in every segment; no word of another env is stored to (not even with its own value), and the
 *                         host words stay.  Afterwards the selected envs' buffers are the snapshot's bits; nothing is re-derived.  ONE launch, no host wait.
 * Refused with SIGMAENV_EINVAL before any launch (sigmaenv_last_error names the reason): a null or not 16-byte aligned blob; bytes != total_bytes; a header whose
 * magic, version or any of the seven quantities differs from the handle's (the message names the first difference). */
#define SIGMAENV_STATE_MAGIC 0x50414E53u /* "SNAP" */
#define SIGMAENV_STATE_VERSION 1u
typedef struct sigmaenv_state_header {
  uint32_t magic, version;
  int32_t n_envs, n_agents, n_nearing, obs_dim, n_short_term, obs_flags, cbf;
  uint32_t observe_calls;     /* host word: stand-alone sigmaenv_observe calls so far */
  uint32_t cbf_groups_valid;  /* host word: the grouped CBF-QP has formed its partition */
  uint32_t reserved0;
  uint64_t total_bytes;
  uint32_t reserved[2];
} sigmaenv_state_header_t;
int sigmaenv_state_layout(sigmaenv_t* h, sigmaenv_state_header_t* out);
int sigmaenv_state_save(sigmaenv_t* h, void* dev_blob, size_t bytes);
int sigmaenv_state_restore(sigmaenv_t* h, const sigmaenv_state_header_t* hdr, const void* dev_blob, size_t bytes, const uint8_t* env_mask);

/* ---- Frames of selected envs, drawn on the device (sigmarl_amd/csrc/sigmaenv_render.inc; the picture: sigmaenv_render.h) ---------------------------------------------
 * What the reference shows through env.render / extra_render and save_video (sigmarl/scenarios/road_traffic.py:1637-1800; is_save_simulation_video,
 * is_real_time_rendering, is_visualize_short_term_path, is_visualize_lane_boundary): a top-down view of map, short-term reference paths and vehicles.  The reference's
 * renderer is a pyglet scene graph; it supplies the list of things drawn, sigmaenv_render.h specifies the pixels (view, fp32 predicates, layers, sample mean, palette,
 * tile walk), and a frame is held to it bit for bit.  A frame of env b reads SIGMAENV_BUF_VERTICES[b,i,0:4], SIGMAENV_BUF_SHORT_TERM[b,i], SIGMAENV_BUF_STATE[b,i,0:2],
 * SIGMAENV_BUF_COL_AGENTS[b,i,:], byte 0 of SIGMAENV_BUF_COL_FLAGS[b,i,:] and the map table's left / right polylines -- as the buffers stand when the launch runs.
 * The renderer holds no env state: nothing of it is part of sigmaenv_state_layout, and an attachment is a caller's setting like an attached evaluator.
 *
 * sigmaenv_render_create   <- the scene set-up of extra_render, road_traffic.py:1637-1659 (the geoms of the lane boundaries :1700-1730 are drawn ONCE here: the background
 *                          kernel rasterises layers 0 and 1 into a device coverage image u16 [H,W] and the map's resolved colours u8 [H,W,3]; the map never visits the
 *                          host as an image).  args: the view (scale px / m, the world point (x0, y1) of the top-left corner), height, width (a multiple of 4), samples
 *                          per axis (1, 2, 4), the half-widths in pixels, flags, the HOST palette u8 [3 + N, 3] (background, boundary, collision, agents), the HOST
 *                          selection i32 [n_sel] (duplicates are legal; an entry outside [0, B) is refused) and ring_frames (0: no ring).  Allocates and waits for the
 *                          two small copies: do not call inside a stream capture.
 * sigmaenv_render_frame    <- one env.render() call, road_traffic.py:1660-1800 (short-term paths :1660-1698, vehicles and heading :560-600): ONE launch on the handle's
 *                          stream, grid = tiles x selected envs, into out (DEVICE u8 [n_sel, H, W, 3], 16-byte aligned) or, out NULL, into the next ring slot.
 *                          src NULL: the handle's buffers; otherwise each non-null pointer of src replaces the handle's buffer of that name, in the handle's own
 *                          layout, 4-byte aligned (the rules of sigmaenv_eval_src_t): how recorded trajectories are drawn after the fact.
 * sigmaenv_render_attach   (h, r, every) / (h, NULL, 0) <- save_video's frame list, one env.render() per step of the rollout: while a renderer is attached, every
 *                          step of sigmaenv_rollout* (every wrapper, and the CBF chain) is taken apart exactly as for an evaluator and the frame of every `every`-th
 *                          step since the attachment goes to the ring: sigmaenv_step -> (sigmaenv_eval_accumulate) -> frame -> (sigmaenv_isb_record ->
 *                          sigmaenv_isb_restart) -> sigmaenv_auto_reset -> (sigmaenv_isb_settle).  The frame shows the step's outcome BEFORE the re-placements clear
 *                          it; end state and records are the fused rollout's, bit for bit.  Needs a ring.  Direct calls of sigmaenv_step_autoreset* are NOT affected.
 * sigmaenv_render_get      the ring's DEVICE base (NULL without one), the frames drawn so far as the host counts them (into the ring or a caller's tensor), those of
 *                          them drawn into the ring (slot = count mod ring_frames) and the ring slot of the newest ring frame (-1 before the first); any of the
 *                          four destinations may be NULL.  No wait.
 * sigmaenv_render_destroy  waits for the handle's stream, detaches, frees.  A renderer whose handle was destroyed first can only be destroyed.
 * Refused with SIGMAENV_EINVAL and sigmaenv_last_error set, before any launch: a null handle (no message), a null renderer, a renderer of another handle; at create a
 * width that is no multiple of 4, samples outside {1, 2, 4}, a selection entry outside [0, B), a non-finite view, unknown flags; an override that is not 4-byte
 * aligned, an out that is not 16-byte aligned, no out and no ring; attaching with every < 1 or without a ring. */
typedef struct sigmaenv_render sigmaenv_render_t;
#define SIGMAENV_RENDER_SHORT_TERM 1 /* flags: draw layer 2, the short-term reference paths (is_visualize_short_term_path) */
typedef struct sigmaenv_render_args {
  float scale, x0, y1;             /* the view: px = (x - x0) * scale, py = (y1 - y) * scale */
  float h_boundary, h_path;        /* half-widths in pixels: lane boundaries; short-term paths and heading marks */
  int32_t height, width, samples;  /* width a multiple of 4; samples per axis 1, 2 or 4 */
  int32_t flags;                   /* SIGMAENV_RENDER_* */
  int32_t n_sel, ring_frames;
  int32_t reserved0;               /* zero */
  const uint8_t* palette;          /* HOST u8 [3 + n_agents, 3] */
  const int32_t* selection;        /* HOST i32 [n_sel] */
  int32_t reserved[4];             /* zero */
} sigmaenv_render_args_t;
typedef struct sigmaenv_render_src {
  const float* vertices;           /* optional device f32 [B, N, 5, 2] */
  const float* short_term;         /* optional device f32 [B, N, n_points_short_term, 2] */
  const float* state;              /* optional device f32 [B, N, 8] */
  const uint8_t* col_agents;       /* optional device u8 [B, N, N] */
  const uint8_t* col_flags;        /* optional device u8 [B, N, 4] */
  int32_t reserved[4];             /* zero */
} sigmaenv_render_src_t;
int sigmaenv_render_create(sigmaenv_t* h, const sigmaenv_render_args_t* args, sigmaenv_render_t** out);
void sigmaenv_render_destroy(sigmaenv_render_t* r);
int sigmaenv_render_frame(sigmaenv_t* h, sigmaenv_render_t* r, const sigmaenv_render_src_t* src, uint8_t* out);
int sigmaenv_render_attach(sigmaenv_t* h, sigmaenv_render_t* r, int32_t every);
int sigmaenv_render_get(sigmaenv_t* h, sigmaenv_render_t* r, void** ring, uint64_t* frames, uint64_t* ring_drawn, int32_t* newest_slot);

#ifdef __cplusplus
}
#endif
#endif /* SIGMAENV_H */
