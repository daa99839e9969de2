// sigmaenv_cbf.inc -- the CBF module on the device (included by sigmaenv.hip): sigmarl/cbf_qp.py + sigmarl/pseudo_distance.py for every env of
// the batch per launch instead of one Python object (and one cvxpy / OSQP solve) per env.
//
// Shared data path (cbf_qp.py:461-727, 2283-2489):
//   * kernel A (sigmaenv_cbf_kin_kernel, one lane per vehicle): covering-circle centres, nominal action ("rl" / "clf"), linearised centre
//     kinematics in float64;
//   * stencil_phase: pseudo distance of 9 stencil points to both lane boundaries for every circle (pseudo_distance.py:69-242, cbf_qp.py:575-665),
//     rounded to fp16 like the reference -- LPT lanes per (vehicle, side) task over the boundary segments of the chunks a bounding-box bound cannot
//     exclude, in two stages: an interval test on the circle centre's projection picks the (segment, circle) candidates, the 9 points are evaluated
//     exactly only for those; lane_estimate: the numpy-float16 finite differences.
// Consumers:
//   * kernel B (sigmaenv_cbf_kernel, workgroup per env): QP-free margins A u + b at the nominal action and the three reward channels
//     (update_qp with is_solve_qp == False, cbf_qp.py:2534-2804);
//   * kernel C (sigmaenv_cbf_qp_kernel<BIG, LEAN, DEFER>, workgroup per env): the centralized CBF-QP (cbf_qp.py:733-1400) -- slacks / lambdas
//     eliminated in closed form, projected Newton on the 2N controls.  Up to 32 vehicles: the LEAN instantiation (12 KB of LDS, two wavefronts per env,
//     the kinematics of kernel A evaluated in its prologue on four lanes per vehicle) + a follow-up launch of the full layout for the envs it flags.
// Arithmetic contract: see oracle/sigmaenv_cbf_oracle.inc (the fp32 / fp16 part is bit-identical to the oracle; the float64 part differs
// only through the device's double-precision sin / cos / tan / atan, and -- in the QP -- through the summation order of its accumulations).

#include <hip/hip_fp16.h>

// wavefront-level ordering point of LDS traffic (one wavefront's LDS instructions execute in order; this keeps the compiler from moving them across)
#define QP_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

namespace cbf {

__device__ __forceinline__ float half_round(float x) { return __half2float(__float2half_rn(x)); }  // IEEE binary16, nearest even

struct Kin { double dx, dy, ax0, ax1, cx, ay0, ay1, cy; };  // per (vehicle, circle): kins["dx"], ["dy"], ["a_ddx"], ["c_ddx"], ["a_ddy"], ["c_ddy"]
struct LaneEst { double sm, g0, g1, h00, h01, h11; };

// ttcbf_lane_affine_coeffs (non-adaptive) + A u + b, cbf_qp.py:2370-2398, 2668-2686
__device__ inline double lane_margin(const sigmaenv_cbf_config_t& cc, const Kin& kn, const LaneEst& e, double u0, double u1) {
  const double dt = cc.dt_taylor, lam = cc.lambda_ttcbf;
  const double h = e.sm - cc.safety_buffer;
  const double dot_h = e.g0 * kn.dx + e.g1 * kn.dy;
  const double A0 = 0.5 * (dt * dt) * (e.g0 * kn.ax0 + e.g1 * kn.ay0);
  const double A1 = 0.5 * (dt * dt) * (e.g0 * kn.ax1 + e.g1 * kn.ay1);
  const double vh0 = kn.dx * e.h00 + kn.dy * e.h01, vh1 = kn.dx * e.h01 + kn.dy * e.h11;
  const double const_dd = e.g0 * kn.cx + e.g1 * kn.cy + (vh0 * kn.dx + vh1 * kn.dy);
  const double b = lam * h + dot_h * dt + 0.5 * (dt * dt) * const_dd;
  return (A0 * u0 + A1 * u1) + b;
}
// ttcbf_pair_affine_coeffs (non-adaptive) + margin, cbf_qp.py:2448-2489, 2733-2754
__device__ inline double pair_margin(const sigmaenv_cbf_config_t& cc, const Kin& ki, const Kin& kj, double dx, double dy, double d_safe_sq, double ui0,
                                     double ui1, double uj0, double uj1) {
  const double dt = cc.dt_taylor, lam = cc.lambda_ttcbf;
  const double vrel_x = ki.dx - kj.dx, vrel_y = ki.dy - kj.dy;
  const double h = dx * dx + dy * dy - d_safe_sq;
  const double dh = 2.0 * (dx * vrel_x + dy * vrel_y);
  const double f = 0.5 * (dt * dt) * 2.0, fm = 0.5 * (dt * dt) * -2.0;
  const double Ai0 = f * (dx * ki.ax0 + dy * ki.ay0), Ai1 = f * (dx * ki.ax1 + dy * ki.ay1);
  const double Aj0 = fm * (dx * kj.ax0 + dy * kj.ay0), Aj1 = fm * (dx * kj.ax1 + dy * kj.ay1);
  const double const_ddh = 2.0 * (vrel_x * vrel_x + vrel_y * vrel_y) + 2.0 * (dx * (ki.cx - kj.cx) + dy * (ki.cy - kj.cy));
  const double b = lam * h + dh * dt + 0.5 * (dt * dt) * const_ddh;
  return (Ai0 * ui0 + Ai1 * ui1) + (Aj0 * uj0 + Aj1 * uj1) + b;
}
__device__ __forceinline__ double clip_d(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }  // NaN stays NaN

// ---- kernel A: per vehicle -- circle centres, nominal action, linearised centre kinematics (cbf_qp.py:2586-2615, 2283-2335) --------
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// kin_vehicle: one vehicle (bi = env * N + vehicle); its C circle centres and centre kinematics go to out_cxy[0 .. C) / out_kin[0 .. C) -- global memory for
// sigmaenv_cbf_kin_kernel (the margin rewards' launch, and the QP's when circle centres are injected), the workgroup's LDS when sigmaenv_cbf_qp_kernel evaluates them itself.
// The float64 trigonometry is the expensive part (every distinct value is evaluated once): a chain of three dependent rounds -- sincos(yaw) | sincos(steering), then the two
// arctangents of the slip angle, then three sincos of (yaw + slip, float32 and float64) and of the slip angle.  LANES says where the evaluations run:
//   LANES == 1 (sigmaenv_cbf_kin_kernel): all seven in the vehicle's one lane, which then takes every circle;
//   LANES == 4 (the QP kernel's prologue: 16 vehicles = one wavefront): the evaluations of a round are independent, so each runs in a lane of its own (same function, other
//   argument) and the results cross the quad by DPP -- seven evaluations deep -> three; after that lane `sub` of the quad takes circle `sub`.  All four lanes of a quad must
//   be active.
// Only the two `if constexpr` places and the range of the two circle loops depend on LANES; everything else is one statement of the operations, so both forms return
// the same bits (tests/test_gpu_cbf.py: test_cbf_qp_one_lane_and_four_lane_kinematics_agree_bitwise).
template <int LANES>
__device__ __forceinline__ void kin_vehicle(const sigmaenv_config_t& c, const sigmaenv_cbf_config_t& cc, const DevBufs& g, const float* __restrict__ actions, size_t bi, int sub,
                                            float2* __restrict__ out_cxy, double2& out_u, Kin* __restrict__ out_kin, double2& out_clf) {
  static_assert(LANES == 1 || LANES == 4, "one lane per vehicle, or a quad");
  const int C = cc.n_circles;
  constexpr bool QUAD = LANES == 4;  // the two circle loops below: every circle, or -- in a quad -- circle `sub` if there is one
  const float4 s0 = reinterpret_cast<const float4*>(g.state + bi * 8)[0];
  const float delta_f = g.state[bi * 8 + 4];
  const float2 a = reinterpret_cast<const float2*>(actions)[bi];
  const float px = s0.x, py = s0.y, psi_f = s0.z, v_f = s0.w;
  const double psi = psi_f, v = v_f, delta = delta_f;
  // the trigonometric values every formula below shares (same function, same argument: same value as evaluating them in place)
  // (the float64 kernels of the contract's sin / cos / atan -- fdlibm's, below 1 ulp -- instead of the device library's: a third of the instructions, and their
  // float32 roundings ARE cr_sin / cr_cos / cr_tan)
  double sin_psi, cos_psi, sin_delta, cos_delta;
  if constexpr (LANES == 1) {
    sigma_sincos_f64(psi, &sin_psi, &cos_psi);
    sigma_sincos_f64(delta, &sin_delta, &cos_delta);
  } else {  // round 1: lane 0 sincos(psi), lane 1 sincos(delta)
    double r1s, r1c;
    sigma_sincos_f64(sub == 1 ? delta : psi, &r1s, &r1c);
    sin_psi = dpp_f64<0x00>(r1s); cos_psi = dpp_f64<0x00>(r1c);
    sin_delta = dpp_f64<0x55>(r1s); cos_delta = dpp_f64<0x55>(r1c);
  }
  const double tan_delta = sin_delta / cos_delta;
  const float sn = (float)sin_psi, cs = (float)cos_psi;  // cr_sin / cr_cos of the yaw
  // get_circle_centers, cbf_qp.py:527-573 (float32).  QUAD: the loop is `if (sub < C)` on circle sub -- it starts at sub and steps by C >= 1, so one pass at most
  for (int ci = QUAD ? sub : 0; ci < C; ci += QUAD ? C : 1) {
    const float lx = (float)cc.circle_x[ci];
    out_cxy[ci] = make_float2((cs * lx + (-sn) * 0.0f) + px, (sn * lx + cs * 0.0f) + py);
  }
  if (cc.nominal == 0) {
    // rl_action_to_u (float32), cbf_qp.py:461-497
    const float r0 = clampf(a.x, cc.min_speed, c.max_speed), r1 = clampf(a.y, cc.min_steering, c.max_steering);
    const float ua = clampf((r0 - v_f) / c.dt, c.min_acc, c.max_acc);
    const float us = clampf((r1 - delta_f) / c.dt, c.min_steering_rate, c.max_steering_rate);
    out_u = make_double2((double)ua, (double)us);
    out_clf = make_double2(0.0, 0.0);
  } else {
    // "clf" nominal controller (cbf_qp.py:2616-2628, 442-459, Python floats): heading towards the third short-term reference point
    const float2 ref = reinterpret_cast<const float2*>(g.short_term + bi * NS * 2)[2];
    const double desired = atan2((double)ref.y - (double)py, (double)ref.x - (double)px);
    double r = fmod(desired - psi + M_PI, 2.0 * M_PI);  // Python float %: sign of the divisor
    if (r != 0.0 && r < 0.0) r += 2.0 * M_PI;
    const double e_h = r - M_PI, e_v = cc.ref_speed - v;
    out_u = make_double2(clip_d(cc.k_clf_speed * e_v, (double)c.min_acc, (double)c.max_acc),
                             clip_d(cc.k_clf_heading * e_h, -cc.steering_rate_max, cc.steering_rate_max));
    out_clf = make_double2(e_v, e_h);  // CLF rows of the QP (cbf_qp.py:1088-1091): speed error, heading error
  }
  // kbm.ode(None, state, [0, 0]) in float32, dynamics.py:103-111
  const float l_wb_f = (float)((double)c.l_f + (double)c.l_r);
  const float kf = (float)((double)c.l_r / ((double)c.l_f + (double)c.l_r));
  const float td = (float)tan_delta;  // cr_tan
  const double k = cc.l_r / cc.l_wb;
  // the slip angle in float32 (beta_f) and float64, then sin / cos of yaw + slip in both precisions and the float32 cos of the slip angle
  float sb_f, cb_f, cos_beta_f;
  double sin_pb, cos_pb;
  if constexpr (LANES == 1) {
    const float beta_f = cr_atan(kf * td);
    cr_sincos(psi_f + beta_f, sb_f, cb_f);
    cos_beta_f = cr_cos(beta_f);
    const double beta = sigma_atan_f64(k * tan_delta);
    sigma_sincos_f64(psi + beta, &sin_pb, &cos_pb);
  } else {
    // round 2: lane 0 cr_atan(kf * td) = (float) atan((double)(kf * td)), lane 1 atan(k * tan_delta)
    const double r2 = sigma_atan_f64(sub == 1 ? k * tan_delta : (double)(kf * td));
    const float beta_f = (float)dpp_f64<0x00>(r2);
    const double beta = dpp_f64<0x55>(r2);
    // round 3: lane 0 cr_sincos(psi_f + beta_f), lane 1 sincos(psi + beta), lane 2 cr_cos(beta_f)
    double r3s, r3c;
    sigma_sincos_f64(sub == 1 ? psi + beta : (sub == 2 ? (double)beta_f : (double)(psi_f + beta_f)), &r3s, &r3c);
    sb_f = (float)dpp_f64<0x00>(r3s); cb_f = (float)dpp_f64<0x00>(r3c);
    sin_pb = dpp_f64<0x55>(r3s); cos_pb = dpp_f64<0x55>(r3c);
    cos_beta_f = (float)dpp_f64<0xAA>(r3c);
  }
  const float d0 = v_f * cb_f;
  const float d1 = v_f * sb_f;
  const float d2 = (v_f / l_wb_f) * td * cos_beta_f;
  const double dpsi = d2, dx = d0, dy = d1;
  // compute_dstate_2nd_time for u = (0,0), (1,0), (0,1), cbf_qp.py:667-695, 2295-2303
  const double sec_delta_sq = 1.0 / (cos_delta * cos_delta);
  const double tan_beta = k * tan_delta;
  const double cos_beta = 1.0 / sqrt(1.0 + tan_beta * tan_beta);
  const double sin_beta = tan_beta * cos_beta;
  const double kt = k * tan_delta;
  double ddx[3], ddy[3], ddp[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double u1 = (q == 1) ? 1.0 : 0.0, u2 = (q == 2) ? 1.0 : 0.0;
    const double dbeta = (k * sec_delta_sq * u2) / (1.0 + kt * kt);
    ddx[q] = u1 * cos_pb - v * sin_pb * (dpsi + dbeta);
    ddy[q] = u1 * sin_pb + v * cos_pb * (dpsi + dbeta);
    ddp[q] = (u1 / cc.l_wb) * cos_beta * tan_delta + (v / cc.l_wb) * cos_beta * sec_delta_sq * u2 - (v / cc.l_wb) * sin_beta * tan_delta * dbeta;
  }
  // compute_center_state_time_derivatives, cbf_qp.py:697-727 (delta_y = 0: the terms are kept, they evaluate to +-0).  QUAD: again `if (sub < C)` on circle sub, as above
  for (int ci = QUAD ? sub : 0; ci < C; ci += QUAD ? C : 1) {
    const double delta_x = cc.circle_x[ci], delta_y = 0.0;
    Kin kn;
    kn.dx = dx - delta_x * sin_psi * dpsi - delta_y * cos_psi * dpsi;
    kn.dy = dy + delta_x * cos_psi * dpsi - delta_y * sin_psi * dpsi;
    double ax[3], ay[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ax[q] = ddx[q] - delta_x * (sin_psi * ddp[q] + cos_psi * dpsi * dpsi) - delta_y * (cos_psi * ddp[q] - sin_psi * dpsi * dpsi);
      ay[q] = ddy[q] + delta_x * (cos_psi * ddp[q] - sin_psi * dpsi * dpsi) - delta_y * (sin_psi * ddp[q] + cos_psi * dpsi * dpsi);
    }
    kn.ax0 = ax[1] - ax[0]; kn.ax1 = ax[2] - ax[0]; kn.cx = ax[0];
    kn.ay0 = ay[1] - ay[0]; kn.ay1 = ay[2] - ay[0]; kn.cy = ay[0];
    out_kin[ci] = kn;
  }
}
__global__ void __launch_bounds__(256) sigmaenv_cbf_kin_kernel(sigmaenv_config_t c, sigmaenv_cbf_config_t cc, DevBufs g, const float* __restrict__ actions,
                                                               float2* __restrict__ out_cxy, double2* __restrict__ out_u, Kin* __restrict__ out_kin,
                                                               double2* __restrict__ out_clf) {
  sigma_poison_lds();
  const size_t bi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t BN = (size_t)c.n_envs * c.n_agents;
  if (bi >= BN) return;
  double2 u, clf;
  kin_vehicle<1>(c, cc, g, actions, bi, 0, out_cxy + bi * cc.n_circles, u, out_kin + bi * cc.n_circles, clf);
  out_u[bi] = u;
  out_clf[bi] = clf;
}

// ---- kernel B: one workgroup per env -- stencil pseudo distances, margins, reward channels ---------------------------------------------
struct Smem {
  float2* cxy;                 // [N][C] circle centres
  double2* u;                  // [N] nominal action
  Kin* kin;                    // [N][C]
  int* path;                   // [N]
  float* d9;                   // [N*C*2][9] fp16 pseudo distances of the stencil, widened
  double* lane;                // [N*C*2] lane margins, [vehicle][circle][side]
  unsigned long long* vp;      // [N] bits of -vP (>= 0): integer order == value order
  uint8_t* wl;                 // [4 wavefronts][64] uint16: stencil phase, the candidates of a wavefront's stage-2 pass
  // bytes of wl: the four wavefronts' stage-2 candidate lists (64 uint16 each) -- and, after the stencil phase, the list of vehicle pairs whose pair rows / pair margins
  // are evaluated (one uint16 per pair)
  __host__ __device__ static size_t wl_bytes(int N) { const size_t pl = (((size_t)N * (N - 1) / 2) * 2 + 15) & ~(size_t)15; return pl > 512 ? pl : 512; }
  int2* tk;                    // [2 N] per (vehicle, side) task: segments of its boundary, last step's closest segment (stencil_prologue)
  double* vn;                  // margin kernel: [N][4] norm bounds of a vehicle's circle kinematics (pair pass of the pair margins); nullptr in the QP layout
  int* cnt;                    // margin kernel: [4] counters
  // QP kernel: only what its phases read (centre kinematics, centres, path rows); the stencil distances live in the bytes of the Hessian, which is built after
  // the lane rows have consumed them (qp_bytes: 3.5 KB instead of 8.1 KB per env at 16 vehicles x 3 circles -- one more resident workgroup per CU)
  __device__ Smem(char* base, int N, int C, float* d9_elsewhere) {
    kin = reinterpret_cast<Kin*>(base);
    cxy = reinterpret_cast<float2*>(kin + N * C);
    path = reinterpret_cast<int*>(cxy + N * C);
    wl = reinterpret_cast<uint8_t*>(path + N);
    tk = reinterpret_cast<int2*>(wl + wl_bytes(N));
    d9 = d9_elsewhere;
    u = nullptr; lane = nullptr; vp = nullptr; vn = nullptr; cnt = nullptr;
  }
  __host__ __device__ static size_t qp_bytes(int N, int C) { return (size_t)N * C * sizeof(Kin) + (size_t)N * C * 8 + (size_t)N * 4 + wl_bytes(N) + (size_t)N * 16; }
  __device__ Smem(char* base, int N, int C) {
    kin = reinterpret_cast<Kin*>(base);
    u = reinterpret_cast<double2*>(kin + N * C);
    lane = reinterpret_cast<double*>(u + N);
    vp = reinterpret_cast<unsigned long long*>(lane + N * C * 2);
    cxy = reinterpret_cast<float2*>(vp + N);
    d9 = reinterpret_cast<float*>(cxy + N * C);
    vn = reinterpret_cast<double*>(d9 + N * C * 2 * 9);  // (every part up to here is a multiple of 8 bytes)
    cnt = reinterpret_cast<int*>(vn + 4 * N);
    path = cnt + 4;
    wl = reinterpret_cast<uint8_t*>(path + N);
    tk = reinterpret_cast<int2*>(wl + wl_bytes(N));
  }
  __host__ __device__ static size_t bytes(int N, int C) {
    return (size_t)N * C * sizeof(Kin) + (size_t)N * 16 + (size_t)N * C * 2 * 8 + (size_t)N * 8 + (size_t)N * C * 8 + (size_t)N * C * 2 * 9 * 4 + (size_t)N * 4 + wl_bytes(N) + (size_t)N * 16 + (size_t)N * 32 + 16;
  }
};

template <int CTRL> __device__ __forceinline__ float dpp_f32(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true)); }
template <int CTRL> __device__ __forceinline__ unsigned dpp_u32(unsigned x) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true); }

// What the stencil phase needs besides the circle centres, requested by the kernel's prologue (so that the loads overlap the kinematics): per task the boundary's
// segment count and last step's closest segment (the step kernel's own point -> polyline query of the vehicle's centre), and the running minima at +inf.
__device__ __forceinline__ void stencil_prologue(const DevMap& m, const DevBufs& g, const Smem& s, int b, int N, int C) {
  for (int t = (int)(blockDim.x - 1u - threadIdx.x); t < 2 * N; t += blockDim.x) {  // (the workgroup's LAST lanes: the first ones evaluate the kinematics)
    const int i = t >> 1, side = t & 1;
    const int path = g.path[((size_t)b * N + i) * 4];
    s.tk[t] = make_int2(m.n_center[(1 + side) * m.n_paths + path] - 1, g.closest[((size_t)b * N + i) * 3 + 1 + side] - 1);
  }
  unsigned* zmin = reinterpret_cast<unsigned*>(s.d9);
  for (int e = threadIdx.x; e < N * C * 18; e += blockDim.x) zmin[e] = 0x7F800000u;
}

// ---- the 9-point stencil pseudo distances of every (vehicle, circle, side) of the env into s.d9 (shared by the margin and the QP kernel) ----
template <int LPT>
__device__ __forceinline__ void stencil_phase(const sigmaenv_cbf_config_t& cc, const DevMap& m, const Smem& s, const float4* __restrict__ seg4,
                                              const float* __restrict__ segl, int seg_stride, int N, int C, int dbg_skip, unsigned long long* stamps = nullptr) {
#ifdef SIGMAENV_PROFILE
#define ST_STAMP(k) do { if (stamps) stamps[k] = __builtin_readcyclecounter(); } while (0)
#else
#define ST_STAMP(k) do { } while (0)
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  // ---- pseudo distances of the 9-point stencils ------------------------------------------------------------------------------------------
  const float f = (float)cc.fd_step;
  const int n_triples = N * C * 2;
  if (dbg_skip & 1) {
  } else if (m.nch > 0) {
    // Pruned scan in two stages (round 6; until round 5 every lane evaluated all 9 C stencil points against its segment -- a float32 division each -- although a point
    // has a valid projection on one or two segments of a boundary: 90 % of the kernel's vector instructions, profiles/r06_qp_stencil2.txt).
    // LPT lanes take one (vehicle, side) TASK and every lane takes 16 / LPT SEGMENTS of the task's first set.  LPT = 8 (the QP kernel): eight tasks per wavefront
    // pass -- all 2 N tasks of a 16-vehicle env in ONE pass of the workgroup's four wavefronts; LPT = 16 (the margin kernel: lighter on registers, six wavefronts
    // per SIMD): four tasks per pass.
    //   Stage 1 (lane = two segments, loop over the circles): the projection parameter's numerator and denominator of the circle's CENTRE point (the stencil's point 0,
    //   in the reference's own arithmetic) and an interval around them that holds the values of all 9 stencil points: the (segment, circle) pair is a CANDIDATE
    //   unless the interval proves 0 <= lambda < 1 false for every point (the bound is derived at stage1 below).  One to three segments per circle survive.
    //   Stage 2 (lane = candidate, up to 64 per pass): the segment travels from its stage-1 lane by ds_bpermute, the circle's 9 stencil points are evaluated with the
    //   reference's operations (pseudo_distance.py:50-118; nine independent chains per lane) and a valid projection's radicand goes to the point's running minimum in LDS
    //   (ds_min_u32 on the bits of a non-negative float: integer order == value order; a minimum does not depend on the order of its operands: the same bits on every run).
    // First set: the four chunks around last step's closest boundary segment of the vehicle's centre (g.closest: the step kernel's own query, so no search here);
    // then -- the bound of round 5 -- every other chunk whose box is not farther from the task's reference point than U + reach, U the largest of the 9 C minima so far.
    // Exactness: a valid projection (0 <= lambda < 1) lies on the segment, so the pseudo distance of a point to a segment is at least its Euclidean distance to the
    // segment, hence to the bounding box of the segment's chunk (SIGMAENV_CHUNK segments, the boxes of the step kernel's pruned scan), hence at least
    // (distance of the REFERENCE point -- the middle circle's centre -- to the box) - (stencil radius + the largest distance of a circle centre from the reference
    // point).  A chunk farther than U + that reach (+ slack for the float32 rounding of these bounds) cannot lower any of the minima: rounding to fp16 is monotonic,
    // and ties do not change a minimum.  If a point has no valid projection in the first set (U = 1000) every chunk is scanned: WHICH chunks the first set holds
    // changes the work, never the result (a stale or foreign closest index is only slow).
    constexpr int LSH = LPT == 4 ? 2 : (LPT == 8 ? 3 : 4);  // LPT lanes per task: 4 / 8 / 16 -- four / two / one segment of the first set per lane, 16 / 8 / 4 tasks per pass
    constexpr int TP = 64 / LPT;            // tasks per wavefront pass
    constexpr int SPL = 16 / LPT;           // segments per lane in the first set
    constexpr int NBD = 64 / LPT;           // chunk boxes per lane
    constexpr bool BOXES_EARLY = LPT >= 8;  // the box distances are requested with the first set (LPT = 4: sixteen registers per lane -- after stage 2 instead)
    const int tr = lane >> LSH, sl = lane & (LPT - 1);
    const int n_tasks = N * 2;
    unsigned* zmin = reinterpret_cast<unsigned*>(s.d9);  // running minima of the radicands (float bits; +inf from stencil_prologue), then -- in place -- the fp16 pseudo distances
    uint16_t* wl = reinterpret_cast<uint16_t*>(s.wl) + wave * 64;  // the wavefront's candidate list of a stage-2 round: source lane | its segment << 6 | circle << 8
    const int C9 = C * 9;
    // the fp16 pseudo distance of a stencil point from the minimum of its radicands (:115-118, :187-197; a point without a valid projection gets 1000, and
    // 1000 also caps the result because the minimum runs over the invalid segments too)
    auto own_distance = [&](float zs) { return (zs < INFINITY) ? fminf(half_round(sqrtf(zs)), 1000.0f) : 1000.0f; };
    for (int base = wave * TP; base < n_tasks; base += n_waves * TP) {
      const bool active = base + tr < n_tasks;
      const int t = active ? base + tr : base;  // an idle group of lanes mirrors the first one (it takes no segments)
      const int side = t & 1, i = t >> 1;
      const int path = s.path[i];
      const int2 tk = s.tk[t];
      const int nseg = tk.x;
      int kc = tk.y;
      const int nchp = (nseg + SIGMAENV_CHUNK - 1) / SIGMAENV_CHUNK;
      // (32-bit element offsets from the kernel-uniform table pointers: scalar base + vector offset addressing, one register per address)
      const float2* polys = reinterpret_cast<const float2*>(m.left);
      const unsigned poff = ((unsigned)side * (unsigned)m.poly_stride >> 1) + (unsigned)path * (unsigned)m.P;
      const unsigned boff = ((unsigned)path * 3u + 1u + (unsigned)side) * (unsigned)m.nch;
      const unsigned sbase = ((unsigned)path * 2u + (unsigned)side) * (unsigned)seg_stride;
      // first set: four chunks around last step's closest segment of this boundary -- requested first; lane sl takes segments sl, sl + LPT, ... of them
      kc = kc < 0 ? 0 : (kc > nseg - 1 ? nseg - 1 : kc);
      int cs = kc / SIGMAENV_CHUNK - (((kc & (SIGMAENV_CHUNK - 1)) >= SIGMAENV_CHUNK / 2) ? 1 : 2);
      cs = cs + 4 > nchp ? nchp - 4 : cs;
      cs = cs < 0 ? 0 : cs;
      // the lane's segments: point, (cos, sin, m_b, m_t - m_b), length -- seven floats each (m_t is only ever used as the difference)
      bool have[SPL];
      float sx[SPL], sy[SPL], sc_[SPL], ss_[SPL], sm[SPL], sd[SPL], sl2[SPL];
      auto load_segment = [&](int h, int k, bool hv) {
        float2 pb = make_float2(0.f, 0.f);
        float4 t4 = make_float4(1.f, 0.f, 0.f, 0.f);
        float l = 1.0f;
        if (hv) { pb = polys[poff + (unsigned)k]; t4 = seg4[sbase + (unsigned)k]; l = segl[sbase + (unsigned)k]; }
        have[h] = hv; sx[h] = pb.x; sy[h] = pb.y; sc_[h] = t4.x; ss_[h] = t4.y; sm[h] = t4.z; sd[h] = t4.w - t4.z; sl2[h] = l;
      };
#pragma unroll
      for (int h = 0; h < SPL; ++h) {
        const int k = SIGMAENV_CHUNK * cs + sl + LPT * h;
        load_segment(h, k, active && k < nseg);
      }
      // reference point of the task's pruning and the reach of its stencils around it
      const float rx = s.cxy[i * C + (C >> 1)].x, ry = s.cxy[i * C + (C >> 1)].y;
      // squared distances of the reference point to the chunk boxes (lane sl looks at chunks sl, sl + LPT, ...)
      float bd[NBD];
      auto box_distances = [&]() {
#pragma unroll
        for (int j = 0; j < NBD; ++j) {
          const int cidx = sl + LPT * j;
          // (the load only needs the path; unused boxes of the table are empty)
          const float4 bx = (cidx < m.nch) ? m.chunk_box[boff + (unsigned)cidx] : make_float4(1e30f, 1e30f, -1e30f, -1e30f);
          const float ddx = fmaxf(fmaxf(bx.x - rx, rx - bx.z), 0.0f), ddy = fmaxf(fmaxf(bx.y - ry, ry - bx.w), 0.0f);
          bd[j] = ddx * ddx + ddy * ddy;  // squared: only compared (the threshold is squared with slack)
        }
      };
      if (BOXES_EARLY) box_distances();  // requested now, used after the first set
      float2 ctr[SIGMAENV_CBF_MAX_CIRCLES];  // the task's circle centres
      float off2 = 0.0f;
#pragma unroll
      for (int ci = 0; ci < SIGMAENV_CBF_MAX_CIRCLES; ++ci) {
        ctr[ci] = s.cxy[i * C + (ci < C ? ci : 0)];
        const float ox = ctr[ci].x - rx, oy = ctr[ci].y - ry;
        off2 = fmaxf(off2, ox * ox + oy * oy);
      }
      const float reach = f * 1.41422f + 1e-4f + sqrtf(off2) * 1.00001f + 1e-6f;
      unsigned long long rest = 0ull;
      QP_WSYNC();
      ST_STAMP(0);
      for (int pass = 0;; ++pass) {
        // ---- stage 1.  For stencil point q of a circle (offsets in {0, +-f}) against a segment, with u = 2^-24 and M >= every intermediate magnitude:
        //   |vx_q - vx_0| <= f + 3 u M (two roundings for q, one for the centre), |x_q - x_0| and |y_q - y_0| <= (|cos| + |sin|) (f + 3 u M) + 6 u M <= A f + 12 u M,
        //   |num_q - num_0| <= (1 + |m_b|) (A f + 16 u M), |den_q - den_0| <= |m_t - m_b| (A f + 16 u M) + 2 u |l|   (num = x + y m_b, den = l - y (m_t - m_b)).
        // The bounds below use 32 u M (E) where 16 u M is needed; the spare covers the rounding of the bounds themselves and of the comparisons.  lambda = fl(num / den)
        // with den > 0: fl(q) < 1 <=> num < den, and fl(q) >= 0 <=> num >= 0 or -2^-150 < q < 0 -- impossible with num <= -16 u and den < 1e30.  So a pair with
        // den_0 - Dd > 0, den_0 < 1e30 and (num_0 + Dn < 0 or num_0 - Dn >= den_0 + Dd) has NO valid stencil point; everything else (incl. NaN: every comparison
        // false) is a candidate and is decided by the exact evaluation of stage 2.
        unsigned cbits = 0u;  // bit h * 4 + ci: segment h of the lane is a candidate for circle ci
#pragma unroll
        for (int h = 0; h < SPL; ++h) {
          if (h == 0 || pass == 0) {  // (later passes: one segment per lane)
            const float cth = sc_[h], sth = ss_[h], mb = sm[h], dm = sd[h], l = sl2[h];
            const float Af = (fabsf(cth) + fabsf(sth)) * f;
            const float B1 = 1.0f + fabsf(mb), B2 = fabsf(dm);
            const float Mp = (fabsf(sx[h]) + fabsf(sy[h])) + (f + 1.0f);
            const float Dl = fabsf(l) * 2.384185791015625e-07f;  // 2^-22 |l|
#pragma unroll
            for (int ci = 0; ci < SIGMAENV_CBF_MAX_CIRCLES; ++ci) {
              if (ci < C) {
                const float2 cc2 = LPT <= 8 ? ctr[ci] : s.cxy[i * C + ci];  // (LPT = 16: read again, eight registers less)
                const float x0 = cc2.x + 0.0f, y0 = cc2.y + 0.0f;
                const float vx = x0 - sx[h], vy = y0 - sy[h];
                const float x = cth * vx + sth * vy;
                const float y = (-sth) * vx + cth * vy;
                const float num = x + y * mb, den = l - y * dm;
                const float E = (Mp + (fabsf(cc2.x) + fabsf(cc2.y))) * 1.9073486328125e-06f;  // 2^-19 M = 32 u M
                const float D = Af + E;
                const float Dn = B1 * D, Dd = B2 * D + Dl;
                const bool none = (den - Dd > 0.0f) & (den < 1e30f) & ((num + Dn < 0.0f) | (num - Dn >= den + Dd));
                cbits |= (have[h] & !none) ? (1u << (h * 4 + ci)) : 0u;
              }
            }
          }
        }
        if (pass == 0) ST_STAMP(1);
        // ---- stage 2: the wavefront's candidates in (segment, circle, lane) order, 64 per round
        constexpr int NB = SPL * SIGMAENV_CBF_MAX_CIRCLES;
        unsigned long long bms[NB];
        int ncand = 0;
#pragma unroll
        for (int b8 = 0; b8 < NB; ++b8) {
          bms[b8] = ((b8 & 3) < C) ? __ballot((cbits >> b8) & 1u) : 0ull;
          ncand += __popcll(bms[b8]);
        }
        for (int c64 = 0; c64 < ncand; c64 += 64) {
          int run = -c64;
#pragma unroll
          for (int b8 = 0; b8 < NB; ++b8) {
            const int pos = run + (int)__popcll(bms[b8] & ((1ull << lane) - 1ull));
            if (((cbits >> b8) & 1u) && pos >= 0 && pos < 64) wl[pos] = (uint16_t)(lane | (b8 >> 2) << 6 | (b8 & 3) << 8);
            run += __popcll(bms[b8]);
          }
          QP_WSYNC();
          const bool mine = c64 + lane < ncand;
          const unsigned ent = wl[mine ? lane : 0];
          const int src = (int)(ent & 63u), hs = (int)((ent >> 6) & 3u), ci = (int)(ent >> 8);
          const int a4 = src << 2;
#define SIGMA_BPF(v) __int_as_float(__builtin_amdgcn_ds_bpermute(a4, __float_as_int(v)))
          // (a bpermute reads ONE register of the source lane: every segment of the source travels and the destination picks)
          float spx = SIGMA_BPF(sx[0]), spy = SIGMA_BPF(sy[0]), sc = SIGMA_BPF(sc_[0]), ss = SIGMA_BPF(ss_[0]), smb = SIGMA_BPF(sm[0]), sdm = SIGMA_BPF(sd[0]), sl_ = SIGMA_BPF(sl2[0]);
#pragma unroll
          for (int h = 1; h < SPL; ++h) {
            const float bx = SIGMA_BPF(sx[h]), by = SIGMA_BPF(sy[h]), bc = SIGMA_BPF(sc_[h]), bs = SIGMA_BPF(ss_[h]), bm = SIGMA_BPF(sm[h]), bdm = SIGMA_BPF(sd[h]), bl = SIGMA_BPF(sl2[h]);
            const bool pick = hs == h;
            spx = pick ? bx : spx; spy = pick ? by : spy; sc = pick ? bc : sc; ss = pick ? bs : ss; smb = pick ? bm : smb; sdm = pick ? bdm : sdm; sl_ = pick ? bl : sl_;
          }
#undef SIGMA_BPF
          const int ts = base + (src >> LSH), is = ts >> 1;  // the candidate's task (its stage-1 lane's group)
          const float2 cc2 = s.cxy[is * C + ci];
          // query points: agent_pos + offsets in float32 (cbf_qp.py:579-593); each against the segment: pseudo_distance.py:50-118, :188
          const float xp = cc2.x + f, xm = cc2.x + (-f), x0 = cc2.x + 0.0f, yp = cc2.y + f, ym = cc2.y + (-f), y0 = cc2.y + 0.0f;
          const float qx[9] = {x0, xp, x0, xm, x0, xp, xp, xm, xm};
          const float qy[9] = {y0, y0, yp, y0, ym, yp, ym, yp, ym};
          unsigned* zrow = zmin + ((((is * C + ci) << 1) + (ts & 1)) * 9);
#pragma unroll
          for (int q = 0; q < 9; ++q) {  // nine independent chains
            const float vx = qx[q] - spx, vy = qy[q] - spy;              // pseudo_distance.py:63
            const float x = sc * vx + ss * vy;                            // :50-65
            const float y = (-ss) * vx + sc * vy;
            const float lam = (x + y * smb) / (sl_ - y * sdm);            // :106
            const float nx = x - lam * sl_, ny = y - 0.0f;                // :107-112
            const float z = fmaf(ny, ny, nx * nx);                        // :115: the radicand of torch.norm -- the correctly rounded root and the fp16 rounding are
                                                                          // monotonic, so min_k fp16(sqrt(z_k)) = fp16(sqrt(min_k z_k)): the root is taken once per point
            if (mine && (lam >= 0.0f) && (lam < 1.0f)) atomicMin(&zrow[q], __float_as_uint(z));  // :188
          }
          QP_WSYNC();
        }
        if (pass == 0) ST_STAMP(2);
        if (pass == 0) {
          // ---- the bound: U = the largest of the task's 9 C minima (a monotonic map of the largest radicand), then the chunks that may still lower a minimum
          if (!BOXES_EARLY) box_distances();
          float U = 0.0f;
          for (int e = sl; e < C9; e += LPT) {
            const int ci = e / 9, q = e - ci * 9;
            U = fmaxf(U, __uint_as_float(zmin[((((i * C + ci) << 1) + side) * 9) + q]));
          }
          U = fmaxf(U, dpp_f32<0xB1>(U)); U = fmaxf(U, dpp_f32<0x4E>(U));          // over the task's lanes: quad_perm x 2 ...
          if (LPT >= 8) U = fmaxf(U, dpp_f32<0x141>(U));                             // ... row_half_mirror ...
          if (LPT == 16) U = fmaxf(U, dpp_f32<0x140>(U));                            // ... row_mirror
          U = own_distance(U);
          const float thr1 = U + reach;
          const float thr = (U < 1000.0f) ? (thr1 * thr1) * 1.00001f + 1e-9f : INFINITY;  // compared with the squared box distances
          unsigned lo = 0u, hi = 0u;
#pragma unroll
          for (int j = 0; j < NBD; ++j) {
            const int cidx = sl + LPT * j;
            const bool cand = active && cidx < nchp && (cidx < cs || cidx > cs + 3) && !(bd[j] > thr);
            if (cand) { if (cidx < 32) lo |= 1u << cidx; else hi |= 1u << (cidx - 32); }
          }
          lo |= dpp_u32<0xB1>(lo); hi |= dpp_u32<0xB1>(hi); lo |= dpp_u32<0x4E>(lo); hi |= dpp_u32<0x4E>(hi);
          if (LPT >= 8) { lo |= dpp_u32<0x141>(lo); hi |= dpp_u32<0x141>(hi); }
          if (LPT == 16) { lo |= dpp_u32<0x140>(lo); hi |= dpp_u32<0x140>(hi); }
          rest = ((unsigned long long)hi << 32) | lo;
        }
        if (pass == 0) ST_STAMP(3);
        if (!__any(rest != 0ull) || (dbg_skip & 8)) break;
        // ---- next pass: the task's LPT / 4 lowest remaining chunks, one segment per lane
        unsigned long long r2 = rest;
        int cidx = -1;
#pragma unroll
        for (int o = 0; o < LPT / 4; ++o) {
          const int bpos = r2 ? (__ffsll((long long)r2) - 1) : -1;
          if (o == (sl >> 2)) cidx = bpos;
          r2 &= r2 - 1ull;
        }
        rest = r2;
        const int k = SIGMAENV_CHUNK * cidx + (sl & 3);
        load_segment(0, k, cidx >= 0 && k < nseg);
#pragma unroll
        for (int h = 1; h < SPL; ++h) have[h] = false;
      }
      QP_WSYNC();
      ST_STAMP(4);
      {  // radicands -> fp16 pseudo distances, in place: the pass's tasks (TP / 2 vehicles, both sides) are one contiguous stretch of the table
        const int first = (base >> 1) * C * 18, count = min(TP / 2, N - (base >> 1)) * C * 18;
        for (int e = lane; e < count; e += 64) s.d9[first + e] = own_distance(__uint_as_float(zmin[first + e]));
      }
    }
  } else {
    // no chunk boxes (maps beyond the pruning table): one wavefront per triple, lanes over all segments
    for (int t = wave; t < n_triples; t += n_waves) {
      const int side = t & 1, ic = t >> 1, i = ic / C, ci = ic - i * C;
      const int path = s.path[i];
      const int n = m.n_center[(1 + side) * m.n_paths + path];
      const float2* poly = reinterpret_cast<const float2*>(m.left + (size_t)side * m.poly_stride + (size_t)path * m.P * 2);
      const size_t sbase = ((size_t)path * 2 + side) * seg_stride;
      const float cx = s.cxy[i * C + ci].x, cy = s.cxy[i * C + ci].y;
      const float xp = cx + f, xm = cx + (-f), x0 = cx + 0.0f, yp = cy + f, ym = cy + (-f), y0 = cy + 0.0f;
      const float qx[9] = {x0, xp, x0, xm, x0, xp, xp, xm, xm};
      const float qy[9] = {y0, y0, yp, y0, ym, yp, ym, yp, ym};
      float best[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) best[q] = INFINITY;
      for (int k = lane; k + 1 < n; k += 64) {
        const float2 pb = poly[k];
        const float4 t4 = seg4[sbase + k];
        const float l = segl[sbase + k];
        const float cth = t4.x, sth = t4.y, mb = t4.z, mt = t4.w;
        const float dm = mt - mb;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const float vx = qx[q] - pb.x, vy = qy[q] - pb.y;
          const float x = cth * vx + sth * vy;
          const float y = (-sth) * vx + cth * vy;
          const float lam = (x + y * mb) / (l - y * dm);
          const float nx = x - lam * l, ny = y - 0.0f;
          const float d = half_round(norm2(nx, ny));
          const bool ok = (lam >= 0.0f) && (lam < 1.0f);
          const float v = ok ? d : 1000.0f;
          best[q] = (v < best[q]) ? v : best[q];
        }
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        float v = best[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const float o = __shfl_xor(v, off, 64);
          v = (o < v) ? o : v;
        }
        if (lane == 0) s.d9[t * 9 + q] = v;
      }
    }
  }
}

// fp16 finite differences of a stencil (cbf_qp.py:624-665): numpy float16 scalar arithmetic, see the oracle
__device__ __forceinline__ LaneEst lane_estimate(const sigmaenv_cbf_config_t& cc, const float* d) {
  const float hd = half_round((float)cc.fd_step);
  const float hd2 = half_round((float)(cc.fd_step * cc.fd_step));
  const float h4 = half_round((float)(4.0 * cc.fd_step * cc.fd_step));
  const float two_d0 = half_round(2.0f * d[0]);
  LaneEst e;
  e.g0 = half_round(half_round(d[1] - d[0]) / hd);
  e.g1 = half_round(half_round(d[2] - d[0]) / hd);
  e.h00 = half_round(half_round(half_round(d[1] - two_d0) + d[3]) / hd2);
  e.h11 = half_round(half_round(half_round(d[2] - two_d0) + d[4]) / hd2);
  e.h01 = half_round(half_round(half_round(half_round(d[5] - d[6]) - d[7]) + d[8]) / h4);
  e.sm = (double)d[0] - cc.circle_radius;
  return e;
}

__global__ void __launch_bounds__(256, 6) sigmaenv_cbf_kernel(sigmaenv_config_t c, sigmaenv_cbf_config_t cc, DevMap m, DevBufs g, const float4* __restrict__ seg4,
                                                              const float* __restrict__ segl, int seg_stride, const float2* __restrict__ in_cxy,
                                                              const double2* __restrict__ in_u, const Kin* __restrict__ in_kin,
                                                              double* __restrict__ margins, int dbg_skip) {
  sigma_poison_lds();
  extern __shared__ __attribute__((aligned(16))) char cbf_smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = c.n_agents, C = cc.n_circles;
  const size_t BN = (size_t)c.n_envs * N;
  Smem s(cbf_smem, N, C);
  for (int i = tid; i < N * C; i += blockDim.x) {
    s.kin[i] = in_kin[(size_t)b * N * C + i];
    s.cxy[i] = in_cxy[(size_t)b * N * C + i];
  }
  for (int i = tid; i < N; i += blockDim.x) {
    s.u[i] = in_u[(size_t)b * N + i];
    s.path[i] = g.path[((size_t)b * N + i) * 4];
    s.vp[i] = 0ull;
  }
  stencil_prologue(m, g, s, b, N, C);
  __syncthreads();
  const int n_triples = N * C * 2;
  stencil_phase<16>(cc, m, s, seg4, segl, seg_stride, N, C, dbg_skip);
  __syncthreads();
  // ---- fp16 finite differences + lane margins, one lane per triple (cbf_qp.py:624-665, 2634-2686) ---------------------------------
  for (int t = tid; t < n_triples && !(dbg_skip & 2); t += blockDim.x) {
    const int ic = t >> 1, i = ic / C, ci = ic - i * C;
    const LaneEst e = lane_estimate(cc, s.d9 + t * 9);
    const double gm = lane_margin(cc, s.kin[i * C + ci], e, s.u[i].x, s.u[i].y);
    s.lane[t] = gm;
    if (margins) margins[((t & 1) ? BN * C : 0) + ((size_t)b * N + i) * C + ci] = gm;
  }
  // ---- pair margins, one lane per (i < j, ci, cj) (cbf_qp.py:2688-2754) -------------------------------------------------------------
  {
    const double d_safe = 2.0 * cc.circle_radius + cc.safety_buffer, d_safe_sq = d_safe * d_safe;
    const int CC = C * C, n_pairs = N * (N - 1) / 2, n_items = n_pairs * CC;
    double* mP = margins ? margins + 2 * BN * C : nullptr;
    auto pair_item = [&](int i, int j, int cc2) {
      const int ci = cc2 / C, cj = cc2 - ci * C;
      const float dxf = s.cxy[i * C + ci].x - s.cxy[j * C + cj].x, dyf = s.cxy[i * C + ci].y - s.cxy[j * C + cj].y;  // float32 tensor difference (:2706)
      const double gm = pair_margin(cc, s.kin[i * C + ci], s.kin[j * C + cj], dxf, dyf, d_safe_sq, s.u[i].x, s.u[i].y, s.u[j].x, s.u[j].y);
      if (mP) mP[((((size_t)b * N + i) * N + j) * C + ci) * C + cj] = gm;
      if (gm < 0.0) {  // min(float(g), 0.0): a NaN margin counts as 0 (:2791)
        const unsigned long long bits = (unsigned long long)__double_as_longlong(-gm);
        atomicMax(&s.vp[i], bits);
        atomicMax(&s.vp[j], bits);
      }
    };
    // Only NEGATIVE pair margins reach the reward channel.  When the margins themselves are not asked for, a PAIR of vehicles is tested first (round 6; the same bound as
    // the QP kernel's candidate flags): with V, A0, A1, Cc the largest norms of a vehicle's circle velocities / control columns / drift accelerations, u its nominal controls
    // and dmin, dmax the extreme distances between the two vehicles' circle centres, every one of the pair's C^2 margins is at least
    //   lambda (dmin^2 - d_safe^2) - dmax (2 dt (V_i + V_j) + dt^2 (Cc_i + Cc_j) + dt^2 (A0_i |u_i0| + A1_i |u_i1| + A0_j |u_j0| + A1_j |u_j1|))      (lambda >= 0);
    // a pair whose bound exceeds 1e-9 has no negative margin and is not evaluated (NaN / inf keep the pair): all but the handful of pairs within ~0.7 m of each other.
    const bool by_pairs = !mP && N <= 255 && cc.lambda_ttcbf >= 0.0 && !(dbg_skip & (4 | 1024));
    if (by_pairs) {
      for (int i = (int)blockDim.x - 1 - tid; i < N; i += blockDim.x) {  // (the last lanes: the first ones have the lane margins above)
        double m4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int ci = 0; ci < C; ++ci) {
          const Kin& k = s.kin[i * C + ci];
          const double v4[4] = {k.dx * k.dx + k.dy * k.dy, k.ax0 * k.ax0 + k.ay0 * k.ay0, k.ax1 * k.ax1 + k.ay1 * k.ay1, k.cx * k.cx + k.cy * k.cy};
#pragma unroll
          for (int e = 0; e < 4; ++e) m4[e] = (v4[e] > m4[e] || v4[e] != v4[e]) ? v4[e] : m4[e];  // (a NaN stays)
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s.vn[4 * i + e] = (double)(__builtin_amdgcn_sqrtf((float)m4[e] * 1.000001f) * 1.000001f);  // (upper bounds; overflow -> inf: the pair is kept)
      }
      if (tid == 0) s.cnt[0] = 0;
      __syncthreads();
      uint16_t* plist = reinterpret_cast<uint16_t*>(s.wl);  // (the stencil phase's candidate lists, free now: Smem::wl_bytes holds every pair)
      const double dt = cc.dt_taylor;
      const int lane = tid & 63;
      for (int p0 = 0; p0 < n_pairs; p0 += blockDim.x) {
        int q = p0 + tid;
        bool keep = false;
        int i = 0, j = 1;
        if (q < n_pairs) {
          while (q >= N - 1 - i) { q -= N - 1 - i; ++i; }
          j = i + 1 + q;
          float dmin2 = INFINITY, dmax2 = 0.0f;
          bool bad = false;
          for (int ci = 0; ci < C; ++ci)
            for (int cj = 0; cj < C; ++cj) {
              const float dx = s.cxy[i * C + ci].x - s.cxy[j * C + cj].x, dy = s.cxy[i * C + ci].y - s.cxy[j * C + cj].y;
              const float d2 = dx * dx + dy * dy;  // (<= 3 roundings: 1e-6 of slack each way below)
              bad |= !(d2 == d2);
              dmin2 = d2 < dmin2 ? d2 : dmin2;
              dmax2 = d2 > dmax2 ? d2 : dmax2;
            }
          const double* vi = s.vn + 4 * i;
          const double* vj = s.vn + 4 * j;
          const double K = 2.0 * dt * (vi[0] + vj[0]) + (dt * dt) * (vi[3] + vj[3])
                           + (dt * dt) * (vi[1] * fabs(s.u[i].x) + vi[2] * fabs(s.u[i].y) + vj[1] * fabs(s.u[j].x) + vj[2] * fabs(s.u[j].y));
          const double LB = cc.lambda_ttcbf * ((double)dmin2 * (1.0 - 1e-6) - d_safe_sq) - (double)(__builtin_amdgcn_sqrtf(dmax2 * 1.000001f) * 1.000001f) * K * (1.0 + 1e-12);
          keep = bad || !(LB > 1e-9);
        }
        const unsigned long long bm = __ballot(keep);
        if (bm != 0ull) {  // (wavefront-uniform)
          int pos0 = 0;
          if (lane == 0) pos0 = atomicAdd(&s.cnt[0], (int)__popcll(bm));
          pos0 = __builtin_amdgcn_readfirstlane(pos0);
          if (keep) plist[pos0 + (int)__popcll(bm & ((1ull << lane) - 1ull))] = (uint16_t)(i | j << 8);
        }
      }
      __syncthreads();
      const int n_rows = s.cnt[0] * CC;
      for (int k = tid; k < n_rows; k += blockDim.x) {
        const int pl = k / CC;
        const unsigned ij = plist[pl];
        pair_item((int)(ij & 0xFFu), (int)(ij >> 8), k - pl * CC);
      }
    } else {
      for (int p = tid; p < n_items && !(dbg_skip & 4); p += blockDim.x) {
        int q = p / CC;
        const int cc2 = p - q * CC;
        int i = 0;
        while (q >= N - 1 - i) { q -= N - 1 - i; ++i; }
        pair_item(i, i + 1 + q, cc2);
      }
    }
  }
  __syncthreads();
  // ---- the three reward channels (cbf_qp.py:2762-2804, written like :2552-2560) ------------------------------------------------------
  for (int i = tid; i < N; i += blockDim.x) {
    const size_t bi = (size_t)b * N + i;
    double vL = INFINITY, vR = INFINITY;
    bool nanL = false, nanR = false;
    for (int ci = 0; ci < C; ++ci) {
      const double gl = s.lane[(i * C + ci) * 2], gr = s.lane[(i * C + ci) * 2 + 1];
      nanL |= (gl != gl); nanR |= (gr != gr);
      vL = (gl < vL) ? gl : vL;
      vR = (gr < vR) ? gr : vR;
    }
    if (nanL) vL = NAN;  // np.min propagates NaN
    if (nanR) vR = NAN;
    const double vP = -__longlong_as_double((long long)s.vp[i]);
    g.reward_info[5 * BN + bi] = (float)clip_d(vL / cc.h_nom, -1.0, 0.0);
    g.reward_info[6 * BN + bi] = (float)clip_d(vR / cc.h_nom, -1.0, 0.0);
    g.reward_info[4 * BN + bi] = (float)clip_d(vP / cc.h_nom, -1.0, 0.0);
  }
}

// ---- kernel C: the centralized CBF-QP of an env (cbf_qp.py:733-1400), one workgroup per env -----------------------------------------------
// Same data as the margin kernel (stencils -> lane rows; pair rows recomputed from the kinematics on every evaluation, and only the
// CANDIDATE ones: rows whose box bound says they cannot become active are dropped before the iterations start).  Every slack and lambda
// is eliminated in closed form (qp_phi), the remaining convex piecewise quadratic problem in the n = 2N controls is solved by a projected
// Newton method ON ONE WAVEFRONT (env b: wavefront b mod n; the others leave after the stencil / candidate phases): in registers for envs with no
// or few candidate rows (qp_newton_registers), else rows over the lanes (LDS float64 atomics for gradient / Hessian: the full layout only), the
// coupled vehicles' compacted system factorised with row k in the registers of lane k, Armijo search
// along the projection arc with a projected-gradient acceptance once the decrease of F is below its rounding noise -- the algorithm of
// oracle/sigmaenv_cbf_oracle.inc (qp_solve).  The candidate list is compacted in row order and a single wavefront's LDS atomics execute in
// program / lane order, so repeated launches return the same bits (tests/test_gpu_cbf.py::test_cbf_qp_is_bitwise_repeatable).
#ifndef QP_STENCIL_LPT
#define QP_STENCIL_LPT 8  /* lanes per stencil task of the QP kernels (4: sixteen tasks per wavefront pass -- measured: 85 spilled registers, 2.8e8 against 4.3e8) */
#endif
#ifndef QP_LEAN_THREADS
#define QP_LEAN_THREADS 128  /* threads per env of the LEAN instantiation: two wavefronts (64: 4.08e8, 128: 4.26e8, 256: 3.83e8 agent-env-steps/s in bench.py --cbf-qp, profiles/r06_qp_lds.txt) */
#endif
constexpr int QP_SMALL_AGENTS = 32;  // up to here: the 2N x 2N Hessian and the candidate list live in LDS as written below (QpSmemT<false>)
constexpr int QP_MAX_AGENTS = 64;    // 33 .. 64 vehicles: QpSmemT<true> -- the Hessian as a packed lower triangle (66 KB at 64 vehicles), the candidate list in HBM

// stop test after a vanishing step: the strict tolerance pg_tol = 1e-6 (1 + |F|), loosened to the ABSOLUTE 1e-4 where that is more (oracle: qp_vanish_tol)
__device__ __forceinline__ double qp_vanish_tol(double pg_tol) { return pg_tol > 1e-4 ? pg_tol : 1e-4; }
// min over 0 <= lambda <= 1, s >= 0, g + h lambda + s >= 0 of ws s^2 + wl lambda^2; first and second derivative in g
__device__ __forceinline__ double qp_phi(double g, double h, double ws, double wl, double& d1, double& d2) {
  d1 = 0.0; d2 = 0.0;
  if (wl <= 0.0) {
    const double t = g + (h > 0.0 ? h : 0.0);
    if (!(t < 0.0)) return 0.0;
    d1 = 2.0 * ws * t; d2 = 2.0 * ws;
    return ws * t * t;
  }
  if (!(g < 0.0)) return 0.0;
  const double d = -g;
  if (h <= 0.0) { d1 = -2.0 * ws * d; d2 = 2.0 * ws; return ws * d * d; }
  const double D = ws * h * h + wl;
  if (ws * h * d <= D) { d1 = -2.0 * ws * wl * d / D; d2 = 2.0 * ws * wl / D; return ws * wl * d * d / D; }
  const double r = d - h;
  d1 = -2.0 * ws * r; d2 = 2.0 * ws;
  return wl + ws * r * r;
}

// LEAN (round 6; the instantiation that solves nearly every env of up to QP_SMALL_AGENTS vehicles): only what the register path of the Newton iteration touches --
// no full Hessian (a 16 x 16 compact system and its factor instead), no gradient / bound vectors, 64 candidate entries, the lane rows in the bytes of the stencil
// distances they are computed from: 12 KB instead of 23 KB per env at 16 vehicles x 3 circles, 13 resident envs per CU instead of 7.  An env the register path
// cannot take (more than 64 candidate rows or more than 8 vehicles in them) is flagged and solved from scratch by the full-layout instantiation in a launch that
// follows (sigmaenv_cbf_qp): the resident env count, not the instruction issue, bounds this kernel (profiles/r06_qp_lds.txt).
template <bool BIG, bool LEAN = false>
struct QpSmemT {
  static_assert(!(BIG && LEAN), "the lean layout is for up to QP_SMALL_AGENTS vehicles");
  static constexpr bool FULL_SMALL = !BIG && !LEAN;  // the instantiation sigmaenv_cbf_qp_deferred_kernel runs
  typedef typename std::conditional<BIG, uint32_t, uint16_t>::type cand_t;
  static constexpr int KIND_SHIFT = BIG ? 30 : 14;           // candidate entry: pair-row index | kind << KIND_SHIFT
  static constexpr uint32_t ROW_MASK = (1u << KIND_SHIFT) - 1u;
  double4* lc;      // [N*C*2] lane rows: A0, A1, b0, h (ttcbf_lane_affine_coeffs, adaptive branch cbf_qp.py:2341-2369)
  double* H;        // [n*n] Hessian, factorised in place
  double *grad, *gn, *p, *u, *un, *lo, *hi, *unom, *clf_e, *clf_v;  // [n] each
  double* sc;       // scalars: 0 F, 1 Fn, 2 dec, 3 step, 4 pg0, 5 pgn
  uint16_t* pij;    // [N(N-1)/2] i | j << 8
  uint8_t* cmap;    // [n] compact unknown -> original index (coupled vehicles only)
  int* coupled;     // [N] vehicle has an active pair row in the current Hessian
  int* sci;         // [4] integer scalars: 0 number of candidate pair rows
  float2* sv;       // [N] speed and steering angle of every vehicle (read with the rest of the input; used when the safe action is written)
  cand_t* cand;     // [2 N(N-1)/2 C^2] candidate pair rows: row index | kind << KIND_SHIFT (0: both vehicles; grouped QPs, cross-group pair: 1 the
                    // row of the lower-numbered vehicle's group problem, 2 the one of the higher-numbered vehicle's)
  uint8_t* grp;     // [N] group of every vehicle (grouped QPs)
  // entry (r, c) of the symmetric Hessian: the full n x n array, or (BIG) the packed lower triangle -- every access goes through here
  __host__ __device__ static int hix(int r, int c, int n) {
    if (!BIG) return r * n + c;
    const int hi = r > c ? r : c, lo = r > c ? c : r;
    return hi * (hi + 1) / 2 + lo;
  }
  static constexpr int LEAN_CAND = 64;  // candidate entries of the lean layout (one lane per candidate row in qp_newton_registers)
  __device__ QpSmemT(char* base, int N, int C, cand_t* cand_hbm) {
    const int n = 2 * N;
    lc = reinterpret_cast<double4*>(base);
    if (LEAN) {
      H = reinterpret_cast<double*>(base + (size_t)N * C * 2 * 36);  // (the stencil distances -- 9 floats per lane row -- start where the lane rows do: see the kernel's lane-row phase)
      gn = H + hwords(N, C); p = gn + n; u = p + n; un = u + n; unom = un + n; clf_e = unom + n; clf_v = clf_e + n;
      grad = lo = hi = nullptr;
      sc = clf_v + n;
      sci = reinterpret_cast<int*>(sc + 8);
      sv = reinterpret_cast<float2*>(sci + 4);
      coupled = reinterpret_cast<int*>(sv + N);
      pij = reinterpret_cast<uint16_t*>(coupled + N);
      uint16_t* after = pij + ((N * (N - 1) / 2 + 3) & ~3);
      cand = reinterpret_cast<cand_t*>(after);
      cmap = reinterpret_cast<uint8_t*>(after + LEAN_CAND);
      grp = cmap + n;
      return;
    }
    H = reinterpret_cast<double*>(lc + N * C * 2);
    grad = H + hwords(N, C); gn = grad + n; p = gn + n; u = p + n; un = u + n; lo = un + n; hi = lo + n; unom = hi + n; clf_e = unom + n; clf_v = clf_e + n;
    sc = clf_v + n;
    sci = reinterpret_cast<int*>(sc + 8);
    sv = reinterpret_cast<float2*>(sci + 4);
    coupled = reinterpret_cast<int*>(sv + N);
    pij = reinterpret_cast<uint16_t*>(coupled + N);
    uint16_t* after = pij + ((N * (N - 1) / 2 + 3) & ~3);
    if (BIG) {
      cand = cand_hbm;
      cmap = reinterpret_cast<uint8_t*>(after);
    } else {
      cand = reinterpret_cast<cand_t*>(after);
      cmap = reinterpret_cast<uint8_t*>(after + ((N * (N - 1) * C * C + 3) & ~3));
    }
    grp = cmap + n;
  }
  // the Hessian's area also receives the Cholesky factor of the compacted Newton system with row stride 8 / 16 / 32 (qp_newton_direction<S>):
  // it must hold S x S entries for the S the unknown count n can select, not only n x n
  __host__ __device__ static int hdim(int n) { return n <= 8 ? 8 : (n <= 16 ? 16 : (n <= 32 ? 32 : n)); }
  // doubles of the Hessian's area: S x S entries, and at least the stencil distances it holds before the first evaluation (N C 2 x 9 floats, see Smem)
  // (BIG: the packed triangle, the 32 x 32 factor of the compacted system, the stencil distances and the candidate flags -- one byte per pair row -- share the area)
  __host__ __device__ static size_t hwords(int N, int C) {
    if (LEAN) {  // the 16 x 16 compact system (and its factor, row stride 16) of qp_newton_registers; before that the candidate flags, one byte per pair row
      const size_t fl = ((size_t)N * (N - 1) / 2 * C * C + 7) / 8;
      return fl > 256 ? fl : 256;
    }
    const size_t n = 2 * (size_t)N;
    const size_t hh = BIG ? n * (n + 1) / 2 : (size_t)hdim(2 * N) * hdim(2 * N), d9 = ((size_t)N * C * 2 * 9 + 1) / 2;
    size_t w = hh > d9 ? hh : d9;
    if (BIG) {
      const size_t fl = ((size_t)N * (N - 1) / 2 * C * C + 7) / 8;
      w = w > 1024 ? w : 1024;
      w = w > fl ? w : fl;
    }
    return w;
  }
  __host__ __device__ static size_t cand_entries(int N, int C) { return (size_t)N * (N - 1) * C * C; }  // both one-sided rows of every pair row
  __host__ __device__ static size_t bytes(int N, int C) {
    const size_t n = 2 * (size_t)N;
    if (LEAN) return (size_t)N * C * 2 * 36 + hwords(N, C) * 8 + 7 * n * 8 + 64 + 16 + (size_t)N * 8 + (size_t)N * 4 + ((size_t)N * (N - 1) / 2 + 4) * 2 + LEAN_CAND * 2 + n + N + 16;
    return (size_t)N * C * 2 * 32 + hwords(N, C) * 8 + 10 * n * 8 + 64 + 16 + (size_t)N * 8 + (size_t)N * 4 + ((size_t)N * (N - 1) / 2 + 4) * 2 + (BIG ? 0 : (cand_entries(N, C) + 4) * 2) + n + N + 16;
  }
};
typedef QpSmemT<false> QpSmem;

// coefficients of pair row pr = ((i < j) pair, ci, cj): ttcbf_pair_affine_coeffs, adaptive branch (cbf_qp.py:2406-2447), from the centre kinematics
template <class Q>
__device__ __forceinline__ void qp_pair_row(const sigmaenv_cbf_config_t& cc, const Smem& s, const Q& q, int C, int pr, int idx[4], double a[4], double& b0,
                                            double& h) {
  const int CC = C * C, pq = pr / CC, c2 = pr - pq * CC, ci = c2 / C, cj = c2 - ci * C;
  const unsigned ij = q.pij[pq];
  const int i = (int)(ij & 0xFFu), j = (int)(ij >> 8);
  const Kin& ki = s.kin[i * C + ci];
  const Kin& kj = s.kin[j * C + cj];
  const double d_safe = 2.0 * cc.circle_radius + cc.safety_buffer, d_safe_sq = d_safe * d_safe;
  const double dt = cc.dt_taylor;
  const double dx = (double)(s.cxy[i * C + ci].x - s.cxy[j * C + cj].x), dy = (double)(s.cxy[i * C + ci].y - s.cxy[j * C + cj].y);
  const double vrel_x = ki.dx - kj.dx, vrel_y = ki.dy - kj.dy;
  h = dx * dx + dy * dy - d_safe_sq;
  const double dh = 2.0 * (dx * vrel_x + dy * vrel_y);
  const double f = 0.5 * (dt * dt) * 2.0, fm = 0.5 * (dt * dt) * -2.0;
  a[0] = f * (dx * ki.ax0 + dy * ki.ay0); a[1] = f * (dx * ki.ax1 + dy * ki.ay1);
  a[2] = fm * (dx * kj.ax0 + dy * kj.ay0); a[3] = fm * (dx * kj.ax1 + dy * kj.ay1);
  const double const_ddh = 2.0 * (vrel_x * vrel_x + vrel_y * vrel_y) + 2.0 * (dx * (ki.cx - kj.cx) + dy * (ki.cy - kj.cy));
  b0 = dh * dt + 0.5 * (dt * dt) * const_ddh;
  idx[0] = 2 * i; idx[1] = 2 * i + 1; idx[2] = 2 * j; idx[3] = 2 * j + 1;
}


// F(u) (returned through q.sc[slot]); gradient into gout; Hessian into q.H when with_H.  Called by ONE wavefront; ends with a wavefront sync.
template <class Q, bool BIG>
__device__ inline void qp_eval(const sigmaenv_cbf_config_t& cc, const Smem& s, const Q& q, int N, int C, const double* __restrict__ uv, double* gout,
                               bool with_H, int slot) {
  const int tid = threadIdx.x & 63, n = 2 * N;  // ONE wavefront evaluates (the Newton phase of the kernel runs on wavefront 0 alone)
  for (int k = tid; k < n; k += 64) gout[k] = 0.0;
  if (with_H) {
    {  // (n * n is even; the packed triangle's n (n + 1) / 2 = N (2 N + 1) is ODD for an odd vehicle count: its last word -- the last unknown's diagonal entry -- was
       //  never cleared and kept accumulating over the evaluations until tools/fuzz_cbf.py --cpm-agents 48 met N = 41)
      double2* H2 = reinterpret_cast<double2*>(q.H);
      const int words = BIG ? n * (n + 1) / 2 : n * n;
      for (int k = tid; k < words / 2; k += 64) H2[k] = make_double2(0.0, 0.0);
      if ((words & 1) && tid == 0) q.H[words - 1] = 0.0;
    }
    for (int k = tid; k < N; k += 64) q.coupled[k] = 0;
  }
  if (tid == 0) q.sc[slot] = 0.0;
  QP_WSYNC();
  double Fp = 0.0;
  for (int k = tid; k < n; k += 64) {  // tracking cost and CLF hinges (cbf_qp.py:914-920, 784-791)
    const double wk = (k & 1) ? cc.qp_w_steer : cc.qp_w_acc, t = (uv[k] - q.unom[k]) * wk;
    Fp += t * t;
    double gk = 2.0 * wk * t, hk = 2.0 * wk * wk;
    const double cv = q.clf_v[k] - q.clf_e[k] * uv[k];
    if (cv > 0.0) {
      Fp += cc.qp_w_clf * cv * cv;
      gk += -2.0 * cc.qp_w_clf * q.clf_e[k] * cv;
      hk += 2.0 * cc.qp_w_clf * q.clf_e[k] * q.clf_e[k];
    }
    atomicAdd(&gout[k], gk);
    if (with_H) atomicAdd(&q.H[Q::hix(k, k, n)], hk);
  }
  // lane rows, then the CANDIDATE pair rows (q.cand: the rows that can be active somewhere in the box, see the kernel)
  const int n_lane = N * C * 2, n_con = n_lane + q.sci[0];
  for (int r = tid; r < n_con; r += 64) {
    int idx[4];
    double a[4], b0, h, w, wl = cc.qp_w_lambda;
    int m;
    if (r < n_lane) {
      const int i = (r >> 1) / C;
      const double4 l4 = q.lc[r];
      idx[0] = 2 * i; idx[1] = 2 * i + 1; idx[2] = idx[3] = 0;
      a[0] = l4.x; a[1] = l4.y; a[2] = a[3] = 0.0; b0 = l4.z; h = l4.w; w = cc.qp_w_lane; m = 2;
    } else {
      const unsigned ce = q.cand[r - n_lane];
      const int kind = (int)(ce >> Q::KIND_SHIFT);
      qp_pair_row(cc, s, q, C, (int)(ce & Q::ROW_MASK), idx, a, b0, h);
      w = cc.qp_w_pair; m = 4;
      if (kind != 0) {
        // cross-group row (ttcbf_pair_affine_coeffs_cross, cbf_qp.py:2491-2532): the vehicle's own half of the pair row -- called with the
        // roles swapped for the higher-numbered vehicle, dx, dy, the relative velocity and c_i - c_j all change sign, which gives exactly
        // (A_j, b0, h) of the pair row -- in the constraint A u + b0 / 2 + rs h lambda >= -s (:1747-1758), lambda always penalised (:1789-1791)
        if (kind == 2) { idx[0] = idx[2]; idx[1] = idx[3]; a[0] = a[2]; a[1] = a[3]; }
        b0 = 0.5 * b0; h = cc.rs * h; w = cc.qp_w_cross; wl = cc.qp_w_lambda_cross; m = 2;
      }
    }
    double g = b0;
    for (int k = 0; k < m; ++k) g += a[k] * uv[idx[k]];
    double d1, d2;
    Fp += qp_phi(g, h, w, wl, d1, d2);
    if (d2 != 0.0) {
      for (int k = 0; k < m; ++k) atomicAdd(&gout[idx[k]], d1 * a[k]);
      if (with_H) {
        for (int k = 0; k < m; ++k)
          for (int l = 0; l < m; ++l)
            if (!BIG || idx[l] <= idx[k]) atomicAdd(&q.H[Q::hix(idx[k], idx[l], n)], d2 * a[k] * a[l]);  // (the packed triangle holds each symmetric pair once)
        if (m == 4) { q.coupled[idx[0] >> 1] = 1; q.coupled[idx[2] >> 1] = 1; }  // off-diagonal blocks: the two vehicles are coupled
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) Fp += __shfl_xor(Fp, off, 64);
  if (tid == 0) q.sc[slot] += Fp;
  QP_WSYNC();
}

// Cholesky factorisation and both triangular solves of the n x n Newton system for n <= 32 by ONE wavefront with row k of the matrix in
// the registers of lane k: pivots and column entries travel by v_readlane (all indices are compile-time constants after unrolling), no
// LDS round trips and no barriers in the O(n^3) part.  Rows / columns >= n are padded with the identity.
// the lane's index in its wavefront from the execution mask (all lanes active where it is used): two instructions, and the work-item id register need not stay
// alive (or spilled) through the solve
__device__ __forceinline__ int qp_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ double qp_bcast(double x, int l) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_readlane(lo, l);
  hi = __builtin_amdgcn_readlane(hi, l);
  return __hiloint2double(hi, lo);
}
// The Newton system restricted to the COUPLED vehicles (those with an active pair row: off-diagonal blocks in H), compacted to m = 2 x
// (coupled vehicles) unknowns and padded with the identity to S in {8, 16, 32}: vehicles without an active pair row have an independent
// 2 x 2 block that their own lane solves in closed form (the common case: most vehicles, most steps).  cmap[r]: original index of compact
// unknown r.  The factor's rows go to LDS in compact layout (stride S) for the back substitution.
template <int S, bool BIG>
__device__ __noinline__ void qp_newton_direction(double* __restrict__ H, double* __restrict__ p, const uint8_t* __restrict__ cmap, int n, int m) {
#pragma clang fp contract(fast)  // a linear solve, not a parity-pinned formula: fused multiply-adds are welcome here
  const int k = qp_lane();
  const int mk = (k < m) ? (int)cmap[k] : 0;
  double r[S];
#pragma unroll
  for (int l = 0; l < S; ++l) r[l] = (k < m && l < m) ? H[QpSmemT<BIG>::hix(mk, (int)cmap[l], n)] : ((k == l) ? 1.0 : 0.0);
  double rhs = (k < m) ? p[mk] : 0.0;
  double inv_own = 1.0;  // 1 / L[k][k]: one reciprocal square root per column instead of a square root and three divisions
#pragma unroll
  for (int col = 0; col < S; ++col) {
    const double pv = qp_bcast(r[col], col);
    const double inv = rsqrt(pv);
    if (k == col) { r[col] = pv * inv; inv_own = inv; }
    else if (k > col) r[col] = r[col] * inv;
#pragma unroll
    for (int l = col + 1; l < S; ++l) {
      const double llc = qp_bcast(r[col], l);
      r[l] -= r[col] * llc;  // (lanes k < l update entries of the upper triangle, which nothing reads)
    }
  }
#pragma unroll
  for (int col = 0; col < S; ++col) {  // L y = rhs
    const double y = qp_bcast(rhs, col) * qp_bcast(inv_own, col);
    if (k == col) rhs = y;
    else if (k > col) rhs -= r[col] * y;
  }
  if (k < m) {  // L^T x = y needs the columns of L: through LDS (row k written by lane k, element k of row col read by lane k)
#pragma unroll
    for (int l = 0; l < S; ++l) if (l <= k) H[k * S + l] = r[l];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int col = S - 1; col >= 0; --col) {
    if (col < m) {
      const double x = qp_bcast(rhs, col) * qp_bcast(inv_own, col);
      if (k == col) rhs = x;
      else if (k < col) rhs -= H[col * S + k] * x;
    }
  }
  if (k < m) p[mk] = rhs;
}

// ---- the Newton iterations in registers: envs with no or few candidate pair rows ------------------------------------------------------
// Without candidate pair rows (the usual case: profiles/r05_qp_stencil.txt) the Hessian is block diagonal with one 2 x 2 block per vehicle
// for every iterate; with a few, only the vehicles of those rows are coupled.  The same iteration as the general one below (same held set, same
// Armijo rule, ONE step length for the whole problem, same stopping tests), but every vehicle's unknowns, gradient and Hessian block stay in
// the registers of the vehicle's lanes: what crosses lanes are the sums and maxima the step-length rule needs, by DPP.  The candidate pair
// rows -- one per lane, coefficients in registers for the whole solve -- read the trial point from LDS and add their terms to a COMPACT
// gradient / Hessian over the vehicles they touch (at most 8), which those vehicles add to their registers and which, completed with
// their own blocks, is the Newton system qp_newton_direction factorises; every other vehicle solves its 2 x 2 system in closed form.
// Lanes: vehicle v owns LPV = 4 / 2 / 1 adjacent lanes (N <= 16 / 32 / 64), which share its 2 C lane rows.
__device__ __forceinline__ double qp_uniform(double x) {  // a wavefront-uniform value, moved to scalar registers (the vector registers are the scarce ones here)
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
__device__ __forceinline__ double qp_wave_sum(double x) {  // (fixed order: the same value on every run and in every lane)
  x += dpp_f64<0xB1>(x); x += dpp_f64<0x4E>(x); x += dpp_f64<0x141>(x); x += dpp_f64<0x140>(x);  // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
  return qp_uniform(((qp_bcast(x, 0) + qp_bcast(x, 16)) + qp_bcast(x, 32)) + qp_bcast(x, 48));
}
__device__ __forceinline__ double qp_wave_max(double x) {
  x = fmax(x, dpp_f64<0xB1>(x)); x = fmax(x, dpp_f64<0x4E>(x)); x = fmax(x, dpp_f64<0x141>(x)); x = fmax(x, dpp_f64<0x140>(x));
  return qp_uniform(fmax(fmax(qp_bcast(x, 0), qp_bcast(x, 16)), fmax(qp_bcast(x, 32), qp_bcast(x, 48))));
}
struct __attribute__((aligned(16))) QpCand { double a[4], b0, h; int k0, k2, pad[2]; };  // a candidate pair row: coefficients; first unknown | compact index << 8 (| unknowns << 16) of its vehicle(s)
static_assert(sizeof(QpCand) == sizeof(Kin), "the candidate rows take the place of the centre kinematics");
struct QpBlock { double F, g0, g1, h00, h01, h11; };  // F: of the whole problem; the rest: the vehicle's
template <int RMAX, bool VOPAQUE = false>
struct QpVehicle {
  const double4* rows;  // the vehicle's lane rows (A0, A1, b0, h) in LDS: the lane takes rows sub, sub + LPV, ...; a row it does not have counts as (0, 0, 1, 0), whose phi is 0 everywhere
  int sub, sh, n_rows;  // lane within the vehicle, log2 LPV, 2 C (0 for a lane without a vehicle)
  const double *unom, *clf_e, *clf_v;  // LDS, by unknown
  double lo0, hi0, lo1, hi1;
  int nrl, lpv;         // rows per lane, lanes per vehicle
  int v2;               // 2 x vehicle: its first unknown
  bool lead;            // first lane of a vehicle that exists: the lane whose per-unknown terms count
  // candidate pair rows: lane c < n_cand evaluates row c
  int n_cand, nc2;      // candidate rows; unknowns of the compact system (2 x vehicles of candidate rows)
  const QpCand* cand;   // LDS: the rows' coefficients, computed once per solve
  int pos2;             // the vehicle's first unknown in the compact system, -1: not in it
  double *xu, *gc, *Hc; // LDS: the point being evaluated (by unknown); compact gradient and Hessian (row stride nc2) of the candidate rows
  __device__ __forceinline__ void eval(const sigmaenv_cbf_config_t& cc, double u0, double u1, QpBlock& e) const {
    double Fp = 0.0, g0 = 0.0, g1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0;
    // (the lane's offsets are re-derived per evaluation: hoisted out of the solve, the LDS addresses built from them were eight spilled registers -- one add each)
    int v2 = this->v2, sub = this->sub;
    asm volatile("" : "+v"(v2), "+v"(sub));
    if (n_cand > 0) {
      if (lead) { xu[v2] = u0; xu[v2 + 1] = u1; }
      const int lane = qp_lane();
      if (lane < nc2) gc[lane] = 0.0;
      for (int k = lane; k < nc2 * nc2; k += 64) Hc[k] = 0.0;
      QP_WSYNC();
    }
    if (lead) {  // tracking cost and CLF hinges (cbf_qp.py:914-920, 784-791)
      const double ce0 = clf_e[v2], ce1 = clf_e[v2 + 1], cv0 = clf_v[v2], cv1 = clf_v[v2 + 1];
      const double t0 = (u0 - unom[v2]) * cc.qp_w_acc, t1 = (u1 - unom[v2 + 1]) * cc.qp_w_steer;
      Fp = t0 * t0; Fp += t1 * t1;
      g0 = 2.0 * cc.qp_w_acc * t0; g1 = 2.0 * cc.qp_w_steer * t1;
      h00 = 2.0 * cc.qp_w_acc * cc.qp_w_acc; h11 = 2.0 * cc.qp_w_steer * cc.qp_w_steer;
      const double c0 = cv0 - ce0 * u0, c1 = cv1 - ce1 * u1;
      if (c0 > 0.0) { Fp += cc.qp_w_clf * c0 * c0; g0 += -2.0 * cc.qp_w_clf * ce0 * c0; h00 += 2.0 * cc.qp_w_clf * ce0 * ce0; }
      if (c1 > 0.0) { Fp += cc.qp_w_clf * c1 * c1; g1 += -2.0 * cc.qp_w_clf * ce1 * c1; h11 += 2.0 * cc.qp_w_clf * ce1 * ce1; }
    }
#pragma unroll
    for (int k = 0; k <= RMAX; ++k) {  // the lane rows, then (k == RMAX) the lane's candidate pair row: ONE inlined qp_phi per pass
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, g = 1.0, h = 0.0, w = cc.qp_w_lane, wl = cc.qp_w_lambda;
      bool pair = false;
      int ck = 0, cp0 = 0, cp2 = 0;  // the candidate row's unknowns: 4 (both vehicles) or 2 (a cross-group row: one vehicle's half); their compact indices
      if (k < RMAX) {
        if (k >= nrl) continue;
        const int r = sub + (k << sh);
        if (r < n_rows) { const double4 l4 = rows[r]; a0 = l4.x; a1 = l4.y; g = l4.z; h = l4.w; }
        g += a0 * u0; g += a1 * u1;
      } else {
        if (n_cand == 0) continue;
        const int ln = qp_lane();
        if (ln < n_cand) {
          const QpCand& cr = cand[ln];
          pair = true;
          ck = cr.k0 >> 16; cp0 = (cr.k0 >> 8) & 0xFF; cp2 = (cr.k2 >> 8) & 0xFF;
          const int ci0 = cr.k0 & 0xFF, ci2 = cr.k2 & 0xFF;
          a0 = cr.a[0]; a1 = cr.a[1]; g = cr.b0; h = cr.h;
          if (ck == 2) { w = cc.qp_w_cross; wl = cc.qp_w_lambda_cross; } else w = cc.qp_w_pair;
          g += a0 * xu[ci0]; g += a1 * xu[ci0 + 1];
          if (ck == 4) { a2 = cr.a[2]; a3 = cr.a[3]; g += a2 * xu[ci2]; g += a3 * xu[ci2 + 1]; }
        }
      }
      // (opaque weights: or the products of them that qp_phi forms are hoisted out of the solve into vector registers it does not have)
      if (k < RMAX && !VOPAQUE) asm volatile("" : "+s"(w), "+s"(wl));
      else if (k < RMAX) asm volatile("" : "+v"(w), "+v"(wl));  // (the deferred kernel's env loop: the scalar form does not compile there -- "illegal VGPR to SGPR copy")
      else asm volatile("" : "+v"(w), "+v"(wl));
      double d1, d2;
      Fp += qp_phi(g, h, w, wl, d1, d2);
      if (d2 != 0.0) {
        if (!pair) {
          g0 += d1 * a0; g1 += d1 * a1;
          h00 += d2 * a0 * a0; h01 += d2 * a0 * a1; h11 += d2 * a1 * a1;
        } else {
          double* H0 = Hc + cp0 * nc2;
          atomicAdd(&gc[cp0], d1 * a0); atomicAdd(&gc[cp0 + 1], d1 * a1);
          atomicAdd(&H0[cp0], d2 * a0 * a0); atomicAdd(&H0[cp0 + 1], d2 * a0 * a1);
          atomicAdd(&H0[nc2 + cp0], d2 * a1 * a0); atomicAdd(&H0[nc2 + cp0 + 1], d2 * a1 * a1);
          if (ck == 4) {
            double* H2 = Hc + cp2 * nc2;
            atomicAdd(&gc[cp2], d1 * a2); atomicAdd(&gc[cp2 + 1], d1 * a3);
            atomicAdd(&H0[cp2], d2 * a0 * a2); atomicAdd(&H0[cp2 + 1], d2 * a0 * a3);
            atomicAdd(&H0[nc2 + cp2], d2 * a1 * a2); atomicAdd(&H0[nc2 + cp2 + 1], d2 * a1 * a3);
            atomicAdd(&H2[cp0], d2 * a2 * a0); atomicAdd(&H2[cp0 + 1], d2 * a2 * a1);
            atomicAdd(&H2[nc2 + cp0], d2 * a3 * a0); atomicAdd(&H2[nc2 + cp0 + 1], d2 * a3 * a1);
            atomicAdd(&H2[cp2], d2 * a2 * a2); atomicAdd(&H2[cp2 + 1], d2 * a2 * a3);
            atomicAdd(&H2[nc2 + cp2], d2 * a3 * a2); atomicAdd(&H2[nc2 + cp2 + 1], d2 * a3 * a3);
          }
        }
      }
    }
    if (lpv >= 2) { g0 += dpp_f64<0xB1>(g0); g1 += dpp_f64<0xB1>(g1); h00 += dpp_f64<0xB1>(h00); h01 += dpp_f64<0xB1>(h01); h11 += dpp_f64<0xB1>(h11); }
    if (lpv == 4) { g0 += dpp_f64<0x4E>(g0); g1 += dpp_f64<0x4E>(g1); h00 += dpp_f64<0x4E>(h00); h01 += dpp_f64<0x4E>(h01); h11 += dpp_f64<0x4E>(h11); }
    if (n_cand > 0) {
      QP_WSYNC();
      if (pos2 >= 0) {  // the candidate rows' share of the vehicle's gradient and block
        g0 += gc[pos2]; g1 += gc[pos2 + 1];
        h00 += Hc[pos2 * nc2 + pos2]; h01 += Hc[pos2 * nc2 + pos2 + 1]; h11 += Hc[(pos2 + 1) * nc2 + pos2 + 1];
      }
    }
    e.F = qp_wave_sum(Fp); e.g0 = g0; e.g1 = g1; e.h00 = h00; e.h01 = h01; e.h11 = h11;
  }
  // largest gradient entry outside the bounds' normal cone at (u0, u1), over the whole problem
  __device__ __forceinline__ double projected_gradient(double u0, double u1, double g0, double g1) const {
    const bool b0 = (u0 <= lo0 && g0 > 0.0) || (u0 >= hi0 && g0 < 0.0), b1 = (u1 <= lo1 && g1 > 0.0) || (u1 >= hi1 && g1 < 0.0);
    return qp_wave_max(lead ? fmax(b0 ? 0.0 : fabs(g0), b1 ? 0.0 : fabs(g1)) : 0.0);
  }
};
// Returns 1 / 0: converged or not, the minimiser in q.u; -1: not handled (more than 64 candidate rows, or more than 8 vehicles in them), nothing
// was changed.  Called by ONE wavefront; N <= 64 (N <= 32 when RMAX < 8).
template <class Q, int RMAX>
__device__ __forceinline__ int qp_newton_registers(const sigmaenv_config_t& c, const sigmaenv_cbf_config_t& cc, const Smem& s, const Q& q, int N, int C,
                                                   int max_it, int& iters, unsigned long long* prof) {
  const int lane = qp_lane();
  QpVehicle<RMAX, Q::FULL_SMALL> V;
  V.n_cand = q.sci[0];
  if (V.n_cand > 64 || V.n_cand > N * C) return -1;  // (one lane per candidate row; their coefficients take the place of the N C centre kinematics)
  const int sh = N <= 16 ? 2 : (N <= 32 ? 1 : 0);
  V.lpv = 1 << sh;
  V.nrl = (2 * C + V.lpv - 1) >> sh;
  const int v = lane >> sh, sub = lane & (V.lpv - 1);
  const bool valid = v < N;
  V.lead = valid && sub == 0;
  const int vc = valid ? v : 0;
  V.v2 = 2 * vc;
  V.xu = q.un; V.gc = q.gn; V.Hc = q.H;
  V.pos2 = -1; V.nc2 = 0;
  V.cand = reinterpret_cast<const QpCand*>(s.kin);  // (the centre kinematics are not needed once the candidate rows are built)
  if (V.n_cand > 0) {
    for (int k = lane; k < N; k += 64) q.coupled[k] = 0;
    QP_WSYNC();
    int idx[4], ck = 0;
    double a[4], b0, h;
    if (lane < V.n_cand) {  // the lane's candidate row, as qp_eval builds it
      const unsigned ce = q.cand[lane];
      const int kind = (int)(ce >> Q::KIND_SHIFT);
      qp_pair_row(cc, s, q, C, (int)(ce & Q::ROW_MASK), idx, a, b0, h);
      ck = 4;
      if (kind != 0) {
        if (kind == 2) { idx[0] = idx[2]; a[0] = a[2]; a[1] = a[3]; }
        b0 = 0.5 * b0; h = cc.rs * h; ck = 2;
      }
      q.coupled[idx[0] >> 1] = 1;
      if (ck == 4) q.coupled[idx[2] >> 1] = 1;
    }
    QP_WSYNC();
    const bool member = valid && q.coupled[vc] != 0;
    const unsigned long long mk = __ballot(member && sub == 0);
    const int mc = __popcll(mk);
    if (mc > 8) return -1;
    const int pos = __popcll(mk & ((1ull << (vc << sh)) - 1ull));
    V.pos2 = member ? 2 * pos : -1;
    V.nc2 = 2 * mc;
    QP_WSYNC();
    if (member && sub == 0) q.coupled[vc] = pos;
    if (lane < V.nc2) q.cmap[lane] = (uint8_t)lane;  // (qp_newton_direction's map of compact unknowns: the compact system is the whole system here)
    QP_WSYNC();
    if (ck != 0) {  // (every lane has read the kinematics it needs: the rows may go where they were)
      QpCand* cr = reinterpret_cast<QpCand*>(s.kin) + lane;
      cr->a[0] = a[0]; cr->a[1] = a[1]; cr->a[2] = a[2]; cr->a[3] = a[3]; cr->b0 = b0; cr->h = h;
      cr->k0 = idx[0] | ((2 * q.coupled[idx[0] >> 1]) << 8) | (ck << 16);
      cr->k2 = ck == 4 ? (idx[2] | ((2 * q.coupled[idx[2] >> 1]) << 8)) : 0;
    }
    QP_WSYNC();
  }
  V.rows = q.lc + vc * 2 * C; V.sub = sub; V.sh = sh; V.n_rows = valid ? 2 * C : 0;
  V.unom = q.unom; V.clf_e = q.clf_e; V.clf_v = q.clf_v;
  V.lo0 = qp_uniform(c.min_acc); V.hi0 = qp_uniform(c.max_acc); V.lo1 = -cc.steering_rate_max; V.hi1 = cc.steering_rate_max;
  double u0 = q.u[2 * vc], u1 = q.u[2 * vc + 1];
  QpBlock e, en;
  bool converged = false;
  // ONE evaluation site (the compiler unrolls the rows and inlines qp_phi into it): the loop evaluates "the next point", which is the current
  // iterate (ITER: at the start, where nothing is known yet), a trial point of the line search (TRIAL) or the last iterate after a step that was
  // accepted without an evaluation (FINAL).  An accepted trial point's evaluation IS the next iterate's -- also for the compact Hessian in LDS.
  enum { ITER, TRIAL, FINAL };
  int mode = ITER, it = 0, ls = 0;
  double n0 = u0, n1 = u1, p0 = 0.0, p1 = 0.0, pg = 0.0, alpha = 1.0, dec = 0.0, step = 0.0, pg_tol = 0.0;
  e.F = e.g0 = e.g1 = e.h00 = e.h01 = e.h11 = 0.0;
  while (max_it > 0) {
    iters = it + 1;
#ifdef SIGMAENV_PROFILE
    const unsigned long long te0 = __builtin_readcyclecounter();
#endif
    V.eval(cc, n0, n1, en);  // (n: the iterate itself at the start and in FINAL)
#ifdef SIGMAENV_PROFILE
    prof[0] += __builtin_readcyclecounter() - te0; prof[2] += 1ull;
#endif
    if (mode == FINAL) { converged = V.projected_gradient(u0, u1, en.g0, en.g1) <= qp_vanish_tol(pg_tol); break; }  // (reached through a vanishing step only)
    bool direction = true;
    if (mode == ITER) e = en;
    else {
      bool accepted = en.F <= e.F + 1e-4 * dec;
      if (!accepted && en.F <= e.F + 1e-12 * fabs(e.F))  // (the rounding noise of F; see the oracle)
        accepted = V.projected_gradient(n0, n1, en.g0, en.g1) <= 0.5 * pg;
      pg_tol = 1e-6 * (1.0 + fabs(e.F));
      if (!accepted) {
        alpha *= 0.5;
        if (++ls == 60) { converged = pg <= pg_tol; break; }  // stalled: same rule as below
        direction = false;
      } else {
        u0 = n0; u1 = n1;
        if (step <= 1e-10 || it == max_it - 1) { converged = V.projected_gradient(u0, u1, en.g0, en.g1) <= (step <= 1e-10 ? qp_vanish_tol(pg_tol) : pg_tol); break; }  // (a vanishing step: the looser test, see the oracle)
        e = en;
        ++it; iters = it + 1;
      }
    }
#ifdef SIGMAENV_PROFILE
    const unsigned long long td0 = __builtin_readcyclecounter();
#endif
    if (direction) {
      // held variables (Bertsekas' epsilon-active set, as below): identity row / column
      // (the band's width: min(1e-4 of the range, |u - P(u - D grad)|) with D the inverse diagonal of H -- Bertsekas' rule, see the oracle)
      const double s0 = e.g0 / e.h00, s1 = e.g1 / e.h11;
      const double band = qp_wave_max(V.lead ? fmax(fabs(u0 - clip_d(u0 - s0, V.lo0, V.hi0)), fabs(u1 - clip_d(u1 - s1, V.lo1, V.hi1))) : 0.0);
      const double eps0 = fmin(1e-4 * (V.hi0 - V.lo0), band), eps1 = fmin(1e-4 * (V.hi1 - V.lo1), band);
      const bool held0 = (u0 - V.lo0 <= eps0 && e.g0 > 0.0) || (V.hi0 - u0 <= eps0 && e.g0 < 0.0);
      const bool held1 = (u1 - V.lo1 <= eps1 && e.g1 > 0.0) || (V.hi1 - u1 <= eps1 && e.g1 < 0.0);
      const double r0 = held0 ? -s0 : -e.g0, r1 = held1 ? -s1 : -e.g1;
      const double h00 = held0 ? 1.0 : e.h00, h11 = held1 ? 1.0 : e.h11, h01 = (held0 || held1) ? 0.0 : e.h01;
      const double det = h00 * h11 - h01 * h01;
      p0 = (h11 * r0 - h01 * r1) / det; p1 = (h00 * r1 - h01 * r0) / det;  // a vehicle on its own: its 2 x 2 system in closed form
      if (V.n_cand > 0) {
        // the vehicles of the candidate rows: the compact system.  LDS holds the candidate rows' part of the Hessian at this iterate (see above);
        // the vehicles put their complete blocks on the diagonal, the held unknowns get identity rows / columns
        const bool writer = V.lead && V.pos2 >= 0;
        if (writer) {
          for (int l = 0; l < V.nc2; ++l) {
            if (held0) { V.Hc[V.pos2 * V.nc2 + l] = 0.0; V.Hc[l * V.nc2 + V.pos2] = 0.0; }
            if (held1) { V.Hc[(V.pos2 + 1) * V.nc2 + l] = 0.0; V.Hc[l * V.nc2 + V.pos2 + 1] = 0.0; }
          }
        }
        QP_WSYNC();
        if (writer) {
          double* Hd = V.Hc + V.pos2 * V.nc2 + V.pos2;
          Hd[0] = h00; Hd[1] = h01; Hd[V.nc2] = h01; Hd[V.nc2 + 1] = h11;
          q.p[V.pos2] = r0; q.p[V.pos2 + 1] = r1;
        }
        QP_WSYNC();
        if (V.nc2 > 8) qp_newton_direction<16, false>(V.Hc, q.p, q.cmap, V.nc2, V.nc2);
        else if (V.nc2 > 4) qp_newton_direction<8, false>(V.Hc, q.p, q.cmap, V.nc2, V.nc2);
        else qp_newton_direction<4, false>(V.Hc, q.p, q.cmap, V.nc2, V.nc2);  // (one pair of vehicles: most envs with candidate rows)
        QP_WSYNC();
        if (V.pos2 >= 0) { p0 = q.p[V.pos2]; p1 = q.p[V.pos2 + 1]; }
      }
      pg = V.projected_gradient(u0, u1, e.g0, e.g1);
      alpha = 1.0; ls = 0;
#ifdef SIGMAENV_PROFILE
      prof[1] += __builtin_readcyclecounter() - td0;
#endif
    }
    // next trial point of the Armijo search along the projection arc
    n0 = clip_d(u0 + alpha * p0, V.lo0, V.hi0); n1 = clip_d(u1 + alpha * p1, V.lo1, V.hi1);
    dec = qp_wave_sum(V.lead ? e.g0 * (n0 - u0) + e.g1 * (n1 - u1) : 0.0);
    step = qp_wave_max(V.lead ? fmax(fabs(n0 - u0), fabs(n1 - u1)) : 0.0);
    mode = TRIAL;
    if (step <= 1e-14) {  // a vanishing step is accepted as it is; what remains is the stopping test at the point it leads to
      pg_tol = 1e-6 * (1.0 + fabs(e.F));
      u0 = n0; u1 = n1; mode = FINAL;
    }
  }
  QP_WSYNC();
  if (V.lead) { q.u[2 * v] = u0; q.u[2 * v + 1] = u1; }
  QP_WSYNC();
  return converged ? 1 : 0;
}

// DEFER: the envs the LEAN launch flagged (defer[env] != 0), solved from scratch with the full layout (Hessian and candidate list in LDS).  A workgroup looks at
// QP_DEFER_SPAN envs -- B / QP_DEFER_SPAN workgroups that find nothing and leave, instead of B that each wait for 23 KB of LDS and four wave slots beside the other
// stream's launch (a 2048-workgroup launch with nothing to do took 20-30 us there: profiles/r06_qp_lds.txt).
constexpr int QP_DEFER_SPAN = 16;
// phase stamps of the profile build (tools/qp_phase_cycles.py); in the product build every stamp is the constant 0 and the whole bookkeeping folds away (it used to
// stay in the product kernel behind a run-time flag: stamp values live across the phases -- a quarter of the kernel's spilled registers)
#ifdef SIGMAENV_PROFILE
#define QP_STAMP() __builtin_readcyclecounter()
#define QP_STAMP_RT() __builtin_amdgcn_s_memrealtime()
#else
#define QP_STAMP() 0ull
#define QP_STAMP_RT() 0ull
#endif
template <bool BIG, bool LEAN, bool DEFER>
__global__ void __launch_bounds__(256, BIG ? 1 : 4) sigmaenv_cbf_qp_kernel(sigmaenv_config_t c, sigmaenv_cbf_config_t cc, DevMap m, DevBufs g, const float4* __restrict__ seg4,
                                                              const float* __restrict__ segl, int seg_stride, const float2* __restrict__ in_cxy,
                                                              const double2* __restrict__ in_u, const Kin* __restrict__ in_kin,
                                                              const double2* __restrict__ in_clf, const float* __restrict__ actions,
                                                              float* __restrict__ actions_safe, double* __restrict__ u_opt, int32_t* __restrict__ info,
                                                              const int32_t* __restrict__ groups, int dbg_skip, uint32_t* __restrict__ cand_hbm, uint8_t* __restrict__ defer) {
  sigma_poison_lds();
  static_assert(!DEFER || (!BIG && !LEAN), "the deferred launch runs the full small layout");
  typedef QpSmemT<BIG, LEAN> Q;
  // (DEFER: the span's flags in ONE load -- lane k of every wavefront reads flag k -- then the set bits in turn)
  unsigned long long todo = 1ull;
  const int b_first = DEFER ? (int)blockIdx.x * QP_DEFER_SPAN : (int)blockIdx.x;
  if (DEFER) {
    const int k = (int)(threadIdx.x & 63u);
    todo = __ballot(k < QP_DEFER_SPAN && b_first + k < c.n_envs && defer[b_first + k] != 0);
  }
#pragma unroll 1
  while (todo != 0ull) {
  const int b = b_first + (DEFER ? __ffsll((long long)todo) - 1 : 0);
  todo &= todo - 1ull;
  do {  // (one env; `break` leaves it)
  extern __shared__ __attribute__((aligned(16))) char cbf_smem[];
  int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int N = c.n_agents, C = cc.n_circles, n = 2 * N;
  const int nwave = (int)((unsigned)b & 3u) < (int)(blockDim.x >> 6) ? (int)((unsigned)b & 3u) : 0;  // the wavefront that compacts the candidate list and runs the Newton iterations
  [[maybe_unused]] const unsigned long long tk0 = QP_STAMP();
  [[maybe_unused]] const unsigned long long rt0 = (dbg_skip & 128) ? QP_STAMP_RT() : 0ull;
  [[maybe_unused]] unsigned long long tk1 = 0, tk2 = 0, tk3 = 0, tk4 = 0, tk5 = 0;
  const bool grouping = groups != nullptr;  // grouped CBF-QPs (cbf_qp.py:1562-2281): the group problems share no variable and are solved as one
  // (BIG: the candidate list of env b in HBM -- written and read by the one wavefront that runs the Newton phase)
  Q q(cbf_smem + ((Smem::qp_bytes(N, C) + 31) & ~(size_t)31), N, C, BIG ? reinterpret_cast<typename Q::cand_t*>(cand_hbm + (size_t)b * Q::cand_entries(N, C)) : nullptr);
  Smem s(cbf_smem, N, C, LEAN ? reinterpret_cast<float*>(q.lc) : reinterpret_cast<float*>(q.H));  // the stencil distances: in the Hessian's bytes (N C 2 x 9 floats <= hwords), LEAN: where the lane rows go
  for (int i = tid; i < N; i += blockDim.x) q.grp[i] = grouping ? (uint8_t)groups[(size_t)b * N + i] : (uint8_t)0;
  // the vehicles' circle centres, nominal actions and centre kinematics: evaluated here (one lane per vehicle: no launch of their own, no round trip through HBM) or --
  // in_kin given: the test hook that injects circle centres -- read as sigmaenv_cbf_kin_kernel left them
  for (int i = tid; i < N * C && in_kin; i += blockDim.x) {
    s.kin[i] = in_kin[(size_t)b * N * C + i];
    s.cxy[i] = in_cxy[(size_t)b * N * C + i];
  }
  stencil_prologue(m, g, s, b, N, C);
  for (int i4 = tid; i4 < 4 * N; i4 += blockDim.x) {  // four lanes per vehicle (kin_vehicle<4>); lane 0 of the quad keeps the per-vehicle values
    const int i = i4 >> 2, sub = i4 & 3;
    double2 un, ce;
    if (in_kin) { un = in_u[(size_t)b * N + i]; ce = in_clf[(size_t)b * N + i]; }
    else kin_vehicle<4>(c, cc, g, actions, (size_t)b * N + i, sub, s.cxy + i * C, un, s.kin + i * C, ce);
    if (sub == 0) {
      s.path[i] = g.path[((size_t)b * N + i) * 4];
      q.sv[i] = make_float2(g.state[((size_t)b * N + i) * 8 + 3], g.state[((size_t)b * N + i) * 8 + 4]);
      q.unom[2 * i] = un.x; q.unom[2 * i + 1] = un.y;
      if (!LEAN) { q.lo[2 * i] = c.min_acc; q.hi[2 * i] = c.max_acc; q.lo[2 * i + 1] = -cc.steering_rate_max; q.hi[2 * i + 1] = cc.steering_rate_max; }  // cbf_qp.py:765-770 (float64 bounds)
      // CLF rows: the speed row acts on the acceleration, the heading row on the steering rate (:784-791, 1088-1091); zero for "rl"
      q.clf_e[2 * i] = ce.x; q.clf_v[2 * i] = cc.lam_clf * 0.5 * (ce.x * ce.x);
      q.clf_e[2 * i + 1] = ce.y; q.clf_v[2 * i + 1] = cc.lam_clf * 0.5 * (ce.y * ce.y);
      q.u[2 * i] = clip_d(un.x, (double)c.min_acc, (double)c.max_acc);  // warm start: U_nom (:1213-1215)
      q.u[2 * i + 1] = clip_d(un.y, -cc.steering_rate_max, cc.steering_rate_max);
    }
  }
  {  // pair table
    const int i = tid;
    if (i < N - 1) {
      const int off = i * (2 * N - i - 1) / 2;
      for (int j = i + 1; j < N; ++j) q.pij[off + j - i - 1] = (uint16_t)(i | (j << 8));
    }
  }
  __syncthreads();
  tk1 = QP_STAMP();
  unsigned long long st_stamps[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
  stencil_phase<QP_STENCIL_LPT>(cc, m, s, seg4, segl, seg_stride, N, C, dbg_skip & 9, st_stamps);
  __syncthreads();
  tk2 = QP_STAMP();
  // lane rows, ttcbf_lane_affine_coeffs adaptive branch (cbf_qp.py:2341-2369).  LEAN: row t (32 bytes at 32 t) goes where the stencil distances lie (36 bytes at 36 t' per
  // row): it covers distances of rows t' <= t only -- every round of the loop reads its distances before any of its rows is written, later rounds read behind them
  for (int t0 = 0; t0 < N * C * 2; t0 += blockDim.x) {
    const int t = t0 + tid;
    double4 row = make_double4(0.0, 0.0, 0.0, 0.0);
    if (t < N * C * 2) {
      const int ic = t >> 1;
      const LaneEst e = lane_estimate(cc, s.d9 + t * 9);
      const Kin& kn = s.kin[ic];
      const double dt = cc.dt_taylor;
      const double h = e.sm - cc.safety_buffer;
      const double A0 = 0.5 * (dt * dt) * (e.g0 * kn.ax0 + e.g1 * kn.ay0);
      const double A1 = 0.5 * (dt * dt) * (e.g0 * kn.ax1 + e.g1 * kn.ay1);
      const double dot_h = e.g0 * kn.dx + e.g1 * kn.dy;
      const double vh0 = kn.dx * e.h00 + kn.dy * e.h01, vh1 = kn.dx * e.h01 + kn.dy * e.h11;
      const double const_dd = e.g0 * kn.cx + e.g1 * kn.cy + (vh0 * kn.dx + vh1 * kn.dy);
      row = make_double4(A0, A1, dot_h * dt + 0.5 * (dt * dt) * const_dd, h);
    }
    if (LEAN) __syncthreads();
    if (t < N * C * 2) q.lc[t] = row;
  }
  if constexpr (LEAN) {  // what the candidate-flag phase's pair pass reads (below), written before the barrier the lane rows need anyway
    const int n_pairs_ = N * (N - 1) / 2, n_pair_rows = n_pairs_ * C * C;
    {
      uint8_t* cflag = reinterpret_cast<uint8_t*>(q.H);
      double* vs = q.gn;
      for (int k = tid; k < (n_pair_rows + 3) / 4; k += blockDim.x) reinterpret_cast<uint32_t*>(cflag)[k] = 0u;
      for (int i = (int)blockDim.x - 1 - tid; i < N; i += blockDim.x) {  // (the workgroup's LAST lanes: the first ones have lane rows to build)
        // (upper bounds of the norms: the largest squared norm over the circles in float64, its root by the 1-ulp hardware float32 root with 1e-6 of slack upwards)
        double m4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int ci = 0; ci < C; ++ci) {
          const Kin& k = s.kin[i * C + ci];
          const double v4[4] = {k.dx * k.dx + k.dy * k.dy, k.ax0 * k.ax0 + k.ay0 * k.ay0, k.ax1 * k.ax1 + k.ay1 * k.ay1, k.cx * k.cx + k.cy * k.cy};
#pragma unroll
          for (int e = 0; e < 4; ++e) m4[e] = (v4[e] > m4[e] || v4[e] != v4[e]) ? v4[e] : m4[e];  // (a NaN stays)
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) vs[4 * i + e] = (double)(__builtin_amdgcn_sqrtf((float)m4[e] * 1.000001f) * 1.000001f);  // (overflow -> inf: the pair is kept)
      }
    }
  }
  if (tid == 0) { q.sci[0] = 0; q.sci[1] = 0; q.sci[2] = 0; }
  __syncthreads();
  tk3 = QP_STAMP();
  uint8_t* cflag = reinterpret_cast<uint8_t*>(q.H);  // (the Hessian's space is free until the first evaluation)
  int any_flag = 0;
  {  // Candidate pair rows.  A row's value is g(u) = b0 + a . u; over the box |a . u| <= sum |a_k| max(|lo_k|, |hi_k|), so a row whose
     // lower bound (plus h when lambda is free and h > 0) is non-negative has phi = 0 for EVERY iterate and is left out of all evaluations
     // (most pairs of a scene are far apart).  A NaN bound keeps the row.  Grouped QPs: a pair of vehicles of different groups has no
     // common row; if they are within observation_range of each other (cbf_qp.py:2103-2108) each gets its own one-sided row.
    const double amax = fmax(fabs((double)c.min_acc), fabs((double)c.max_acc)), wmax = cc.steering_rate_max;
    const int n_pairs = N * (N - 1) / 2, CC = C * C, n_pair_rows = n_pairs * CC;
    // the flag of pair row pr, exactly as the oracle evaluates it
    auto row_flag = [&](int pr) -> uint8_t {
      int idx[4];
      double a[4], b0, h;
      qp_pair_row(cc, s, q, C, pr, idx, a, b0, h);
      const int i = idx[0] >> 1, j = idx[2] >> 1;
      uint8_t f = 0;
      if (!grouping || q.grp[i] == q.grp[j]) {
        const double lb = b0 - (fabs(a[0]) + fabs(a[2])) * amax - (fabs(a[1]) + fabs(a[3])) * wmax + ((cc.qp_w_lambda <= 0.0 && h > 0.0) ? h : 0.0);
        f = !(lb > 1e-12) ? 1 : 0;
      } else {
        const float* si = g.state + ((size_t)b * N + i) * 8;
        const float* sj = g.state + ((size_t)b * N + j) * 8;
        const double d0 = (double)si[0] - (double)sj[0], d1 = (double)si[1] - (double)sj[1];
        if (sqrt(d0 * d0 + d1 * d1) <= cc.observation_range + 1e-9) {  // _euclid(centers_flat[i], centers_flat[j]) <= obs_range + 1e-9
          const double hx = cc.rs * h, extra = (cc.qp_w_lambda_cross <= 0.0 && hx > 0.0) ? hx : 0.0;
          const double lb1 = 0.5 * b0 - fabs(a[0]) * amax - fabs(a[1]) * wmax + extra;
          const double lb2 = 0.5 * b0 - fabs(a[2]) * amax - fabs(a[3]) * wmax + extra;
          f = (uint8_t)((!(lb1 > 1e-12) ? 2 : 0) | (!(lb2 > 1e-12) ? 4 : 0));
        }
      }
      return f;
    };
    // LEAN (round 6): a PAIR of vehicles first.  With V, A0, A1, Cc the largest norms of a vehicle's circle velocities / control columns / drift accelerations and
    // dmin, dmax the extreme distances between the two vehicles' circle centres, every one of the pair's C^2 rows has (Cauchy-Schwarz on each product of the row)
    //   lb >= [lambda free] max(0, dmin^2 - d_safe^2) - dmax (2 dt (V_i + V_j) + dt^2 (Cc_i + Cc_j) + dt^2 (amax (A0_i + A0_j) + wmax (A1_i + A1_j))),
    // so a pair whose bound exceeds 1e-9 (the rows' own threshold is 1e-12; the bound's rounding is ~1e-14) has no candidate row and its rows are not evaluated at
    // all: in a 16-vehicle CPM scene that is ~85 % of the 120 pairs (all but the ones within ~0.7 m).  NaN / inf anywhere keeps the pair.  The other pairs' rows are
    // evaluated exactly as before, densely over (listed pair, circle pair).  Grouped QPs: pairs of different groups are always listed (their one-sided rows have
    // another bound).  1080 rows in 9 rounds of 128 lanes -> one round over the pairs + ~2 over the listed rows (profiles/r06_qp_lds.txt).
    bool by_pairs = false;
    if constexpr (LEAN) {
      if (!(dbg_skip & 1024)) {
        by_pairs = true;
        double* vs = q.gn;                                         // [N][4]: V, A0, A1, Cc per vehicle (gn and p: 4 N doubles, free until the Newton phase)
        uint16_t* plist = reinterpret_cast<uint16_t*>(s.wl);       // the listed pairs (the stencil phase's candidate lists, free now: Smem::wl_bytes holds every pair)
        const double d_safe = 2.0 * cc.circle_radius + cc.safety_buffer, d_safe_sq = d_safe * d_safe, dt = cc.dt_taylor;
        for (int p0 = 0; p0 < n_pairs; p0 += blockDim.x) {
          const int pq = p0 + tid;
          bool keep = false;
          if (pq < n_pairs) {
            const unsigned ij = q.pij[pq];
            const int i = (int)(ij & 0xFFu), j = (int)(ij >> 8);
            keep = true;
            if (!grouping || q.grp[i] == q.grp[j]) {
              // (the rows' own d = float32 difference of the centres; its squared length in float32 carries <= 3 roundings: 1e-6 of slack each way)
              float dmin2 = INFINITY, dmax2 = 0.0f;
              bool bad = false;
              for (int ci = 0; ci < C; ++ci)
                for (int cj = 0; cj < C; ++cj) {
                  const float dx = s.cxy[i * C + ci].x - s.cxy[j * C + cj].x, dy = s.cxy[i * C + ci].y - s.cxy[j * C + cj].y;
                  const float d2 = dx * dx + dy * dy;
                  bad |= !(d2 == d2);
                  dmin2 = d2 < dmin2 ? d2 : dmin2;
                  dmax2 = d2 > dmax2 ? d2 : dmax2;
                }
              const double* vi = vs + 4 * i;
              const double* vj = vs + 4 * j;
              const double K = 2.0 * dt * (vi[0] + vj[0]) + (dt * dt) * (vi[3] + vj[3]) + (dt * dt) * (amax * (vi[1] + vj[1]) + wmax * (vi[2] + vj[2]));
              const double hterm = (cc.qp_w_lambda <= 0.0) ? fmax(0.0, (double)dmin2 * (1.0 - 1e-6) - d_safe_sq) : 0.0;
              const double LB = hterm - (double)(__builtin_amdgcn_sqrtf(dmax2 * 1.000001f) * 1.000001f) * K * (1.0 + 1e-12);
              keep = bad || !(LB > 1e-9);
            }
          }
          const unsigned long long bm = __ballot(keep);
          if (bm != 0ull) {  // (wavefront-uniform)
            int pos0 = 0;
            if (lane == 0) pos0 = atomicAdd(&q.sci[2], (int)__popcll(bm));
            pos0 = __builtin_amdgcn_readfirstlane(pos0);
            if (keep) plist[pos0 + (int)__popcll(bm & ((1ull << lane) - 1ull))] = (uint16_t)pq;
          }
        }
        __syncthreads();
        const int n_rows = q.sci[2] * CC;
        for (int k = tid; k < n_rows; k += blockDim.x) {
          const int pl = k / CC, pr = (int)plist[pl] * CC + (k - pl * CC);
          const uint8_t f = row_flag(pr);
          any_flag |= f;
          cflag[pr] = f;
        }
      }
    }
    if (!by_pairs) {
      for (int pr = tid; pr < n_pair_rows; pr += blockDim.x) {
        const uint8_t f = row_flag(pr);
        any_flag |= f;
        cflag[pr] = f;  // flags first; compacted in a fixed order below so that the list, and with it the order of every accumulation of the
      }                 // Newton phase, is the same on every run
    }
  }
  // (usually there is no candidate row at all: nothing to compact, the count stays 0.  One barrier and an LDS word instead of __syncthreads_or: three barriers and the
  //  y / z work-item ids, whose register then stayed alive -- spilled -- through the phases before)
  if (__any(any_flag != 0) && lane == 0) atomicOr(&q.sci[1], 1);
  __syncthreads();
  any_flag = q.sci[1];
  tk4 = QP_STAMP();
  if (any_flag && wave == nwave) {
    const int n_pair_rows = N * (N - 1) / 2 * C * C;
    int base = 0;
    for (int r0 = 0; r0 < n_pair_rows; r0 += 64) {
      const int pr = r0 + lane;
      const unsigned f = pr < n_pair_rows ? cflag[pr] : 0u;
      const unsigned long long bm1 = __ballot((f & 3u) != 0u);  // the common row, or the lower-numbered vehicle's cross row
      // (LEAN: the first LEAN_CAND entries are kept -- with more than that the env is not solved here -- the count is the true one)
      if ((f & 3u) && (!LEAN || base + __popcll(bm1 & ((1ull << lane) - 1ull)) < Q::LEAN_CAND)) q.cand[base + __popcll(bm1 & ((1ull << lane) - 1ull))] = (typename Q::cand_t)(pr | ((f & 2u) ? (1u << Q::KIND_SHIFT) : 0u));
      base += __popcll(bm1);
      const unsigned long long bm2 = __ballot((f & 4u) != 0u);  // the higher-numbered vehicle's cross row
      if ((f & 4u) && (!LEAN || base + __popcll(bm2 & ((1ull << lane) - 1ull)) < Q::LEAN_CAND)) q.cand[base + __popcll(bm2 & ((1ull << lane) - 1ull))] = (typename Q::cand_t)(pr | (2u << Q::KIND_SHIFT));
      base += __popcll(bm2);
    }
    if (lane == 0) q.sci[0] = base;
  }
  if (any_flag) __syncthreads();
  // The Newton iterations run on wavefront 0 alone: every phase below is either short (<= 2N unknowns, ~150 rows) or serial by nature, and
  // a single wavefront needs no workgroup barriers between them; the other wavefronts leave and free their slots for the next workgroup.
  // WHICH wavefront: wavefront w of a workgroup runs on SIMD w, so with "wavefront 0" the Newton phases of all resident workgroups queued on ONE SIMD of the CU
  // (four wave slots at 128 VGPRs: at most four workgroups per CU, three SIMDs idle through every Newton phase); workgroup b uses wavefront b mod 4
  if (wave != nwave) break;
  tid = lane;  // (the wavefront's lane index from here on)
  const int max_it = (dbg_skip & 16) ? 1 : ((dbg_skip & 64) ? 0 : 100);
  int iters = 0;
  [[maybe_unused]] unsigned long long tc0 = QP_STAMP(), tc_eval = 0, tc_chol = 0, tc_ls = 0, tcx;
#define QP_TIC() (tcx = QP_STAMP())
#define QP_TOC(acc) (acc += QP_STAMP() - tcx)
  bool converged = false;
  // no or few candidate pair rows (nearly always): the iteration in registers; otherwise the general one below, with everything in LDS
  unsigned long long tprof[3] = {0ull, 0ull, 0ull};
  QP_TIC();
  const int in_registers = ((dbg_skip & 256) || ((dbg_skip & 512) && q.sci[0] > 0)) ? -1 : qp_newton_registers<Q, BIG ? 8 : 4>(c, cc, s, q, N, C, max_it, iters, tprof);
  converged = in_registers > 0;
  if (LEAN && in_registers < 0) {  // not an env for the register path: the full-layout launch that follows solves it (nothing was written for it here)
    if (lane == 0) defer[b] = 1;
    break;
  }
  if (in_registers >= 0) QP_TOC(tc_eval);
  tk5 = QP_STAMP();
  if constexpr (!LEAN)
  for (int it = 0; it < max_it && !converged && in_registers < 0; ++it) {
    iters = it + 1;
    QP_TIC();
    qp_eval<Q, BIG>(cc, s, q, N, C, q.u, q.grad, true, 0);
    QP_TOC(tc_eval);
    QP_TIC();
    // variables held at a bound against the descent direction: identity row / column, zero right-hand side
    // (held = Bertsekas' epsilon-active set, as in the oracle: at or within 1e-4 of the range of a bound with the gradient pushing against
    // it; such a variable moves along its own scaled gradient and the projection puts it onto the bound)
    double band = 0.0;  // (the band's width shrinks with the step: min(1e-4 of the range, |u - P(u - D grad)|), D the inverse diagonal of H -- Bertsekas' rule, see the oracle)
    for (int k = tid; k < n; k += 64) band = fmax(band, fabs(q.u[k] - clip_d(q.u[k] - q.grad[k] / q.H[Q::hix(k, k, n)], q.lo[k], q.hi[k])));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) band = fmax(band, __shfl_xor(band, off, 64));
    for (int k = tid; k < n; k += 64) {
      const double eps = fmin(1e-4 * (q.hi[k] - q.lo[k]), band);
      const bool held = (q.u[k] - q.lo[k] <= eps && q.grad[k] > 0.0) || (q.hi[k] - q.u[k] <= eps && q.grad[k] < 0.0);
      q.p[k] = held ? -q.grad[k] / q.H[Q::hix(k, k, n)] : -q.grad[k];
      q.gn[k] = held ? 1.0 : 0.0;  // (gn is free until the line search: the held flags)
    }
    QP_WSYNC();
    for (int k = tid; k < n; k += 64) {  // (only the rows / columns of held variables are touched: usually none or a few)
      if (q.gn[k] != 0.0) {
        for (int l = 0; l < n; ++l) { q.H[Q::hix(k, l, n)] = 0.0; q.H[Q::hix(l, k, n)] = 0.0; }
      }
    }
    QP_WSYNC();
    for (int k = tid; k < n; k += 64) if (q.gn[k] != 0.0) q.H[Q::hix(k, k, n)] = 1.0;
    QP_WSYNC();
    // which vehicles are coupled through an active pair row (a non-zero entry outside their own 2 x 2 block)
    const bool coupled = lane < N && q.coupled[lane] != 0;  // set by the evaluation that built H
    const unsigned long long cm = __ballot(coupled);
    const int m2 = 2 * __popcll(cm);
    if (m2 <= 32) {  // (nearly always, also at N = 32: few vehicles of a scene interact at a time)
      if (!(dbg_skip & 32)) {
        const int a = lane;
        if (a < N) {
          if (coupled) {
            const int pos = __popcll(cm & ((1ull << a) - 1ull));
            q.cmap[2 * pos] = (uint8_t)(2 * a);
            q.cmap[2 * pos + 1] = (uint8_t)(2 * a + 1);
          } else {  // independent 2 x 2 block (identity rows where a bound holds the variable): closed form
            const double h00 = q.H[Q::hix(2 * a, 2 * a, n)], h01 = q.H[Q::hix(2 * a + 1, 2 * a, n)], h11 = q.H[Q::hix(2 * a + 1, 2 * a + 1, n)];
            const double r0 = q.p[2 * a], r1 = q.p[2 * a + 1];
            const double det = h00 * h11 - h01 * h01;
            q.p[2 * a] = (h11 * r0 - h01 * r1) / det;
            q.p[2 * a + 1] = (h00 * r1 - h01 * r0) / det;
          }
        }
        QP_WSYNC();
        if (m2 > 16) qp_newton_direction<32, BIG>(q.H, q.p, q.cmap, n, m2);
        else if (m2 > 8) qp_newton_direction<16, BIG>(q.H, q.p, q.cmap, n, m2);
        else if (m2 > 0) qp_newton_direction<8, BIG>(q.H, q.p, q.cmap, n, m2);
      }
    } else {
      // more than 16 coupled vehicles: the full system through LDS
      // Cholesky H = L L^T in place (lower triangle): per column the pivot, the column scaling and the trailing update
      for (int col = 0; col < n; ++col) {
        const double dcc = sqrt(q.H[Q::hix(col, col, n)]);
        QP_WSYNC();
        for (int k = col + tid; k < n; k += 64) q.H[Q::hix(k, col, n)] = (k == col) ? dcc : q.H[Q::hix(k, col, n)] / dcc;
        QP_WSYNC();
        const int rem = n - col - 1;
        for (int e2 = tid; e2 < rem * rem; e2 += 64) {
          const int k = col + 1 + e2 / rem, l = col + 1 + (e2 - (e2 / rem) * rem);
          if (l <= k) q.H[Q::hix(k, l, n)] -= q.H[Q::hix(k, col, n)] * q.H[Q::hix(l, col, n)];
        }
        QP_WSYNC();
      }
      {  // L y = rhs, L^T p = y; lanes over the rows
        for (int col = 0; col < n; ++col) {  // forward substitution
          const double y = q.p[col] / q.H[Q::hix(col, col, n)];
          QP_WSYNC();
          for (int k = lane; k < n; k += 64) {
            if (k == col) q.p[col] = y;
            if (k > col) q.p[k] -= q.H[Q::hix(k, col, n)] * y;
          }
          QP_WSYNC();
        }
        for (int col = n - 1; col >= 0; --col) {  // back substitution with L^T
          const double x = q.p[col] / q.H[Q::hix(col, col, n)];
          QP_WSYNC();
          for (int k = lane; k < n; k += 64) {
            if (k == col) q.p[col] = x;
            if (k < col) q.p[k] -= q.H[Q::hix(col, k, n)] * x;
          }
          QP_WSYNC();
        }
      }
    }
    QP_WSYNC();
    {
      // projected gradient at u (lanes over the unknowns: two per lane beyond 32 vehicles)
      double pg = 0.0;
      for (int k = lane; k < n; k += 64) {
        const bool at_bound = (q.u[k] <= q.lo[k] && q.grad[k] > 0.0) || (q.u[k] >= q.hi[k] && q.grad[k] < 0.0);
        pg = fmax(pg, at_bound ? 0.0 : fabs(q.grad[k]));
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) pg = fmax(pg, __shfl_xor(pg, off, 64));
      if (lane == 0) q.sc[4] = pg;
    }
    QP_WSYNC();
    QP_TOC(tc_chol);
    QP_TIC();
    // Armijo search along the projection arc (see the oracle for the acceptance rule near the rounding noise of F)
    double alpha = 1.0;
    bool accepted = false;
    double step = 0.0;
    for (int ls = 0; ls < 60 && !accepted; ++ls) {
      {
        double dec = 0.0, st = 0.0;
        for (int k = lane; k < n; k += 64) {
          const double v = clip_d(q.u[k] + alpha * q.p[k], q.lo[k], q.hi[k]);
          q.un[k] = v;
          dec += q.grad[k] * (v - q.u[k]);
          st = fmax(st, fabs(v - q.u[k]));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { dec += __shfl_xor(dec, off, 64); st = fmax(st, __shfl_xor(st, off, 64)); }
        if (lane == 0) { q.sc[2] = dec; q.sc[3] = st; }
      }
      QP_WSYNC();
      step = q.sc[3];
      const double dec = q.sc[2];
      if (step <= 1e-14) { accepted = true; break; }
      qp_eval<Q, BIG>(cc, s, q, N, C, q.un, q.gn, false, 1);
      const double F = q.sc[0], Fn = q.sc[1];
      if (Fn <= F + 1e-4 * dec) { accepted = true; break; }
      if (Fn <= F + 1e-12 * fabs(F)) {  // (the rounding noise of F; see the oracle)
        {
          double pg = 0.0;
          for (int k = lane; k < n; k += 64) {
            const bool held = (q.un[k] <= q.lo[k] && q.gn[k] > 0.0) || (q.un[k] >= q.hi[k] && q.gn[k] < 0.0);
            pg = fmax(pg, held ? 0.0 : fabs(q.gn[k]));
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) pg = fmax(pg, __shfl_xor(pg, off, 64));
          if (lane == 0) q.sc[5] = pg;
        }
        QP_WSYNC();
        if (q.sc[5] <= 0.5 * q.sc[4]) { accepted = true; break; }
      }
      alpha *= 0.5;
      QP_WSYNC();
    }
    QP_TOC(tc_ls);
    // no further descent within rounding / a vanishing step: the minimiser -- unless the projected gradient says otherwise (the iteration has
    // stalled: reported as not converged, the nominal action is used, as the reference does when its solver fails); same rule as the oracle
    const double pg_tol = 1e-6 * (1.0 + fabs(q.sc[0]));
    if (!accepted) { converged = q.sc[4] <= pg_tol; break; }
    QP_WSYNC();
    for (int k = tid; k < n; k += 64) q.u[k] = q.un[k];
    QP_WSYNC();
    if (step <= 1e-10 || it == max_it - 1) {  // (the gradient of the 1e9-weighted terms has a noise floor of ~1e-5: steps do not shrink to zero; at the
                                              // iteration limit the same test decides)
      qp_eval<Q, BIG>(cc, s, q, N, C, q.u, q.gn, false, 1);
      {
        double pg = 0.0;
        for (int k = lane; k < n; k += 64) {
          const bool at_bound = (q.u[k] <= q.lo[k] && q.gn[k] > 0.0) || (q.u[k] >= q.hi[k] && q.gn[k] < 0.0);
          pg = fmax(pg, at_bound ? 0.0 : fabs(q.gn[k]));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) pg = fmax(pg, __shfl_xor(pg, off, 64));
        converged = pg <= (step <= 1e-10 ? qp_vanish_tol(pg_tol) : pg_tol);  // (a vanishing step: the looser test, see the oracle)
      }
      break;
    }
  }
  // ---- outputs: the minimiser, u_to_rl_action (cbf_qp.py:499-525: float64 because the numpy input promotes), status -------------------
  bool finite = true;
  for (int k = tid; k < n; k += 64) finite = finite && isfinite(q.u[k]);
  const bool ok = converged && __ballot(!finite) == 0ull;  // (one wavefront is here)
  for (int i = tid; i < N; i += 64) {
    const size_t bi = (size_t)b * N + i;
    const double ua = ok ? q.u[2 * i] : q.unom[2 * i], us = ok ? q.u[2 * i + 1] : q.unom[2 * i + 1];  // fallback: the nominal action (:1274-1283)
    const double dt64 = cc.dt_taylor * 0.5;  // Parameters.dt as the Python float it is
    const float2 sv = q.sv[i];
    double v = (double)sv.x + ua * dt64;
    double st = (double)sv.y + us * dt64;
    const double sp = st + M_PI;
    double r = fabs(sp) < 2.0 * M_PI ? sp : fmod(sp, 2.0 * M_PI);  // (fmod(x, y) is x itself for |x| < y)
    if (r != 0.0 && r < 0.0) r += 2.0 * M_PI;
    st = r - M_PI;
    v = clip_d(v, (double)cc.min_speed, (double)c.max_speed);
    st = clip_d(st, (double)cc.min_steering, (double)c.max_steering);
    reinterpret_cast<float2*>(actions_safe)[bi] = make_float2((float)v, (float)st);
    // world_state.nominal_action_*: the safe action (cbf_qp.py:1343-1379), or -- when the safe action is applied -- the clamped policy
    // action (:1315-1325) / the CLF controller's target (:1084-1085, 1326-1337)
    float2 nomv = make_float2((float)v, (float)st);
    if (grouping && cc.nominal != 0) {  // grouped "clf": U_nom itself (:2262-2268)
      nomv = make_float2((float)q.unom[2 * i], (float)q.unom[2 * i + 1]);
    } else if ((cc.is_apply_cbf_action || grouping) && cc.nominal == 0) {  // grouped "rl": the clamped policy action (:2254-2260)
      const float2 a = reinterpret_cast<const float2*>(actions)[bi];
      nomv = make_float2(clampf(a.x, cc.min_speed, c.max_speed), clampf(a.y, cc.min_steering, c.max_steering));
    } else if (cc.is_apply_cbf_action) {
      nomv = make_float2(sv.x + (float)q.clf_e[2 * i], (float)q.clf_e[2 * i + 1]);
    }
    reinterpret_cast<float2*>(g.cbf_nominal)[bi] = nomv;
    if (u_opt) { u_opt[bi * 2] = q.u[2 * i]; u_opt[bi * 2 + 1] = q.u[2 * i + 1]; }
  }
  if (info && tid == 0) { info[2 * b] = iters; info[2 * b + 1] = ok ? 1 : 0; }
#ifdef SIGMAENV_PROFILE
  if ((dbg_skip & 128) && u_opt && tid == 0 && 2 * N >= 15) {  // profiling aid: shader-clock cycles (total, evaluation with Hessian, factorisation + solves, line search)
    double* d = u_opt + (size_t)b * N * 2;
    d[0] = (double)(QP_STAMP() - tc0); d[1] = (double)tc_eval; d[2] = (double)tc_chol; d[3] = (double)tc_ls;
    d[4] = (double)(tk1 - tk0); d[5] = (double)(tk2 - tk1); d[6] = (double)(tc0 - tk2);  // load, stencil phase, lane rows + candidate rows
    d[7] = (double)q.sci[0];  // candidate pair rows of the env
    d[10] = (double)(tk3 - tk2); d[11] = (double)(tk4 - tk3); d[12] = (double)(tc0 - tk4); d[13] = (double)(QP_STAMP() - tk5);  // lane rows, candidate flags, compaction; (register path) the output phase
    if (in_registers >= 0) { d[2] = (double)tprof[0]; d[3] = (double)tprof[1]; d[14] = (double)tprof[2]; }  // register path: cycles in evaluations, in the directions; evaluations
    if (2 * N >= 22) d[21] = (double)q.sci[2];  // pairs whose rows were evaluated (LEAN)
    d[8] = (double)rt0; d[9] = (double)QP_STAMP_RT();  // wall clock (100 MHz) at the workgroup's start and here
    if (2 * N >= 21) { d[15] = (double)(st_stamps[0] - tk1); d[16] = (double)(st_stamps[1] - st_stamps[0]); d[17] = (double)(st_stamps[2] - st_stamps[1]); d[18] = (double)(st_stamps[3] - st_stamps[2]);
                       d[19] = (double)(st_stamps[4] - st_stamps[3]); d[20] = (double)(tk2 - st_stamps[4]); }  // stencil phase of the Newton wavefront: set-up, stage 1, stage 2, bound, later passes, conversion
  }
#endif
  } while (0);
  if (DEFER) {
    __syncthreads();  // (the wavefronts that left the env's Newton phase to one of them wait here: the next env reuses the LDS)
    if (threadIdx.x == 0) defer[b] = 0;
  }
  }
}

// group_agents_k_nearest (cbf_qp.py:193-310) and the ordering update_grouped_cbf_qps gives its result (:1899-1902: members sorted, groups
// ordered by their first member), one thread per env: farthest-point seeds, then every vehicle joins the nearest group (centroid) with
// room.  Python float arithmetic = doubles, one operation each.  Runs once per run (use_fixed_groups, :1897-1909).
__device__ __forceinline__ double grp_sqdist(double ax, double ay, double bx, double by) { const double dx = ax - bx, dy = ay - by; return dx * dx + dy * dy; }
__global__ void __launch_bounds__(64) sigmaenv_cbf_group_kernel(DevBufs g, int B, int N, int m, int32_t* __restrict__ groups) {
  sigma_poison_lds();
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  constexpr int M = QP_MAX_AGENTS;
  double x[M], y[M], cx[M], cy[M], d[M];
  int seeds[M], raw[M], size[M], ord[M], first[M];
  bool is_seed[M];
  for (int i = 0; i < N; ++i) { x[i] = (double)g.state[((size_t)b * N + i) * 8]; y[i] = (double)g.state[((size_t)b * N + i) * 8 + 1]; is_seed[i] = false; raw[i] = -1; }
  const int K = (N + m - 1) / m;
  int ns = 0;
  seeds[ns++] = 0; is_seed[0] = true;
  while (ns < K) {
    int best = -1;
    double best_dist = -1.0;
    for (int i = 0; i < N; ++i) {
      if (is_seed[i]) continue;
      double d_min = INFINITY;
      for (int k = 0; k < ns; ++k) d_min = fmin(d_min, grp_sqdist(x[i], y[i], x[seeds[k]], y[seeds[k]]));
      if (d_min > best_dist) { best_dist = d_min; best = i; }
    }
    seeds[ns++] = best; is_seed[best] = true;
  }
  for (int k = 0; k < K; ++k) { raw[seeds[k]] = k; size[k] = 1; cx[k] = x[seeds[k]]; cy[k] = y[seeds[k]]; }
  for (int i = 0; i < N; ++i) {
    if (raw[i] >= 0) continue;
    for (int k = 0; k < K; ++k) { d[k] = grp_sqdist(x[i], y[i], cx[k], cy[k]); ord[k] = k; }
    for (int a = 1; a < K; ++a) {  // stable insertion sort (list.sort)
      const int v = ord[a];
      int bb = a - 1;
      while (bb >= 0 && d[ord[bb]] > d[v]) { ord[bb + 1] = ord[bb]; --bb; }
      ord[bb + 1] = v;
    }
    for (int a = 0; a < K; ++a) {
      const int k = ord[a];
      if (size[k] < m) {
        raw[i] = k; size[k] += 1;
        const double kk = (double)size[k];
        cx[k] = cx[k] + (x[i] - cx[k]) / kk; cy[k] = cy[k] + (y[i] - cy[k]) / kk;
        break;
      }
    }
  }
  for (int k = 0; k < K; ++k) first[k] = N;
  for (int i = N - 1; i >= 0; --i) first[raw[i]] = i;
  for (int i = 0; i < N; ++i) {
    int r = 0;
    for (int k = 0; k < K; ++k) r += (first[k] < first[raw[i]]) ? 1 : 0;
    groups[(size_t)b * N + i] = r;
  }
}

}  // namespace cbf

extern "C" int sigmaenv_cbf_attach(sigmaenv_t* h, const sigmaenv_cbf_config_t* cfg, const float* seg_left, const float* seg_right, int32_t seg_stride) {
  if (!h) return SIGMAENV_EINVAL;
  if (!cfg || !seg_left || !seg_right || seg_stride < 1) { h->err = "cbf_attach: null argument"; return SIGMAENV_EINVAL; }
  if (cfg->n_circles < 1 || cfg->n_circles > SIGMAENV_CBF_MAX_CIRCLES) { h->err = "cbf_attach: n_circles out of range"; return SIGMAENV_EINVAL; }
  // fields that took over formerly reserved bytes of the struct: a caller that still fills the old layout leaves them zero, which would
  // silently clamp the steering-rate box to [0, 0] (INTEGRATION.md section 8)
  if (!(cfg->steering_rate_max > 0.0)) { h->err = "cbf_attach: steering_rate_max must be > 0 (field added in place of a reserved one: rebuild the caller against the current header)"; return SIGMAENV_EINVAL; }
  if (cfg->is_grouping && (!(cfg->observation_range >= 0.0) || !(cfg->rs >= 0.0) || !(cfg->rs <= 1.0))) {
    h->err = "cbf_attach: grouped CBF-QPs need observation_range >= 0 and 0 <= rs <= 1";
    return SIGMAENV_EINVAL;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (h->cbf_seg4) {  // attached before: the earlier tables and intermediates are released first
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (void* q : {h->cbf_seg4, h->cbf_segl, h->cbf_cxy, h->cbf_u, h->cbf_kin, h->cbf_clf, h->cbf_safe, (void*)h->cbf_groups, h->cbf_cand_big, h->cbf_defer}) if (q) dev_free(h, q);
    h->cbf_seg4 = h->cbf_segl = h->cbf_cxy = h->cbf_u = h->cbf_kin = h->cbf_clf = h->cbf_safe = nullptr;
    h->cbf_groups = nullptr;
    h->cbf_cand_big = nullptr;
    h->cbf_defer = nullptr;
  }
  const int np = h->n_paths;
  std::vector<int32_t> cnt((size_t)3 * np);
  HIPCHK(h, hipMemcpyAsync(cnt.data(), h->map.n_center, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int p = 0; p < np; ++p) {
    if (cnt[np + p] - 1 > seg_stride || cnt[2 * np + p] - 1 > seg_stride) { h->err = "cbf_attach: seg_stride smaller than a boundary's segment count"; return SIGMAENV_EINVAL; }
  }
  // device layout: [path][side][seg_stride] of (cos, sin, m_b, m_t) and of the length
  const size_t n = (size_t)np * 2 * seg_stride;
  std::vector<float4> h4(n);
  std::vector<float> hl(n);
  for (int p = 0; p < np; ++p)
    for (int side = 0; side < 2; ++side) {
      const float* src = (side ? seg_right : seg_left) + (size_t)p * seg_stride * 5;
      for (int k = 0; k < seg_stride; ++k) {
        const size_t o = ((size_t)p * 2 + side) * seg_stride + k;
        h4[o] = make_float4(src[5 * k], src[5 * k + 1], src[5 * k + 2], src[5 * k + 3]);
        hl[o] = src[5 * k + 4];
      }
    }
  float4* d4 = nullptr;
  float* dl = nullptr;
  int rc;
  if ((rc = dev_alloc(h, (void**)&d4, n * sizeof(float4))) != SIGMAENV_OK) return rc;
  if ((rc = dev_alloc(h, (void**)&dl, n * sizeof(float))) != SIGMAENV_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(d4, h4.data(), n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dl, hl.data(), n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const size_t BN = (size_t)h->B * h->N, Cc = cfg->n_circles;
  void *d_cxy = nullptr, *d_u = nullptr, *d_kin = nullptr;  // per-vehicle intermediates between the two kernels
  if ((rc = dev_alloc(h, &d_cxy, BN * Cc * sizeof(float2), true)) != SIGMAENV_OK) return rc;
  if ((rc = dev_alloc(h, &d_u, BN * sizeof(double2), true)) != SIGMAENV_OK) return rc;
  if ((rc = dev_alloc(h, &d_kin, BN * Cc * sizeof(cbf::Kin), true)) != SIGMAENV_OK) return rc;
  void* d_clf = nullptr;
  if ((rc = dev_alloc(h, &d_clf, BN * sizeof(double2), true)) != SIGMAENV_OK) return rc;
  void* d_safe = nullptr;  // safe actions of sigmaenv_rollout's QP step
  if ((rc = dev_alloc(h, &d_safe, BN * 2 * sizeof(float), true)) != SIGMAENV_OK) return rc;
  h->cbf_cxy = d_cxy; h->cbf_u = d_u; h->cbf_kin = d_kin; h->cbf_clf = d_clf; h->cbf_safe = d_safe;
  h->cbf_groups_valid = false;
  if (cfg->is_grouping) {
    if (cfg->max_group_size < 1) { h->err = "cbf_attach: max_group_size must be >= 1"; return SIGMAENV_EINVAL; }  // cbf_qp.py:1575-1576
    if ((rc = dev_alloc(h, (void**)&h->cbf_groups, BN * sizeof(int32_t))) != SIGMAENV_OK) return rc;
  }
  h->cbf_cfg = *cfg;
  h->cbf_seg4 = d4;
  h->cbf_segl = dl;
  h->cbf_seg_stride = seg_stride;
  return SIGMAENV_OK;
}

// profile build only: phase-ablation mask of the CBF kernels (tools/cbf_timing.py, tools/qp_phase_cycles.py); the product passes 0
static int cbf_debug_skip() {
#ifdef SIGMAENV_PROFILE
  static const int v = getenv("SIGMAENV_CBF_DEBUG_SKIP") ? atoi(getenv("SIGMAENV_CBF_DEBUG_SKIP")) : 0;
  return v;
#else
  return 0;
#endif
}

// Test hook (include/sigmaenv.h): the circle centres the two CBF entry points work on are replaced by the caller's ([B,N,C,2] device f32; NULL: computed again)
extern "C" int sigmaenv_cbf_inject_centers(sigmaenv_t* h, const float* centers) {
  if (!h) return SIGMAENV_EINVAL;
  h->cbf_centers_inject = centers;
  return SIGMAENV_OK;
}
// sigmaenv_cbf_kin_kernel on `actions` into the handle's cbf_cxy / cbf_u / cbf_kin / cbf_clf, then the injected circle centres (if any) over the computed ones
static int cbf_launch_kin(sigmaenv* h, const float* actions) {
  const size_t BN = (size_t)h->B * h->N;
  hipLaunchKernelGGL(cbf::sigmaenv_cbf_kin_kernel, dim3((unsigned)((BN + 255) / 256)), dim3(256), 0, h->stream, h->cfg, h->cbf_cfg, h->buf, actions,
                     (float2*)h->cbf_cxy, (double2*)h->cbf_u, (cbf::Kin*)h->cbf_kin, (double2*)h->cbf_clf);
  if (!h->cbf_centers_inject) return SIGMAENV_OK;
  HIPCHK(h, hipMemcpyAsync(h->cbf_cxy, h->cbf_centers_inject, BN * h->cbf_cfg.n_circles * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_cbf_rewards(sigmaenv_t* h, const float* actions, double* margins) {
  if (!h) return SIGMAENV_EINVAL;
  if (!actions) { h->err = "cbf_rewards: null actions"; return SIGMAENV_EINVAL; }
  if (!h->cbf_seg4) { h->err = "cbf_rewards: sigmaenv_cbf_attach has not been called"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rck = cbf_launch_kin(h, actions); if (rck) return rck; }
  const int slot = timer_begin(h, SIGMAENV_KERNEL_CBF_MARGIN);
  hipLaunchKernelGGL(cbf::sigmaenv_cbf_kernel, dim3(h->B), dim3(256), cbf::Smem::bytes(h->N, h->cbf_cfg.n_circles), h->stream, h->cfg, h->cbf_cfg, h->map,
                     h->buf, (const float4*)h->cbf_seg4, (const float*)h->cbf_segl, h->cbf_seg_stride, (const float2*)h->cbf_cxy, (const double2*)h->cbf_u,
                     (const cbf::Kin*)h->cbf_kin, margins, cbf_debug_skip());
  HIPCHK(h, hipGetLastError());
  timer_end(h, SIGMAENV_KERNEL_CBF_MARGIN, slot);
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_cbf_qp(sigmaenv_t* h, const float* actions, float* actions_safe, double* u_opt, int32_t* info) {
  if (!h) return SIGMAENV_EINVAL;
  if (!actions || !actions_safe) { h->err = "cbf_qp: null actions / actions_safe"; return SIGMAENV_EINVAL; }
  if (!h->cbf_seg4) { h->err = "cbf_qp: sigmaenv_cbf_attach has not been called"; return SIGMAENV_EINVAL; }
  if (h->N > cbf::QP_MAX_AGENTS) { h->err = "cbf_qp: more than 64 agents"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  const int Cc = h->cbf_cfg.n_circles;
  // up to 32 vehicles: the LEAN instantiation (register-path Newton iterations only) for every env, then the full-layout one (Hessian and candidate list in LDS) for the
  // envs the first launch flagged; 33 .. 64: packed Hessian in LDS, candidate list in HBM (one workgroup per CU)
  const bool big = h->N > cbf::QP_SMALL_AGENTS;
  const size_t smem0 = (cbf::Smem::qp_bytes(h->N, Cc) + 31) & ~(size_t)31;
  const size_t smem = smem0 + (big ? cbf::QpSmemT<true>::bytes(h->N, Cc) : cbf::QpSmemT<false>::bytes(h->N, Cc));
  const size_t smem_lean = smem0 + cbf::QpSmemT<false, true>::bytes(h->N, Cc);
  if (smem > 160 * 1024) { h->err = "cbf_qp: the problem does not fit the 160 KB of LDS (vehicles x circles)"; return SIGMAENV_EINVAL; }
  if (!big && (size_t)h->N * (h->N - 1) / 2 * Cc * Cc > cbf::QpSmemT<false>::ROW_MASK) { h->err = "cbf_qp: too many pair rows for the 14-bit candidate index"; return SIGMAENV_EINVAL; }
  if (big && !h->cbf_cand_big) {
    const int rc = dev_alloc(h, (void**)&h->cbf_cand_big, (size_t)h->B * cbf::QpSmemT<true>::cand_entries(h->N, Cc) * sizeof(uint32_t), true);
    if (rc != SIGMAENV_OK) return rc;
  }
  if (!big && !h->cbf_defer) {
    const int rc = dev_alloc(h, (void**)&h->cbf_defer, (size_t)h->B);
    if (rc != SIGMAENV_OK) return rc;
    HIPCHK(h, hipMemsetAsync(h->cbf_defer, 0, (size_t)h->B, h->stream));
  }
  if (smem > 64 * 1024) {
    if (big) { HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(cbf::sigmaenv_cbf_qp_kernel<true, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); }
    else { HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(cbf::sigmaenv_cbf_qp_kernel<false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); }
  }
  const bool grouping = h->cbf_cfg.is_grouping != 0;
  if (grouping && !h->cbf_groups_valid) {  // the partition of the first call stays (use_fixed_groups, cbf_qp.py:1897-1909)
    hipLaunchKernelGGL(cbf::sigmaenv_cbf_group_kernel, dim3((unsigned)((h->B + 63) / 64)), dim3(64), 0, h->stream, h->buf, h->B, h->N, h->cbf_cfg.max_group_size,
                       h->cbf_groups);
    HIPCHK(h, hipGetLastError());
    h->cbf_groups_valid = true;
  }
  // the per-vehicle kinematics are evaluated inside the QP kernel; only with injected circle centres (test hook) they come from a launch of their own
  const bool own_kin = h->cbf_centers_inject != nullptr;
  if (own_kin) { const int rck = cbf_launch_kin(h, actions); if (rck) return rck; }
  const int slot = timer_begin(h, SIGMAENV_KERNEL_CBF_QP);
#define SIGMA_QP_ARGS h->cfg, h->cbf_cfg, h->map, h->buf, (const float4*)h->cbf_seg4, (const float*)h->cbf_segl, h->cbf_seg_stride, (const float2*)(own_kin ? h->cbf_cxy : nullptr), \
                      (const double2*)(own_kin ? h->cbf_u : nullptr), (const cbf::Kin*)(own_kin ? h->cbf_kin : nullptr), (const double2*)(own_kin ? h->cbf_clf : nullptr), actions, actions_safe, u_opt, info, \
                      (const int32_t*)(grouping ? h->cbf_groups : nullptr), cbf_debug_skip(), (uint32_t*)h->cbf_cand_big, (uint8_t*)h->cbf_defer
  if (big) hipLaunchKernelGGL((cbf::sigmaenv_cbf_qp_kernel<true, false, false>), dim3(h->B), dim3(256), smem, h->stream, SIGMA_QP_ARGS);
  else {
    hipLaunchKernelGGL((cbf::sigmaenv_cbf_qp_kernel<false, true, false>), dim3(h->B), dim3(QP_LEAN_THREADS), smem_lean, h->stream, SIGMA_QP_ARGS);
#ifndef QP_NO_FAT  /* (experiment: what the second launch costs when no env is left to it) */
    hipLaunchKernelGGL((cbf::sigmaenv_cbf_qp_kernel<false, false, true>), dim3((unsigned)((h->B + cbf::QP_DEFER_SPAN - 1) / cbf::QP_DEFER_SPAN)), dim3(256), smem, h->stream, SIGMA_QP_ARGS);
#endif
  }
#undef SIGMA_QP_ARGS
  HIPCHK(h, hipGetLastError());
  timer_end(h, SIGMAENV_KERNEL_CBF_QP, slot);
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_cbf_regroup(sigmaenv_t* h) {
  if (!h) return SIGMAENV_EINVAL;
  h->cbf_groups_valid = false;
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_cbf_get_groups(sigmaenv_t* h, int32_t* groups_host) {
  if (!h) return SIGMAENV_EINVAL;
  if (!groups_host || !h->cbf_groups || !h->cbf_groups_valid) { h->err = "cbf_get_groups: no groups (grouped sigmaenv_cbf_qp has not run)"; return SIGMAENV_EINVAL; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(groups_host, h->cbf_groups, (size_t)h->B * h->N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SIGMAENV_OK;
}
