// sigmaenv_step_wave.inc -- the fused step kernel, ONE WAVEFRONT PER TILE, no workgroup barrier anywhere (included by sigmaenv.hip).
//
// A tile is G environments x N agents = S <= 64 agent slots and belongs to one wavefront from the first load to the last store; the
// wavefronts of a workgroup never synchronise.  With 16 agents and one environment per wavefront a launch of 4096 environments is 4096
// independent wavefronts (4 per SIMD, all resident at once): while one waits for memory the others issue, and no phase parks three
// quarters of a workgroup behind a barrier as the workgroup-per-tile form did (81.9k shader cycles per tile there, of which B2 43k
// VALU-bound and the rest latency-bound on one wavefront of four -- profiles/r02_a_phase_cycles.txt).
//
// Phases of a wavefront (reference citations relative to /root/reference/sigmarl, see sigmaenv.hip / sigmaenv_device.h):
//   A   two lanes per agent : action clamp + bicycle Euler step; the two independent tan -> atan chains (old / new steering angle) and the
//                             two sine / cosine pairs run side by side in the lane pair (DPP quad swap), vertices, state write-out
//   S   the pruned scan as a balanced work list: lane per (agent, polyline) for the candidate chunks, then lane per (task, chunk) item,
//                             per-task results merged by LDS atomics (see scan_tile_balanced).  Segments within the circumradius are
//                             appended to ONE list per tile in LDS for the edge tests.
//   E   lane per listed segment: code and end points from LDS (the scan stored them beside the entry), the four rectangle edges' crossing tests (interX) ORed
//                             into the agent's flag, in passes of 64 entries; a tile whose list overflowed: lane per (agent, side, edge) over every segment of the
//                             boundaries with a near one
//   B1  lane per unordered agent pair: mutual distance, rectangle-rectangle tests of close pairs
//   C   lane per agent      : reward, short-term path, done / counters by ballots
//   D   lane per item       : observation rows (observe_tile<WAVE>)
//   R   fused device-side resets of the finished envs (auto_reset_tile<WAVE>)
// Exactness of the scan is unchanged (DESIGN.md "Pruned scan"): the same candidate chunks, the same per-segment arithmetic; "first minimal
// index" is the 64-bit minimum over (distance bits, index).

__device__ __forceinline__ float dpp_swap1(float v) {  // value of the other lane of the pair (quad_perm [1, 0, 3, 2])
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}

// K1 with the trigonometric chains of WorldCustom.step + KinematicBicycleModel (helper_training.py:797-861, dynamics.py:62-192) laid out
// over a lane pair: `par` (wavefront-uniform) = the agent owns lanes (2 sl, 2 sl + 1), h = lane & 1.  Same operations and operation
// order per value as bicycle_step / rect_vertices; both lanes end up with every result.
__device__ __forceinline__ void bicycle_step_pair(const sigmaenv_config_t& c, const CfgDerived& dv, float s[8], float u0, float u1, float uc[2], float cs_yaw[2], bool par, int h, float cr[3]) {
  const float a0 = clampf(u0, -c.max_speed, c.max_speed);
  const float a1 = clampf(u1, -c.max_steering, c.max_steering);
  uc[0] = a0;
  uc[1] = a1;
  float x = s[0], y = s[1], psi = s[2], v = s[3], delta = s[4];
  float u_acc = (a0 - v) / c.dt;
  float u_sr = (a1 - delta) / c.dt;
  u_acc = clampf(u_acc, c.min_acc, c.max_acc);
  u_sr = clampf(u_sr, c.min_steering_rate, c.max_steering_rate);
  const float l_wb = dv.l_wb, k_beta = dv.k_beta;  // (float)(l_f + l_r), (float)(l_r / (l_f + l_r)) in float64: kernel-uniform, derived once on the host (derive_config)
  const float dt = c.dt;
  float delta_new = delta + dt * u_sr;
  delta_new = remainder_pos(delta_new + PI32, TWO_PI32) - PI32;
  // stage 1: tan / atan of the old and of the new steering angle
  float tan_d, beta, beta1, tan_new;
  {
    const float x1 = (par && h) ? delta_new : delta;
    const float t1 = cr_tan(x1);
    const float b1 = cr_atan(k_beta * t1);
    if (par) {
      const float t1o = dpp_swap1(t1), b1o = dpp_swap1(b1);
      tan_d = h ? t1o : t1;
      tan_new = h ? t1 : t1o;
      beta = h ? b1o : b1;
      beta1 = h ? b1 : b1o;
    } else {
      tan_d = t1;
      beta = b1;
      tan_new = cr_tan(delta_new);
      beta1 = cr_atan(k_beta * tan_new);
    }
  }
  // stage 2: sin / cos of (psi + beta), cos of beta
  float s0, c0, cosb;
  {
    const float x2 = (par && h) ? beta : (psi + beta);
    float sa, ca;
    cr_sincos(x2, sa, ca);
    if (par) {
      const float so = dpp_swap1(sa), co = dpp_swap1(ca);
      s0 = h ? so : sa;
      c0 = h ? co : ca;
      cosb = h ? ca : co;
    } else {
      s0 = sa;
      c0 = ca;
      cosb = cr_cos(beta);
    }
  }
  const float dx0 = v * c0;
  const float dx1 = v * s0;
  const float dx2 = (v / l_wb) * tan_d * cosb;
  x = x + dt * dx0;
  y = y + dt * dx1;
  psi = psi + dt * dx2;
  v = v + dt * u_acc;
  const float course = psi + beta1;
  // stage 3: sin / cos of the course (velocity) and of the new yaw (vertices)
  float s1, c1, sy, cy;
  {
    const float x3 = (par && h) ? psi : course;
    float sa, ca;
    cr_sincos(x3, sa, ca);
    if (par) {
      const float so = dpp_swap1(sa), co = dpp_swap1(ca);
      s1 = h ? so : sa;
      c1 = h ? co : ca;
      sy = h ? sa : so;
      cy = h ? ca : co;
    } else {
      s1 = sa;
      c1 = ca;
      cr_sincos(psi, sy, cy);
    }
  }
  s[0] = x; s[1] = y; s[2] = psi; s[3] = v; s[4] = delta_new;
  s[5] = v * c1;
  s[6] = v * s1;
  s[7] = beta1;
  cs_yaw[0] = cy;
  cs_yaw[1] = sy;
  cr[0] = tan_new; cr[1] = c1; cr[2] = s1;  // for the next step of the same launch (bicycle_step_pair_carried)
}

// The same step for the 2nd, 3rd, ... step of ONE launch (sigmaenv_step_autoreset_n).  Three of the step's quantities are functions of the state the previous step of
// the launch left behind and were computed there already: tan(delta) and beta = atan(k tan(delta)) (delta is last step's delta_new: tan_d and state[7]), and
// sin / cos(psi + beta) (last step's sin / cos of the course); a re-placed agent has delta = beta = 0 and the start table's cos / sin of its yaw.  With them carried
// (Smem::carry) the middle one of the three lane-pair stages disappears: stage 1 evaluates sin / cos of beta (lane 0: for cos(beta)) beside sin / cos of delta_new (lane 1:
// tan, then atan), stage 3 is unchanged.  Same functions of the same arguments: bit-identical to bicycle_step_pair (tests/test_gpu_nstep.py holds the T-step launch to T
// single launches, which take the full path).  cr: in = (tan_d, c0, s0) of the old state, out = the new state's.
__device__ __forceinline__ void bicycle_step_pair_carried(const sigmaenv_config_t& c, const CfgDerived& dv, float s[8], float u0, float u1, float uc[2], float cs_yaw[2], int h, float cr[3]) {
  const float a0 = clampf(u0, -c.max_speed, c.max_speed);
  const float a1 = clampf(u1, -c.max_steering, c.max_steering);
  uc[0] = a0;
  uc[1] = a1;
  float x = s[0], y = s[1], psi = s[2], v = s[3], delta = s[4];
  const float beta = s[7];
  float u_acc = (a0 - v) / c.dt;
  float u_sr = (a1 - delta) / c.dt;
  u_acc = clampf(u_acc, c.min_acc, c.max_acc);
  u_sr = clampf(u_sr, c.min_steering_rate, c.max_steering_rate);
  const float l_wb = dv.l_wb, k_beta = dv.k_beta;  // (float)(l_f + l_r), (float)(l_r / (l_f + l_r)) in float64: kernel-uniform, derived once on the host (derive_config)
  const float dt = c.dt;
  float delta_new = delta + dt * u_sr;
  delta_new = remainder_pos(delta_new + PI32, TWO_PI32) - PI32;
  // stage 1: sin / cos of (lane 1) the new steering angle -> tan -> atan, (lane 0) the sideslip angle -> cos(beta)
  double sd, cd;
  sigma_sincos_f64((double)(h ? delta_new : beta), &sd, &cd);
  const float t1 = (float)(sd / cd);         // cr_tan(delta_new) in lane 1
  const float b1 = cr_atan(k_beta * t1);     // beta1 in lane 1
  const float cb = (float)cd;                // cr_cos(beta) in lane 0
  const float t1o = dpp_swap1(t1), b1o = dpp_swap1(b1), cbo = dpp_swap1(cb);
  const float tan_new = h ? t1 : t1o, beta1 = h ? b1 : b1o, cosb = h ? cbo : cb;
  const float tan_d = cr[0], c0 = cr[1], s0 = cr[2];
  const float dx0 = v * c0;
  const float dx1 = v * s0;
  const float dx2 = (v / l_wb) * tan_d * cosb;
  x = x + dt * dx0;
  y = y + dt * dx1;
  psi = psi + dt * dx2;
  v = v + dt * u_acc;
  const float course = psi + beta1;
  // stage 3: sin / cos of the course (velocity) and of the new yaw (vertices)
  float sa, ca;
  cr_sincos(h ? psi : course, sa, ca);
  const float so = dpp_swap1(sa), co = dpp_swap1(ca);
  const float s1 = h ? so : sa, c1 = h ? co : ca, sy = h ? sa : so, cy = h ? ca : co;
  s[0] = x; s[1] = y; s[2] = psi; s[3] = v; s[4] = delta_new;
  s[5] = v * c1;
  s[6] = v * s1;
  s[7] = beta1;
  cs_yaw[0] = cy;
  cs_yaw[1] = sy;
  cr[0] = tan_new; cr[1] = c1; cr[2] = s1;
}

// get_rectangle_vertices (helper_scenario.py:695-826) from a known cos / sin of the yaw
__device__ __forceinline__ void rect_vertices_cs(const CfgDerived& dv, float px, float py, float cs, float sn, float* v /*5x2*/) {
  const float lh = dv.lh, wh = dv.wh;  // (float)(length / 2), (float)(width / 2) in float64 (derive_config)
  const float nsn = -sn;
  const float bx[5] = {lh, lh, -lh, -lh, lh};
  const float by[5] = {wh, -wh, -wh, wh, wh};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    v[2 * k] = (cs * bx[k] + nsn * by[k]) + px;
    v[2 * k + 1] = (sn * bx[k] + cs * by[k]) + py;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// S: the pruned scan of a tile as a balanced work list.  update_distances (world_state_rt.py:582-656) and the candidate segments of
// the boundary part of update_collisions (world_state_rt_sim.py:398-411).
//   S1  lane per (agent, polyline) "task": the candidate chunks (mask stages, as in the block kernels) -> one work item per
//       (task, chunk of SIGMAENV_CHUNK segments) appended to a list in LDS (offsets by a wavefront prefix sum)
//   S2  lane per ITEM: the chunk's segments against the task's query points; partial results merge into per-task accumulators with
//       LDS atomics: the centre-point query as min over (distance bits << 32 | segment index) -- distances are >= 0, so the unsigned order
//       of the bit patterns is the numeric order and the 64-bit minimum is "smallest distance, lowest index" (torch.min, helper_scenario.py:883);
//       the corner queries as min over the bits of the SQUARED distance (value only, square root after the reduction)
//   S3  lane per task: accumulators -> dref / dleft / dright / closest indices
// Every lane of S2 carries the same amount of work whatever the distribution of candidates over the agents (a lane that walked its own
// task's chunks made the whole wavefront wait for the task with the most candidates: 2.56e7 VALU instructions per 4096 envs, r02_b).
// ---------------------------------------------------------------------------------------------------------------------
// inclusive prefix sum over the 64 lanes on the VALU's data-parallel primitives (no LDS round trips): shifts within the rows of 16 lanes,
// then the row totals broadcast into the following rows (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3); lanes without a
// source add the identity 0.  All lanes must be active.
__device__ __forceinline__ int wave_inclusive_sum(int v, int /*lane*/) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

struct ScanItemOut {
  float best;
  int bk;
  float bs0, bs1, bs2, bs3;
  unsigned near_bits;  // bit u: segment u of the lane's run lies within the circumradius (boundaries only)
  Seg4 sg[SIGMAENV_CHUNK];  // the lane's run of segments as loaded (the first SEGS of them): the listed ones' end points go to LDS for phase E
};

// one chunk of one task: its SIGMAENV_CHUNK segments against the centre point (and, for a boundary, the four corner query points).
// poly_off: float offset of the task's polyline in the shared map table (32-bit: the loads take the table base from scalar registers)
// SEGS: the lane takes SEGS consecutive segments of the chunk starting at segment u0 (the whole chunk, or -- in a sparsely filled last
// round -- a half / a quarter of it, the other lanes of the item taking the rest; the partial results merge through the same atomics)
template <bool FASTDIV, int SEGS>
__device__ __forceinline__ void scan_chunk(const DevMap& m, const Smem& s, int sl, int pl, unsigned poly_off, int npt, int ch, int u0, bool first_of_env,
                                           const float near_thr, ScanItemOut& o) {
  const float cgx = s.st[sl * 8], cgy = s.st[sl * 8 + 1];
  const unsigned kmax = (unsigned)(npt - 2 < 0 ? 0 : npt - 2);
  Seg4 (&sg)[SIGMAENV_CHUNK] = o.sg;
#pragma unroll
  for (int u = 0; u < SIGMAENV_CHUNK; ++u) {
    const unsigned k = min((unsigned)(ch * SIGMAENV_CHUNK + u0 + u), kmax);
    sg[u] = u < SEGS ? *reinterpret_cast<const Seg4*>(m.center + (poly_off + 2u * k)) : Seg4{0.f, 0.f, 0.f, 0.f};
  }
  // corner query points: agent 0 of every env still sees last step's vertices (world_state_rt_sim.py:439-448)
  const float* qv = first_of_env ? (s.vold + sl * 10) : (s.vnew + sl * 10);
  float q0x = 0.f, q0y = 0.f, q1x = 0.f, q1y = 0.f, q2x = 0.f, q2y = 0.f, q3x = 0.f, q3y = 0.f;
  if (pl != 0) { q0x = qv[0]; q0y = qv[1]; q1x = qv[2]; q1y = qv[3]; q2x = qv[4]; q2y = qv[5]; q3x = qv[6]; q3y = qv[7]; }
  o.bs0 = INFINITY; o.bs1 = INFINITY; o.bs2 = INFINITY; o.bs3 = INFINITY;
  unsigned near_bits = 0u;
  // The centre query stays in the SQUARED domain per segment; the lane takes ONE correctly rounded root, of its smallest radicand.  Exact, incl. the reference's tie
  // rule (torch.min returns the FIRST index of the smallest ROOTED distance, and different radicands can share a root): for fp32 d with successor d+,
  // sqrt_rn(z) > d  <=>  z > d d+  (no fp32 z lies in (d d+, (d + ulp / 2)^2], and sqrt(z) is never a rounding midpoint), and fma(-d+, d, z) has the sign of
  // z - d d+ exactly.  So with d = sqrt_rn(min z): segment u's rooted distance equals the lane's minimum iff fma(-d+, d, z_u) <= 0 -- the lowest such u is what the
  // sequential `d_u < best` scan of rooted distances selects -- and "d_u > near_thr" is fma(-thr+, thr, z_u) > 0.  (A NaN radicand is never selected and counts as
  // near, as before; an empty / non-finite lane leaves bk unset.)
  const float near_thr_up = __uint_as_float(__float_as_uint(near_thr) + 1u);
  float zc[SEGS];
  float zbest = INFINITY;
#pragma unroll
  for (int u = 0; u < SEGS; ++u) {
    const int k = ch * SIGMAENV_CHUNK + u0 + u;
    const bool valid = k + 1 < npt;
    const float ax = sg[u].ax, ay = sg[u].ay;
    const float lx = sg[u].bx - ax, ly = sg[u].by - ay;
    const float len2 = lx * lx + ly * ly;
    const float rcp = FASTDIV ? shared_rcp(len2) : 0.0f;
    const float z0 = point_segment_sq_t<FASTDIV>(cgx, cgy, ax, ay, lx, ly, len2, rcp);
    zc[u] = z0;
    if (valid && z0 < zbest) zbest = z0;
    if (pl != 0) {
      const float v0 = point_segment_sq_t<FASTDIV>(q0x, q0y, ax, ay, lx, ly, len2, rcp);
      const float v1 = point_segment_sq_t<FASTDIV>(q1x, q1y, ax, ay, lx, ly, len2, rcp);
      const float v2 = point_segment_sq_t<FASTDIV>(q2x, q2y, ax, ay, lx, ly, len2, rcp);
      const float v3 = point_segment_sq_t<FASTDIV>(q3x, q3y, ax, ay, lx, ly, len2, rcp);
      if (valid) {
        o.bs0 = fmin_nc(o.bs0, v0); o.bs1 = fmin_nc(o.bs1, v1); o.bs2 = fmin_nc(o.bs2, v2); o.bs3 = fmin_nc(o.bs3, v3);
        // only a segment within the rectangle's circumradius of the (new) centre can cross an edge (DESIGN.md "Pruned scan")
        if (!(fmaf(-near_thr_up, near_thr, z0) > 0.0f)) near_bits |= 1u << u;
      }
    }
  }
  {
    const float d = sqrtf(zbest);
    const float d_up = __uint_as_float(__float_as_uint(d) + 1u);
    o.best = d; o.bk = 0x7FFFFFFF;
#pragma unroll
    for (int u = SEGS - 1; u >= 0; --u) {
      const int k = ch * SIGMAENV_CHUNK + u0 + u;
      if (k + 1 < npt && fmaf(-d_up, d, zc[u]) <= 0.0f) o.bk = k;
    }
  }
  o.near_bits = near_bits;  // (the caller appends them to the tile's list: scan_tile_balanced)
  if (near_bits) atomicAdd(&s.nearn[sl * 2 + (pl - 1)], (int)__popc(near_bits));  // (no value returned: the count tells the overflow walk of phase E which boundaries have a near segment at all)
}
__device__ __forceinline__ void scan_merge(const Smem& s, int sl, int pl, const ScanItemOut& o) {
  if (o.bk != 0x7FFFFFFF) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(o.best) << 32) | (unsigned)o.bk;
    atomicMin(&s.acc64[sl * 3 + pl], key);
  }
  if (pl != 0) {
    uint32_t* a = s.acc32 + (sl * 2 + (pl - 1)) * 4;
    atomicMin(&a[0], __float_as_uint(o.bs0)); atomicMin(&a[1], __float_as_uint(o.bs1));
    atomicMin(&a[2], __float_as_uint(o.bs2)); atomicMin(&a[3], __float_as_uint(o.bs3));
  }
}

template <bool FASTDIV>
__device__ __forceinline__ void scan_tile_balanced(const DevMap& m, const CfgDerived& dv, const DevBufs& g, const Smem& s, const Tile& t, int G, int lane) {
  // tasks are numbered pl * SG + sl with SG = the slots of a FULL tile (kernel-uniform: division by multiplication); slots beyond a ragged
  // last tile stay idle
  const int N = t.N, slots = t.slots, SG = G * N, n_tasks = SG * 3, cap = ITEM_CAP(SG), near_cap = SG * NEAR_CAP, xy_cap = Smem::near_xy_cap(SG, N);
  const float near_thr = m.rect_radius + 1e-4f;
  // The tile's list of near segments: the wavefront owns the tile, so the position of a lane's entries is the number listed so far (wavefront-uniform, in a register)
  // plus a prefix sum over the lanes of the pass -- no LDS counter.  (One counter per tile bumped by an atomic add per chunk serialises: up to 64 lanes on ONE address,
  // S2 +2,700 cycles per tile-step against the per-boundary counters it replaced, more than phase E gains; profiles/edge_list_phase_cycles.txt.)
  // An entry is its code and, for the first xy_cap entries, the segment's end points as the lane holds them (one 16-byte store): phase E then needs no map load.
  int near_total = 0;
  auto near_append = [&](unsigned nb, int code0, const Seg4 (&sg)[SIGMAENV_CHUNK]) {  // all lanes; nb = 0: nothing to list
    const int cnt = (int)__popc(nb);
    const int incl = wave_inclusive_sum(cnt, lane);
    int slot = near_total + incl - cnt;
    near_total += __builtin_amdgcn_readlane(incl, 63);
#pragma unroll
    for (int u = 0; u < SIGMAENV_CHUNK; ++u) {
      if ((nb >> u) & 1u) {
        if (slot < near_cap) s.nearl[slot] = (uint16_t)(code0 + u);
        if (slot < xy_cap) s.nearxy[slot] = make_float4(sg[u].ax, sg[u].ay, sg[u].bx, sg[u].by);
        ++slot;
      }
    }
  };
  // ---- S1: candidate chunks per task
  for (int base = 0; base < n_tasks; base += 64) {
    // lane -> task: left boundaries, right boundaries, THEN the centre lines.  The work list is filled in lane order, so the centre-line items (one query point
    // instead of five) end up at its tail: the last, sparsely filled round of S2 is then a centre-line-only round that skips the corner queries altogether
    // (with the centre lines in front the first round mixed 30 cheap items with 34 full ones at the full round's price, and the tail round paid for five queries)
    const int tl = base + lane;
    const int grp_raw = fdiv(tl, g.mSG), sl_raw = tl - grp_raw * SG;
    const int pl_raw = grp_raw >= 2 ? 0 : grp_raw + 1;
    const int tpm = pl_raw * SG + sl_raw;  // pl-major task number (the work list's item code)
    const bool act = tl < n_tasks && sl_raw < slots;
    const int pl = act ? pl_raw : 0, sl = act ? sl_raw : 0;
    const int task = sl * 3 + pl;
    unsigned long long mk = 0ull;
#ifdef SIGMAENV_PROFILE
    int lvl_prof = 0;
#endif
    if (act) {
      MaskTask mt;
      mask_stage1(m, mt, task, s.path[sl], s.cp[task]);
      mask_stage2<true>(m, s, mt, true, N);
#ifdef SIGMAENV_PROFILE
      lvl_prof = mt.lvl;
#endif
      const float px = mt.px, py = mt.py, T2 = mt.T2;
      const int nch = mt.nch;
      mk = neigh_candidates(m, mt);  // the boxes of the listed neighbour chunks
      if (mt.own_within && mt.own < nch) mk |= 1ull << mt.own;  // the chunk of last step's closest segment is within T by construction
      if (!mt.fast) {  // far from the own path: two-level search over all boxes
        const float4* gbox = m.group_box + ((size_t)mt.path * 3 + pl) * 8;
        unsigned gm = 0u;
#pragma unroll 1
        for (int gidx = 0; gidx < 8; ++gidx) {
          if (gidx * 8 < nch && box_within(gbox[gidx], px, py, T2)) gm |= 1u << gidx;
        }
        while (gm) {
          const int gidx = __ffs((int)gm) - 1;
          gm &= gm - 1u;
#pragma unroll 1
          for (int q = 0; q < 8; ++q) {
            const int cidx = gidx * 8 + q;
            if (cidx < nch && box_within(mt.box[cidx], px, py, T2)) mk |= 1ull << cidx;
          }
        }
      }
      s.npts[task] = mt.npt;
      s.acc64[task] = ~0ull;
      if (pl != 0) {
        const int bt = sl * 2 + (pl - 1);
        uint32_t* a = s.acc32 + bt * 4;
        a[0] = 0x7F800000u; a[1] = 0x7F800000u; a[2] = 0x7F800000u; a[3] = 0x7F800000u;
        s.nearn[bt] = 0;
      }
    }
#ifdef SIGMAENV_PROFILE
    if (g.dbg_ts && lane == 0 && base == 0) g.dbg_ts[(size_t)t.env0 / (size_t)G * 16 + 10] = __builtin_readcyclecounter();  // end of S1 (candidate masks)
    {  // neighbour-level statistics of the tile: tasks beyond the near level, passes with such a task, tasks at the tight level, the first agent's among the first
      const unsigned long long bfar = __ballot(act && lvl_prof >= 2), btight = __ballot(act && lvl_prof == 0);
#ifndef SIGMAENV_PROFILE_RT
      if (g.dbg_ts && lane == 0) {
        unsigned long long* row = g.dbg_ts + (size_t)t.env0 / (size_t)G * 16;
        row[12] += (unsigned long long)__popcll(bfar); row[13] += bfar ? 1ull : 0ull; row[14] += (unsigned long long)__popcll(btight);
        row[15] += (unsigned long long)__popcll(bfar & 0x0000000100010001ull);
      }
#endif
    }
#endif
    // work list + S2 in rounds: one round unless the tile has more candidate chunks than the list holds (agents far from their paths)
    bool pending = act;
    do {
      const int cnt = pending ? __popcll(mk) : 0;
      const int incl = wave_inclusive_sum(cnt, lane);
      const int off = incl - cnt;
      const bool listed = pending && off + cnt <= cap;  // (a single task never exceeds the list: at most 64 chunks, and ITEM_CAP >= 64 -- the first pending task of a round always fits)
      if (listed) {
        int j = off;
        while (mk) {
          const int ch = __ffsll((long long)mk) - 1;
          mk &= mk - 1ull;
          s.items[j++] = (uint16_t)((tpm << 6) | ch);
        }
      }
      const unsigned long long unl = __ballot(pending && !listed);  // offsets grow with the lane: the listed tasks are a prefix
      const int total = unl ? __builtin_amdgcn_readlane(off, __builtin_amdgcn_readfirstlane(__ffsll((long long)unl) - 1)) : __builtin_amdgcn_readlane(incl, 63);
      pending = pending && !listed;
      wave_sync();
#ifdef SIGMAENV_PROFILE
      if (g.dbg_ts && lane == 0) {  // work-list statistics of the tile: items, rounds
        g.dbg_ts[(size_t)t.env0 / (size_t)G * 16 + 8] += (unsigned long long)total;
        g.dbg_ts[(size_t)t.env0 / (size_t)G * 16 + 9] += 1ull;
      }
#endif
      // ---- S2: one lane per listed (task, chunk); a last round that fills at most half / a quarter of the wavefront gives every item two /
      // four lanes (two segments / one segment each) instead of leaving the lanes idle
      auto item_part = [&](int it, auto segs_tag, int u0, unsigned& nb, int& code0, Seg4 (&sgo)[SIGMAENV_CHUNK]) {
        constexpr int SEGS = decltype(segs_tag)::value;
        const unsigned code = s.items[it];
        const int tpm2 = (int)(code >> 6), ch = (int)(code & 63u);
        const int pl2 = fdiv(tpm2, g.mSG), sl2 = tpm2 - pl2 * SG;
        const bool first = (sl2 - fdiv(sl2, g.mN) * N) == 0;
        ScanItemOut o;
        const unsigned poly_off = (unsigned)pl2 * (unsigned)m.poly_stride + (unsigned)s.path[sl2] * (unsigned)(m.P * 2);
        scan_chunk<FASTDIV, SEGS>(m, s, sl2, pl2, poly_off, s.npts[sl2 * 3 + pl2], ch, u0, first, near_thr, o);
        scan_merge(s, sl2, pl2, o);
        nb = o.near_bits;
#pragma unroll
        for (int u = 0; u < SIGMAENV_CHUNK; ++u) sgo[u] = o.sg[u];
        code0 = ((sl2 * 2 + (pl2 - 1)) << 8) | (ch * SIGMAENV_CHUNK + u0);  // (boundary task << 8) | first segment of the lane's run
      };
      int it0 = 0;
      for (; it0 + 64 <= total; it0 += 64) {
        unsigned nb = 0u;
        int code0 = 0;
        Seg4 sgo[SIGMAENV_CHUNK];
        item_part(it0 + lane, std::integral_constant<int, SIGMAENV_CHUNK>{}, 0, nb, code0, sgo);
        near_append(nb, code0, sgo);
      }
      const int rem = total - it0;
      unsigned nb = 0u;
      int code0 = 0;
      Seg4 sgo[SIGMAENV_CHUNK] = {};
      if (rem > 32) {
        if (lane < rem) item_part(it0 + lane, std::integral_constant<int, SIGMAENV_CHUNK>{}, 0, nb, code0, sgo);
      } else if (rem > 16) {
        if ((lane >> 1) < rem) item_part(it0 + (lane >> 1), std::integral_constant<int, SIGMAENV_CHUNK / 2>{}, (lane & 1) * (SIGMAENV_CHUNK / 2), nb, code0, sgo);
      } else if (rem > 0) {
        if ((lane >> 2) < rem) item_part(it0 + (lane >> 2), std::integral_constant<int, SIGMAENV_CHUNK / 4>{}, (lane & 3) * (SIGMAENV_CHUNK / 4), nb, code0, sgo);
      }
      if (rem > 0) near_append(nb, code0, sgo);
      wave_sync();
    } while (__any(pending));
  }
#ifdef SIGMAENV_PROFILE
  if (g.dbg_ts && lane == 0) g.dbg_ts[(size_t)t.env0 / (size_t)G * 16 + 11] = __builtin_readcyclecounter();  // end of S2 (all rounds)
#endif
  if (lane == 0) *s.nearc = near_total;  // for phase E
  // ---- S3: results per task
  const float wh = dv.wh;
  for (int tpm = lane; tpm < n_tasks; tpm += 64) {
    const int pl = fdiv(tpm, g.mSG), sl = tpm - pl * SG;
    if (sl >= slots) continue;
    const unsigned long long key = s.acc64[sl * 3 + pl];
    const float best = __uint_as_float((uint32_t)(key >> 32));
    const int bk = (int)(uint32_t)key;
    s.cp[sl * 3 + pl] = bk + 1;
    if (pl == 0) {
      s.dref[sl] = best;
    } else {
      float* dst = (pl == 1 ? s.dleft : s.dright) + sl * 5;
      dst[0] = best - wh;  // world_state_rt.py:608-610
    }
  }
  // the corner queries' roots (one correctly rounded sqrtf of the reduced squared distance per (boundary task, corner)), spread over all lanes: two passes of
  // one root per lane for a 16-agent tile instead of four roots in each of the 32 boundary lanes of the pass above
  for (int w = lane; w < slots * 8; w += 64) {
    const int bt = w >> 2, q = w & 3, sl = bt >> 1;  // bt = 2 sl + (0 left | 1 right): the accumulators are laid out [bt][corner]
    float* dst = ((bt & 1) ? s.dright : s.dleft) + sl * 5;
    dst[1 + q] = sqrtf(__uint_as_float(s.acc32[w]));
  }
}

// (i, j), i < j, of the u-th unordered agent pair of an env as i | j << 8: a compile-time table for the fixed-shape instantiations (the
// generic ones build it in LDS)
template <int SN>
struct PairTable {
  uint16_t v[SN * (SN - 1) / 2 > 0 ? SN * (SN - 1) / 2 : 1];
  constexpr PairTable() : v() {
    int k = 0;
    for (int i = 0; i < SN - 1; ++i)
      for (int j = i + 1; j < SN; ++j) v[k++] = (uint16_t)(i | (j << 8));
  }
};
template <int SN>
__device__ const PairTable<SN> kPairTable{};

#ifndef STEP_WAVE_MIN_WAVES
#define STEP_WAVE_MIN_WAVES 4  // <= 128 VGPRs: four wavefronts per SIMD
#endif
// blockDim.x = 64 * (wavefronts per workgroup); every wavefront owns tile blockIdx.x * waves + wave and its own slice of the dynamic LDS
// SN > 0: instantiations for fixed tile shapes -- SN agents, SG envs per wavefront, 2 observed neighbours (obs_dim 32): every count,
// stride, LDS offset and index divisor of the tile is a compile-time constant (16 x 1 is the metric's own shape; the generic
// instantiations, SN = 0, read them from the config and divide through the precomputed multipliers).  -10 % instructions, a third of the
// scalar-register spills, 0.0490 -> 0.0427 ms per step at 16 x 4096.
// ALL arguments of the step kernel, passed as one struct by value: the kernarg segment then holds exactly this layout, and the kernel reads it
// through a pointer (see the step loop below) instead of keeping ~130 scalar registers' worth of arguments alive
struct StepKernArgs {
  DevMap m;
  DevBufs g;
  const float* actions_base;  // step t reads actions_base + t * act_stride
  float* slab_base;           // step t records into slab_base + t * slab_stride (nullptr: no record)
  size_t act_stride, slab_stride;
  uint64_t seed, counter0;    // step t draws its resets from (seed, counter0 + t)
  int G_arg, tile_lds, path_first, path_count, n_steps;
};
template <class T>
__device__ __forceinline__ T* as_global(T* p) {  // a pointer read from the kernarg segment by hand is generic: tell the compiler it is global memory
  return (T*)(__attribute__((address_space(1))) T*)p;
}
// The map and buffer tables (~50 pointers) are re-read from the kernarg segment at the top of EVERY step of the in-kernel step loop, through a
// pointer the compiler cannot see through: as plain by-value arguments they are loop invariants, all live across the whole loop body, and the
// register allocator spilled 187 scalars into vector lanes and 271 vector registers to scratch (1072 B per lane) -- against 57 / 0 for the
// single-step body, where each pointer dies after its last use.  ~10 wide scalar loads per step (scalar cache hits) buy that back.
#define SIGMA_COPY_GLOBAL(dst, src, f) dst.f = as_global(src.f)
__device__ __forceinline__ void load_step_tables(const __attribute__((address_space(4))) StepKernArgs* ka, DevMap& m, DevBufs& g) {
  SIGMA_COPY_GLOBAL(m, ka->m, center); SIGMA_COPY_GLOBAL(m, ka->m, left); SIGMA_COPY_GLOBAL(m, ka->m, right); SIGMA_COPY_GLOBAL(m, ka->m, yaw);
  SIGMA_COPY_GLOBAL(m, ka->m, n_center); SIGMA_COPY_GLOBAL(m, ka->m, n_left); SIGMA_COPY_GLOBAL(m, ka->m, n_right); SIGMA_COPY_GLOBAL(m, ka->m, is_loop);
  SIGMA_COPY_GLOBAL(m, ka->m, chunk_box); SIGMA_COPY_GLOBAL(m, ka->m, group_box); SIGMA_COPY_GLOBAL(m, ka->m, chunk_neigh); SIGMA_COPY_GLOBAL(m, ka->m, start_table);
  m.P = ka->m.P; m.n_paths = ka->m.n_paths; m.yaw_stride = ka->m.yaw_stride; m.neigh_radius = ka->m.neigh_radius; m.neigh_radius_far = ka->m.neigh_radius_far;
  m.nch = ka->m.nch; m.fast_div = ka->m.fast_div; m.rect_radius = ka->m.rect_radius; m.poly_stride = ka->m.poly_stride;
  m.n_lists = ka->m.n_lists; m.neigh_radius_tight = ka->m.neigh_radius_tight;
  m.list_first16 = ka->m.list_first16; m.list_count16 = ka->m.list_count16; m.cdf0 = ka->m.cdf0; m.cdf1 = ka->m.cdf1; m.cdf2 = ka->m.cdf2;
  SIGMA_COPY_GLOBAL(g, ka->g, state); SIGMA_COPY_GLOBAL(g, ka->g, prev_pos); SIGMA_COPY_GLOBAL(g, ka->g, vertices); SIGMA_COPY_GLOBAL(g, ka->g, short_term);
  SIGMA_COPY_GLOBAL(g, ka->g, dist_ref); SIGMA_COPY_GLOBAL(g, ka->g, dist_left); SIGMA_COPY_GLOBAL(g, ka->g, dist_right); SIGMA_COPY_GLOBAL(g, ka->g, dist_bound);
  SIGMA_COPY_GLOBAL(g, ka->g, dist_agents); SIGMA_COPY_GLOBAL(g, ka->g, reward); SIGMA_COPY_GLOBAL(g, ka->g, reward_info); SIGMA_COPY_GLOBAL(g, ka->g, obs);
  SIGMA_COPY_GLOBAL(g, ka->g, action); SIGMA_COPY_GLOBAL(g, ka->g, cbf_nominal); SIGMA_COPY_GLOBAL(g, ka->g, path); SIGMA_COPY_GLOBAL(g, ka->g, closest);
  SIGMA_COPY_GLOBAL(g, ka->g, nearing); SIGMA_COPY_GLOBAL(g, ka->g, timer); SIGMA_COPY_GLOBAL(g, ka->g, col_agents); SIGMA_COPY_GLOBAL(g, ka->g, col_flags);
  SIGMA_COPY_GLOBAL(g, ka->g, done); SIGMA_COPY_GLOBAL(g, ka->g, reset_mask); SIGMA_COPY_GLOBAL(g, ka->g, reset_full); SIGMA_COPY_GLOBAL(g, ka->g, fresh);
  SIGMA_COPY_GLOBAL(g, ka->g, slab); SIGMA_COPY_GLOBAL(g, ka->g, dbg_ts2); SIGMA_COPY_GLOBAL(g, ka->g, dbg_ts);
  SIGMA_COPY_GLOBAL(g, ka->g, lanelet_centers); SIGMA_COPY_GLOBAL(g, ka->g, lanelet_neigh); SIGMA_COPY_GLOBAL(g, ka->g, bnd_left);
  SIGMA_COPY_GLOBAL(g, ka->g, bnd_n_center); SIGMA_COPY_GLOBAL(g, ka->g, bnd_is_loop);
  g.n_lanelets = ka->g.n_lanelets; g.lanelet_pts = ka->g.lanelet_pts; g.bnd_poly_stride = ka->g.bnd_poly_stride; g.bnd_P = ka->g.bnd_P; g.mVT1 = ka->g.mVT1;
  g.obs_salt = 0u;  // (the step's and the resets' observations: told apart by the env's own counters)
  g.mN = ka->g.mN; g.mT1 = ka->g.mT1; g.mT2 = ka->g.mT2; g.mTP = ka->g.mTP; g.mW = ka->g.mW; g.mSG = ka->g.mSG; g.dbg_skip = ka->g.dbg_skip;
}
#undef SIGMA_COPY_GLOBAL

// VAR: the non-default observation rows (obs_flags != 0, observe_tile_variant) are compiled in -- launched for such configurations only, so that the default
// row's instantiations keep their register budget (generic: 96 VGPRs without, 121 + scratch with)
// MTVS: the mtv distance with the per-rectangle records staged once per agent (phase B1) -- its own instantiations (the metric's 16 x 1 shape), launched for
// mtv configurations only: compiled into the c2c kernel as a run-time branch the extra code cost the headline 0.5-0.7 % (block placement / instruction cache)
template <bool FASTDIV, bool PAR, int SN = 0, int SG = 0, bool VAR = false, bool MTVS = false>
__global__ void __launch_bounds__(256, STEP_WAVE_MIN_WAVES) sigmaenv_step_wave_kernel(const sigmaenv_config_t* __restrict__ cfg_dev, StepKernArgs args) {
  sigma_poison_lds();
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane0 = threadIdx.x & 63;
  {
    const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile0 = blockIdx.x * (blockDim.x >> 6) + wave0;
    if (tile0 * (SN ? SG : args.G_arg) >= cfg_dev->n_envs) return;  // (no barrier anywhere: a wavefront may leave alone)
  }
#ifdef SIGMAENV_PROFILE
#define TSW(k) do { unsigned long long* ts_ = as_global(ka->g.dbg_ts); if (ts_ && lane == 0) ts_[(size_t)tile_index * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
#define SKIP(bit) (ka->g.dbg_skip & (bit))
#else
#define TSW(k) do { } while (0)
#define SKIP(bit) false
#endif
  // profile build with -DSIGMAENV_PROFILE_RT (make prof_rt): slots 12..15 of a tile's stamp row hold the 100 MHz wall clock (s_memrealtime: the same on every XCD) at the
  // start of the step, before phase R and at the end, and the wavefront's placement (HW_ID | XCC_ID << 32) -- tools/launch_timeline.py
#if defined(SIGMAENV_PROFILE) && defined(SIGMAENV_PROFILE_RT)
#define TSRT(k) do { unsigned long long* ts_ = as_global(ka->g.dbg_ts); if (ts_ && lane == 0) ts_[(size_t)tile_index * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TSRT(k) do { } while (0)
#endif
  // n_steps > 1 (sigmaenv_step_autoreset_n): the wavefront steps ITS tile n_steps times in a row -- step t with actions_base + t * act_stride, the
  // reset stream of counter0 + t, the record row at slab_base + t * slab_stride -- exactly what n_steps launches do one after the other.  Envs never
  // read each other, so no wavefront waits for another one: the tiles drift apart, a tile with a long reset tail in one step catches up in the
  // next, and the launch ramp / tail and the host's per-step enqueue are paid once per n_steps.
  // The loop body is the single-step kernel, and it is compiled AS the single-step kernel: every input of a step -- lane and tile index, and the
  // kernarg segment with the config pointer, the map / buffer tables and the scalars -- passes through an empty asm at the top of the step, so nothing
  // in the body is a loop invariant and nothing but the step counter is live across the loop.  Left to itself the compiler hoists every invariant
  // of this 100 KB body (50 table pointers, 41 config words, all per-lane index arithmetic) out of the loop and keeps them live across it: 187
  // scalar and 271 vector spills, 1072 B of scratch per lane, against 57 / 0 / 0 for the straight-line body.  The re-derivation costs ~10 wide
  // scalar loads (scalar-cache hits) per step.
  for (int step_i = 0;; ++step_i) {
  int lane = lane0;
  unsigned long long kap = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+v"(lane));
  __builtin_assume(lane >= 0 && lane < 64);  // (the asm hides the value range: trip counts of the lane-strided loops depend on it)
  asm volatile("" : "+s"(kap));
  // (the kernarg segment holds the config pointer, then the struct)
  struct KernargLayout { const sigmaenv_config_t* cfg_dev; StepKernArgs a; };
  const __attribute__((address_space(4))) StepKernArgs* ka = (const __attribute__((address_space(4))) StepKernArgs*)(kap + __builtin_offsetof(KernargLayout, a));
  if (step_i >= ka->n_steps) break;
  // The arbiter of a SIMD serves its wavefronts oldest first: of the four tiles a SIMD steps through a T-step launch the first one ended after 0.72 of the launch, the last one
  // alone at its end (tools/launch_timeline_n.py) -- a quarter of the launch ran with three, two, one wavefront per SIMD.  A priority that FALLS with the wavefront's own
  // progress (cyclically: 3, 2, 1, 0 over four steps) lets the ones behind catch up at every step: a SIMD's wavefronts end within a step of each other.  (Finer rotations --
  // per phase, per half step -- are slower: wavefronts in lockstep contend for the same units; aligning the ends of a SIMD's wavefronts in the last steps by their
  // slot number changes nothing: what is left is the imbalance BETWEEN SIMDs; profiles/r05_wave_priority.txt.)
  if (ka->n_steps > 1) {  // (a single-step launch has no progress to compare -- and keeps the priority of every other kernel it may run beside)
    const int pr = 3 - (step_i & 3);
    switch (pr) {
      case 3: __builtin_amdgcn_s_setprio(3); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      default: __builtin_amdgcn_s_setprio(0); break;
    }
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), tile_index = blockIdx.x * (blockDim.x >> 6) + wave;
  const int tile_lds = ka->tile_lds;
  // The map / buffer tables and the launch scalars are read from the kernarg segment PER PHASE (STEP_TABLES: the pointer is laundered again, so the
  // compiler cannot merge a phase's loads with an earlier phase's and stretch their live ranges over the phases in between): ~50 pointers loaded at the
  // top of the step sat in scalar registers across the scan and were spilled into vector lanes and read back (v_readlane) all over the body.
#define STEP_KA(kav) asm volatile("" : "+s"(kap)); const __attribute__((address_space(4))) StepKernArgs* kav = (const __attribute__((address_space(4))) StepKernArgs*)(kap + __builtin_offsetof(KernargLayout, a))
#define STEP_TABLES(mv, gv)                                                                                                                 \
  DevMap mv;                                                                                                                                \
  DevBufs gv;                                                                                                                               \
  {                                                                                                                                         \
    STEP_KA(ka_);                                                                                                                           \
    load_step_tables(ka_, mv, gv);                                                                                                          \
    if (SN > 0) {                                                                                                                           \
      constexpr int SK_ = 2;                                                                                                                \
      gv.mN = magic_u32(SN); gv.mT1 = magic_u32(NS + 4 * SK_); gv.mT2 = magic_u32(SK_ + 1); gv.mTP = magic_u32(SN * (SN - 1) / 2);        \
      if (!VAR) gv.mW = magic_u32(SN * (4 + 2 * NS + 11 * SK_ + 1) + 1);                                                                  \
      gv.mSG = magic_u32((SG > 0 ? SG : 1) * SN);                                                                                         \
    }                                                                                                                                       \
  }
  // The config pointer stays a REAL `const __restrict__` kernel argument: the compiler then knows no store of the kernel touches the config and
  // reads its words with scalar loads (through a laundered pointer they became 59 vector loads per step).  What is opaque per step is the element
  // index 0 it is dereferenced at, which keeps the loads inside the loop just the same.
  int cfg_zero = 0;
  asm volatile("" : "+s"(cfg_zero));
  const sigmaenv_config_t& c = cfg_dev[cfg_zero];
  const CfgDerived& dv = reinterpret_cast<const DevConfig*>(cfg_dev)[cfg_zero].d;  // (the device copy of the config is a DevConfig: sigmaenv_create)
  const int G = SN ? SG : ka->G_arg;
  Tile t(c, G, tile_index);
  if (SN > 0) {
    constexpr int SK = 2;
    t.N = SN; t.K = SK;
    if (!VAR) { t.D = 4 + 2 * NS + 11 * SK; t.DL = t.D; }  // (VAR: the configured row's width, from the Tile constructor)
    if (SG == 1) { t.nenv = 1; t.env0 = tile_index; }
    t.slots = t.nenv * SN; t.a0 = (size_t)t.env0 * SN;
  }
  const int N = t.N;
  char* base = smem_raw + (size_t)wave * tile_lds;
  Smem s(base, G * N, N, t.K, t.DL, true);
  unsigned long long* s_mask = reinterpret_cast<unsigned long long*>(base + ((Smem::bytes(G * N, N, t.K, t.DL, true) + 15) & ~(size_t)15));
  int* s_full = reinterpret_cast<int*>(s_mask + G);
  int* s_any = s_full + G;
  s.nearc = s_any + 1;  // (the word between the any-reset flag and the reset's env list, which starts at s_any + 2: free in every phase)
  int* s_tim = reinterpret_cast<int*>(base + ((Smem::bytes(G * N, N, t.K, t.DL, true) + 15) & ~(size_t)15) + 16 * (size_t)G + 16);  // [G][4]: timer rows between the steps of one launch
  // The first step of a launch reads the tile from HBM, the last one writes it back; in between the tile lives in LDS (it is all there after a
  // step: state, vertices, closest indices, short-term path, path row, timers) and only the record row of the step, and whatever a reset
  // re-places, goes to HBM.  Same values either way: the steps of one launch see exactly what separate launches would have read back.
  const bool first = step_i == 0, last = step_i + 1 >= ka->n_steps;
  TSW(0);
  if (first) TSRT(12);  // (a T-step launch: the wavefront's start of the launch; slot 14 holds the end of its last step)
#if defined(SIGMAENV_PROFILE) && defined(SIGMAENV_PROFILE_RT)
  { unsigned long long* ts_ = as_global(ka->g.dbg_ts); if (ts_ && lane == 0) ts_[(size_t)tile_index * 16 + 15] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32); }
#endif
  if (SN == 0 && step_i == 0) {  // pair table rows: row i holds (i, i+1) .. (i, N-1)
    for (int i = lane; i < N - 1; i += 64) {
      const int off = i * (2 * N - i - 1) / 2;
      for (int j = i + 1; j < N; ++j) s.pidx[off + j - i - 1] = (uint16_t)(i | (j << 8));
    }
  }
  // ---- A: dynamics + vertices; two lanes per agent when the tile has at most 32 slots -----------------------------------------
  {
    STEP_TABLES(m, g);
    STEP_KA(ka_a);
    const float* __restrict__ actions = as_global(ka_a->actions_base) + (size_t)step_i * ka_a->act_stride;
    constexpr bool par = PAR;  // the host instantiates PAR = (2 G N <= 64)
    const int sl_raw = par ? (lane >> 1) : lane, h = par ? (lane & 1) : 0;
    const bool act = sl_raw < t.slots;
    const int sl = act ? sl_raw : 0;
    const size_t gi = t.a0 + sl;
    float st[8], uc[2], csy[2];
    // every load of the phase is requested first (the stores below would otherwise fence the later loads behind them)
    const float2 u = reinterpret_cast<const float2*>(actions)[gi];
    float4 s0, s1;
    int pth, cp0, cp1, cp2;
    float2 vo[5], pp, spo[NS];
    int4 tm;
    if (first) {
      const float4* gs = reinterpret_cast<const float4*>(g.state + gi * 8);
      s0 = gs[0]; s1 = gs[1];
      pth = g.path[gi * 4];
      // last step's vertices: agent 0's corner queries and the whole mtv matrix still see them (world_state_rt_sim.py:439-448)
      const float2* gv = reinterpret_cast<const float2*>(g.vertices + gi * 10);
#pragma unroll
      for (int k = 0; k < 5; ++k) vo[k] = gv[k];
      cp0 = g.closest[gi * 3 + 0]; cp1 = g.closest[gi * 3 + 1]; cp2 = g.closest[gi * 3 + 2];
      pp = reinterpret_cast<const float2*>(g.prev_pos)[gi];
      const float2* gst = reinterpret_cast<const float2*>(g.short_term + gi * NS * 2);
#pragma unroll
      for (int k = 0; k < NS; ++k) spo[k] = gst[k];
      tm = reinterpret_cast<const int4*>(g.timer)[t.env0 + fdiv(sl, g.mN)];  // step count and counters of the env
      if (act && h == 0 && sl - fdiv(sl, g.mN) * N == 0) s_tim[fdiv(sl, g.mN) * 4 + 3] = tm.w;  // episodes_reset: only the resets change it (LDS copy for the noise key)
    } else {  // the tile as the previous step of this launch (and its resets) left it in LDS
      const float4* ls = reinterpret_cast<const float4*>(s.st + sl * 8);
      s0 = ls[0]; s1 = ls[1];
      pth = s.path[sl];
#pragma unroll
      for (int k = 0; k < 5; ++k) vo[k] = make_float2(s.vnew[sl * 10 + 2 * k], s.vnew[sl * 10 + 2 * k + 1]);
      cp0 = s.cp[sl * 3 + 0]; cp1 = s.cp[sl * 3 + 1]; cp2 = s.cp[sl * 3 + 2];
      pp = make_float2(s0.x, s0.y);  // state_buffer.add stored the position after every step, a reset re-stores it (road_traffic.py:1226-1240, :910-923)
#pragma unroll
      for (int k = 0; k < NS; ++k) spo[k] = make_float2(s.shrt[sl * NS * 2 + 2 * k], s.shrt[sl * NS * 2 + 2 * k + 1]);
      tm = reinterpret_cast<const int4*>(s_tim)[fdiv(sl, g.mN)];
    }
    const int loop_flag = m.is_loop[pth];
    st[0] = s0.x; st[1] = s0.y; st[2] = s0.z; st[3] = s0.w; st[4] = s1.x; st[5] = s1.y; st[6] = s1.z; st[7] = s1.w;
    float cr3[3] = {0.f, 1.f, 0.f};
    if (par && !first) { cr3[0] = s.carry[sl * 3]; cr3[1] = s.carry[sl * 3 + 1]; cr3[2] = s.carry[sl * 3 + 2]; }
    if (SKIP(1)) { uc[0] = u.x; uc[1] = u.y; csy[0] = 1.f; csy[1] = 0.f; }
    else if (par && !first) bicycle_step_pair_carried(c, dv, st, u.x, u.y, uc, csy, h, cr3);  // (step_i >= 1: wavefront-uniform)
    else bicycle_step_pair(c, dv, st, u.x, u.y, uc, csy, par, h, cr3);
    float v[10];
    rect_vertices_cs(dv, st[0], st[1], csy[0], csy[1], v);
    if (act && h == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s.st[sl * 8 + k] = st[k];
      if (last) {
        reinterpret_cast<float2*>(g.action)[gi] = make_float2(uc[0], uc[1]);
        float4* go = reinterpret_cast<float4*>(g.state + gi * 8);
        go[0] = make_float4(st[0], st[1], st[2], st[3]);
        go[1] = make_float4(st[4], st[5], st[6], st[7]);
      }
      s.cs[sl * 2] = csy[0]; s.cs[sl * 2 + 1] = csy[1];
      s.carry[sl * 3] = cr3[0]; s.carry[sl * 3 + 1] = cr3[1]; s.carry[sl * 3 + 2] = cr3[2];
      s.path[sl] = pth;
      s.fresh[sl] = 0;  // stepped (phase R sets it again for the agents it re-places)
      s.thr[sl * 3] = pp.x; s.thr[sl * 3 + 1] = pp.y;
      s.thr[sl * 3 + 2] = __int_as_float(tm.x);
      s.flags[sl * 4 + 0] = 0;  // boundary collision: phase E sets it from the lanes that find a crossing
      s.flags[sl * 4 + 1] = loop_flag;
      s.flags[sl * 4 + 2] = tm.y;  // counters: the first agent's lane of every env keeps them for the done() bookkeeping
      s.near[sl * (t.K > 0 ? t.K : 1)] = tm.z;  // (the nearest-neighbour list is only filled by the observation phase)
      s.cp[sl * 3 + 0] = cp0; s.cp[sl * 3 + 1] = cp1; s.cp[sl * 3 + 2] = cp2;
    }
    if (act && h == (par ? 1 : 0)) {
      float2* gvo = reinterpret_cast<float2*>(g.vertices + gi * 10);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        s.vold[sl * 10 + 2 * k] = vo[k].x; s.vold[sl * 10 + 2 * k + 1] = vo[k].y;
        s.vnew[sl * 10 + 2 * k] = v[2 * k]; s.vnew[sl * 10 + 2 * k + 1] = v[2 * k + 1];
        if (last) gvo[k] = make_float2(v[2 * k], v[2 * k + 1]);
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) { s.shrt[sl * NS * 2 + 2 * k] = spo[k].x; s.shrt[sl * NS * 2 + 2 * k + 1] = spo[k].y; }
    }
  }
  wave_sync();
  TSW(1);
  // ---- S: distance queries (lane per (agent, polyline)); full-scan fallback one agent at a time -------------------------------
  {
  STEP_TABLES(m, g);
  if (SKIP(2)) {
  } else if (m.nch > 0) {
    scan_tile_balanced<FASTDIV>(m, dv, g, s, t, G, lane);
  } else {
    for (int sl = 0; sl < t.slots; ++sl) {
      const int i = sl % N;
      const float* si = s.st + sl * 8;
      const float* qv = (i == 0) ? (s.vold + sl * 10) : (s.vnew + sl * 10);
      AgentScan r;
      agent_scan_full<true>(m, c, s.path[sl], lane, si[0], si[1], qv, s.vnew + sl * 10, r);
      if (lane == 0) {
        s.dref[sl] = r.d_ref;
#pragma unroll
        for (int q = 0; q < 5; ++q) { s.dleft[sl * 5 + q] = r.dl[q]; s.dright[sl * 5 + q] = r.dr[q]; }
        s.cp[sl * 3 + 0] = r.cp_ref; s.cp[sl * 3 + 1] = r.cp_l; s.cp[sl * 3 + 2] = r.cp_r;
        s.npts[sl * 3] = m.n_center[s.path[sl]];
        s.flags[sl * 4 + 0] = r.hit ? 1 : 0;
      }
    }
  }
  }
  wave_sync();
  TSW(2);
  // ---- E: rectangle edge x listed boundary segment (interX, helper_scenario.py:1165-1196; world_state_rt_sim.py:398-411) --------
  {
  // (the common path reads LDS only: the map's tables are fetched inside the two branches that load from the map)
  STEP_KA(ka_e);
  if (ka_e->m.nch > 0 && !SKIP(4) && !SKIP(2)) {  // (a skipped scan leaves no list)
    const int total = __builtin_amdgcn_readfirstlane(*s.nearc), near_cap = G * N * NEAR_CAP, xy_cap = Smem::near_xy_cap(G * N, N);
#ifdef SIGMAENV_PROFILE
    if (unsigned long long* ts_ = as_global(ka_e->g.dbg_ts); ts_ && lane == 0) {
      // list statistics of the tile, in the upper halves of the work-list words: entries, tile-steps whose list overflowed; in the upper halves of the
      // neighbour-level words 12 / 13: tile-steps that needed a second pass, tile-steps with an entry beyond the coordinate capacity (taken from the map)
      ts_[(size_t)tile_index * 16 + 8] += (unsigned long long)total << 32;
      ts_[(size_t)tile_index * 16 + 9] += (unsigned long long)(total > near_cap ? 1 : 0) << 32;
#ifndef SIGMAENV_PROFILE_RT
      ts_[(size_t)tile_index * 16 + 12] += (unsigned long long)((total <= near_cap && total > 64) ? 1 : 0) << 32;
      ts_[(size_t)tile_index * 16 + 13] += (unsigned long long)((total <= near_cap && total > xy_cap) ? 1 : 0) << 32;
#endif
    }
#endif
    if (total <= near_cap) {
      // one lane per listed segment: its code and its end points from LDS (the scan's lane stored them as it held them), the four edges of its agent's rectangle
      // tested in turn.  The flag of an agent is the OR over its entries and edges, so neither the order of the list nor the pass an entry falls into enters the
      // result, and the tests are those of the lane-per-(entry, edge) form operand for operand.  An entry beyond the coordinate capacity takes its segment from
      // the map by its code, as every entry did before; a pass without such an entry (wavefront-uniform) touches no table.
      for (int base = 0; base < total; base += 64) {
        const int w = base + lane, wc = min(w, total - 1);
        const unsigned code = s.nearl[wc];
        const int bt = (int)(code >> 8), sl = bt >> 1, side = bt & 1;
        float4 sg;
        if (min(base + 63, total - 1) < xy_cap) {
          sg = s.nearxy[wc];
        } else {
          STEP_KA(ka_f);
          const float* center = as_global(ka_f->m.center);
          const unsigned poly_off = (unsigned)(side + 1) * (unsigned)ka_f->m.poly_stride + (unsigned)s.path[sl] * (unsigned)(ka_f->m.P * 2);
          if (wc < xy_cap) {
            sg = s.nearxy[wc];
          } else {
            const Seg4 q = *reinterpret_cast<const Seg4*>(center + (poly_off + 2u * (code & 255u)));
            sg = make_float4(q.ax, q.ay, q.bx, q.by);
          }
        }
        if (w < total) {
          const float lx = sg.z - sg.x, ly = sg.w - sg.y;
          const float S2 = lx * sg.y - ly * sg.x;
          const float* pv = s.vnew + sl * 10;
          bool hit = false;
#pragma unroll
          for (int e4 = 0; e4 < 4; ++e4) {
            const Edge ed = make_edge(pv[2 * e4], pv[2 * e4 + 1], pv[2 * e4 + 2], pv[2 * e4 + 3]);
            hit |= edge_hits_segment(ed, sg.x, sg.y, sg.z, sg.w, lx, ly, S2);
          }
          if (hit) s.flags[sl * 4 + 0] = 1;
        }
      }
    } else {
      STEP_TABLES(m, g);
      (void)g;
      // the list overflowed (more than NEAR_CAP close segments per slot of the tile: the `dense` map of tests/synthetic_maps.py): lane per (agent, side, edge),
      // every real segment of each boundary that counted a near one -- a superset of the listed ones, which cannot change the OR
      for (int base = 0; base < t.slots * 2; base += 16) {
        const int bt = base + (lane >> 2), e4 = lane & 3;
        const bool act = bt < t.slots * 2;
        const int btc = act ? bt : 0;
        const int sl = btc >> 1, side = btc & 1;
        const int cnt = (act && s.nearn[btc] > 0) ? (s.npts[sl * 3 + 1 + side] - 1) : 0;
        const float* pv = s.vnew + sl * 10 + 2 * e4;
        const Edge ed = make_edge(pv[0], pv[1], pv[2], pv[3]);
        const unsigned poly_off = (unsigned)(side + 1) * (unsigned)m.poly_stride + (unsigned)s.path[sl] * (unsigned)(m.P * 2);
        bool hit = false;
        for (int j = 0; __any(j < cnt); ++j) {
          if (j < cnt) {
            const Seg4 sg = *reinterpret_cast<const Seg4*>(m.center + (poly_off + 2u * (unsigned)j));
            const float lx = sg.bx - sg.ax, ly = sg.by - sg.ay;
            const float S2 = lx * sg.ay - ly * sg.ax;
            hit |= edge_hits_segment(ed, sg.ax, sg.ay, sg.bx, sg.by, lx, ly, S2);
          }
        }
        if (hit) s.flags[sl * 4 + 0] = 1;
      }
    }
  }
  }
  TSW(3);
  // ---- B1: mutual distances + agent-agent collisions (one lane per unordered pair) ------------------------------------------
  {
  STEP_TABLES(m, g);
  if (!SKIP(8)) {
    const float diag = dv.diag;  // sqrtf(world_x_dim^2 + world_y_dim^2), helper_scenario.py:1140-1143 (derive_config)
    const int TP = N * (N - 1) / 2;
    const int n_pairs = t.nenv * TP;
    // The N terms 1 - decreasing_lin(d_ij) of every agent's proximity penalty (road_traffic.py:1086-1110, helper_scenario.py:960-996) are staged HERE, by the
    // lane that has just computed d_ij (one evaluation per unordered pair -- d_ij and d_ji are the same float -- instead of one per ordered pair in a pass of
    // its own), in the observation area, which is free until phase D; the agent's lane of phase C then only adds them in index order.  The division by the
    // constant (x1 - x0) goes through its reciprocal (exact, see div_shared; the numerator is 0 or at least an ulp of the thresholds).
    const bool pen_staged = !c.is_testing_mode && (c.rew_flags & SIGMAENV_REW_DISTANCE) && N <= t.DL;
    const float pen_x0 = c.threshold_near_other_agents_low, pen_x1 = c.threshold_near_other_agents_high;
    const float pen_den = pen_x1 - pen_x0;
    const bool pen_fast = pen_den >= 0x1p-60f && pen_den <= 0x1p60f;
    const float pen_rcp = pen_fast ? shared_rcp(pen_den) : 0.0f;
    auto pen_term = [&](float d) {
      const float x = clampf(d, pen_x0, pen_x1);
      const float q = pen_fast ? div_shared(x - pen_x0, pen_den, pen_rcp) : (x - pen_x0) / pen_den;
      return 1.0f - q;
    };
    // mtv: what the distance of a pair takes from ONE of its rectangles alone -- the two unit edge axes (a root and two divisions each) and the extents of its own
    // vertices on them -- is evaluated once per agent here and staged behind the penalty terms (8 floats per slot), instead of once per pair the agent is part of
    // (15 times at 16 agents): the same operations in the same order (rect_mtv_record), the pair's lane then only projects the OTHER rectangle (mtv_pair_staged)
    const bool mtv_staged = MTVS && c.distance_type != SIGMAENV_DIST_C2C && N + MTV_REC <= t.DL;
    float* mtv_rec = s.obs + t.slots * N;
    wave_sync();  // (phase E has read the scan's work areas, which share these bytes)
    for (int sl = lane; sl < t.slots; sl += 64) {
      const int i = sl - fdiv(sl, g.mN) * N;
      s.dist[sl * DIST_STRIDE(N) + i] = diag;
      s.col[sl * COL_STRIDE(N) + i] = 0;
      if (pen_staged) s.obs[sl * N + i] = pen_term(diag);
    }
    if (mtv_staged) {
      for (int sl = lane; sl < t.slots; sl += 64) rect_mtv_record(s.vold + sl * 10, mtv_rec + sl * MTV_REC);
      wave_sync();
    }
    for (int base = 0; base < n_pairs; base += 64) {
      const int p = base + lane;
      const bool in_range = p < n_pairs;
      int si = 0, sj = 0, i = 0, j = 0;
      bool near = false;
      if (in_range) {
        const int e = fdiv(p, g.mTP);
        const unsigned ij = SN > 0 ? kPairTable<(SN > 0 ? SN : 2)>.v[p - e * TP] : s.pidx[p - e * TP];
        i = (int)(ij & 0xFFu); j = (int)(ij >> 8);
        si = e * N + i; sj = e * N + j;
        float d;
        if (!mtv_staged) d = pair_distance(c, s.st, s.vold, si, sj);
        else d = mtv_pair_staged(s.vold + si * 10, s.vold + sj * 10, mtv_rec + si * MTV_REC, mtv_rec + sj * MTV_REC);  // (si < sj, as pair_distance orders them)
        s.dist[si * DIST_STRIDE(N) + j] = d;
        s.dist[sj * DIST_STRIDE(N) + i] = d;
        if (pen_staged) { const float pt = pen_term(d); s.obs[si * N + j] = pt; s.obs[sj * N + i] = pt; }
        uint8_t col = 0;
        if (c.distance_type == SIGMAENV_DIST_C2C) {
          // world_state_rt_sim.py:382-393; rectangles whose circumcircles are disjoint cannot produce a proper edge crossing
          near = !(d > 2.0f * m.rect_radius + 1e-4f);
        } else {
          col = (d == 0.0f) ? 1 : 0;  // :394-396
        }
        if (!near) { s.col[si * COL_STRIDE(N) + j] = col; s.col[sj * COL_STRIDE(N) + i] = col; }
      }
      // the 16 (edge of A, edge of B) tests of a close pair, one per lane, four pairs per pass (interX, helper_scenario.py:1165-1196)
      unsigned long long todo = __ballot(near);
      while (todo) {
        const int q = lane >> 4, tt = lane & 15;
        unsigned long long rest = todo;
        int src = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int b = rest ? (__ffsll((long long)rest) - 1) : -1;
          if (k == q) src = b;
          rest &= rest - 1ull;
        }
        todo = rest;
        const int a_sl = __shfl(si, src < 0 ? 0 : src, 64), b_sl = __shfl(sj, src < 0 ? 0 : src, 64);
        bool hit = false;
        if (src >= 0) {
          const float* va = s.vnew + a_sl * 10 + 2 * (tt >> 2);
          const float* vb = s.vnew + b_sl * 10 + 2 * (tt & 3);
          const Edge ed = make_edge(va[0], va[1], va[2], va[3]);
          const float dx2 = vb[2] - vb[0], dy2 = vb[3] - vb[1];
          const float S2 = dx2 * vb[1] - dy2 * vb[0];
          hit = edge_hits_segment(ed, vb[0], vb[1], vb[2], vb[3], dx2, dy2, S2);
        }
        const unsigned long long hb = __ballot(hit);
        if (src >= 0 && tt == 0) {
          const uint8_t col = ((hb >> (q * 16)) & 0xFFFFull) ? 1 : 0;
          const int ea = fdiv(a_sl, g.mN) * N;
          s.col[a_sl * COL_STRIDE(N) + (b_sl - ea)] = col;
          s.col[b_sl * COL_STRIDE(N) + (a_sl - ea)] = col;
        }
      }
    }
  }
  wave_sync();
  TSW(4);
  // the two matrices leave LDS row by row (coalesced)
  if (last) for (int k = lane; k < t.slots * N; k += 64) {
    const int sl = fdiv(k, g.mN), j = k - sl * N;
    g.dist_agents[t.a0 * N + k] = s.dist[sl * DIST_STRIDE(N) + j];
    g.col_agents[t.a0 * N + k] = s.col[sl * COL_STRIDE(N) + j];
  }

  }
  // ---- C: reward, short-term path, per-env done()/counters via ballots (one lane per agent) -----------------------------------
  {
  STEP_TABLES(m, g);
  STEP_KA(ka_c);
  const float* __restrict__ actions = as_global(ka_c->actions_base) + (size_t)step_i * ka_c->act_stride;  // (read again by the CBF-QP deviation penalty only)
  // (the N terms 1 - decreasing_lin(d_ij) of every agent's proximity penalty were staged by phase B1)
  const bool pen_staged = !c.is_testing_mode && (c.rew_flags & SIGMAENV_REW_DISTANCE) && N <= t.DL && !SKIP(8);
  if (!SKIP(16)) {
    const bool act = lane < t.slots;
    const int sl = act ? lane : 0;
    const int e = fdiv(sl, g.mN), i = sl - e * N;
    const size_t gi = t.a0 + sl;
    const size_t BN = (size_t)c.n_envs * N;
    int col_a = 0, col_l = 0, goal = 0, entry = 0;
    if (act) {
      // the new short-term reference path (needed at the end of the phase) is requested first: its loads would otherwise queue behind the
      // phase's stores
      float sp[NS * 2];
      short_term_path(m.center + (size_t)s.path[sl] * m.P * 2, s.npts[sl * 3], s.flags[sl * 4 + 1] != 0, s.cp[sl * 3], sp);
      const float* si = s.st + sl * 8;
      const float2 pp = make_float2(s.thr[sl * 3], s.thr[sl * 3 + 1]);
      float w[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) w[k] = __uint_as_float(W_REF_BITS[k]);
      float mvx = si[0] - pp.x, mvy = si[1] - pp.y;                  // road_traffic.py:972-974
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < NS; ++k) {  // the short-term path of the PREVIOUS step (:976-984), staged in LDS by phase A
        const float2 sp = make_float2(s.shrt[sl * NS * 2 + 2 * k], s.shrt[sl * NS * 2 + 2 * k + 1]);
        float rx = sp.x - pp.x, ry = sp.y - pp.y;
        float mp = mvx * rx + mvy * ry;
        acc = acc + mp * w[k];
      }
      const float denom = dv.rew_denom;  // (float)(max_speed * dt) in float64 (derive_config)
      float rew = 0.0f;
      rew += acc / denom * c.reward_progress;                        // :986-991
      {  // entry / exit segments of non-loop paths (world_state_rt_sim.py:413-424) and the boundary minimum (world_state_rt.py:648-656)
        const int pth = s.path[sl];
        if (!s.flags[sl * 4 + 1]) {
          const float* lb = m.left + (size_t)pth * m.P * 2;
          const float* rb = m.right + (size_t)pth * m.P * 2;
          const int nl = m.n_left[pth], nr = m.n_right[pth];
          entry = interx_rect_seg(s.vnew + sl * 10, lb[0], lb[1], rb[0], rb[1]) ? 1 : 0;
          goal = interx_rect_seg(s.vnew + sl * 10, lb[2 * (nl - 1)], lb[2 * (nl - 1) + 1], rb[2 * (nr - 1)], rb[2 * (nr - 1) + 1]) ? 1 : 0;
        }
        float mbnd = INFINITY;
#pragma unroll
        for (int q = 0; q < 5; ++q) mbnd = fminf(mbnd, s.dleft[sl * 5 + q]);
#pragma unroll
        for (int q = 0; q < 5; ++q) mbnd = fminf(mbnd, s.dright[sl * 5 + q]);
        s.dbound[sl] = mbnd;
      }
      float reward_goal = (float)goal * c.reward_reach_goal;
      if ((N & 3) == 0) {  // the row of collision bytes is word aligned (COL_STRIDE): N / 4 LDS reads instead of N  (:1008-1013)
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(s.col + sl * COL_STRIDE(N));
        uint32_t any = 0u;
        for (int j = 0; j < N / 4; ++j) any |= cw[j];
        col_a = any != 0u;
      } else {
        for (int j = 0; j < N; ++j) col_a |= s.col[sl * COL_STRIDE(N) + j];
      }
      float pca = (float)col_a * c.penalty_collide_with_agents;
      col_l = s.flags[sl * 4 + 0];
      float pcl = (float)col_l * c.penalty_collide_with_boundaries;  // :1021-1026
      float pen_lane = decreasing_lin(s.dbound[sl], c.threshold_near_boundary_low, c.threshold_near_boundary_high) * c.penalty_near_boundary;
      bool has_near = false;
      float near_other = 0.0f;
      if (c.is_testing_mode) {                                       // :1050-1055
        rew += reward_goal; rew += pca; rew += pcl;
      } else {
        if (c.rew_flags & SIGMAENV_REW_EXACT_SPARSE) { rew += pca; rew += pcl; }
        if (c.rew_flags & SIGMAENV_REW_TTC) {                        // :1064-1084
          float p = ttc_penalty(c, s.st + e * N * 8, N, i);
          near_other = p; has_near = true;
          rew += p; rew += pen_lane; rew += pca; rew += pcl;
          if (c.rew_flags & SIGMAENV_REW_HAS_SPARSE) { rew += pca; rew += pcl; }
        }
        if (c.rew_flags & SIGMAENV_REW_DISTANCE) {                   // :1086-1110
          float ssum = 0.0f;
          if (pen_staged) {
            for (int j = 0; j < N; ++j) ssum += s.obs[sl * N + j];
          } else {  // decreasing_lin (helper_scenario.py:960-996) with the division by the constant (x1 - x0) through its reciprocal (exact, see
             // div_shared; the numerator is 0 or at least an ulp of the thresholds)
            const float x0 = c.threshold_near_other_agents_low, x1 = c.threshold_near_other_agents_high;
            const float denom2 = x1 - x0;
            const bool fast = denom2 >= 0x1p-60f && denom2 <= 0x1p60f;
            const float rcp = fast ? shared_rcp(denom2) : 0.0f;
            for (int j0 = 0; j0 < N; j0 += 4) {
              float d[4];
#pragma unroll
              for (int u2 = 0; u2 < 4; ++u2) d[u2] = s.dist[sl * DIST_STRIDE(N) + min(j0 + u2, N - 1)];
#pragma unroll
              for (int u2 = 0; u2 < 4; ++u2) {
                if (j0 + u2 < N) {
                  const float x = clampf(d[u2], x0, x1);
                  const float q = fast ? div_shared(x - x0, denom2, rcp) : (x - x0) / denom2;
                  ssum += 1.0f - q;
                }
              }
            }
          }
          float p = ssum * c.penalty_near_other_agents;
          near_other = p; has_near = true;
          rew += p; rew += pen_lane;
          if (c.rew_flags & SIGMAENV_REW_HAS_SPARSE) { rew += pca; rew += pcl; }
        }
        if (c.rew_flags & SIGMAENV_REW_CBF_QP) {                     // :1112-1139 with is_solve_qp == True
          // deviation of the applied (clamped) action from world_state.nominal_action_*, which sigmaenv_cbf_qp left behind
          const float2 nomv = reinterpret_cast<const float2*>(g.cbf_nominal)[gi];
          const float2 ua = reinterpret_cast<const float2*>(actions)[gi];
          const float cur0 = clampf(ua.x, -c.max_speed, c.max_speed), cur1 = clampf(ua.y, -c.max_steering, c.max_steering);
          const float pv = c.penalty_deviate_from_cbf_vel * (fabsf(cur0 - nomv.x) / c.max_speed);
          const float ps = c.penalty_deviate_from_cbf_steer * (fabsf(cur1 - nomv.y) / c.max_steering);
          rew += pv + ps;
          if (c.rew_flags & SIGMAENV_REW_HAS_SPARSE) { rew += pca; rew += pcl; }
        }
        if (c.rew_flags & SIGMAENV_REW_CBF) {                        // :1112-1151 with is_solve_qp == False
          // the three margin channels CBFQP.update_qp wrote before this step (sigmaenv_cbf_rewards)
          const float cbf_rew = ((g.reward_info[5 * BN + gi] + g.reward_info[6 * BN + gi]) + g.reward_info[4 * BN + gi]) / 3.0f;
          rew += cbf_rew;
          if (c.rew_flags & SIGMAENV_REW_HAS_SPARSE) { rew += pca; rew += pcl; }
        }
      }
      float r = clampf(rew, -1.0f, 1.0f);                            // :1249
      s.rew[sl] = r;
      // update_state_after_rewarding: new short-term path (world_state_rt_sim.py:450-454)
#pragma unroll
      for (int k = 0; k < NS; ++k) { s.shrt[sl * NS * 2 + 2 * k] = sp[2 * k]; s.shrt[sl * NS * 2 + 2 * k + 1] = sp[2 * k + 1]; }
      if (last) {
        g.reward[gi] = r;
        // RewardInfo.reset() at the top of every reward() zeroes all agents' entries except three fields
        // (helper_scenario.py:128-138): only the last agent's values of the other fields survive the loop.
        const bool last_agent = (i == N - 1);
        g.reward_info[1 * BN + gi] = last_agent ? reward_goal : 0.0f;
        g.reward_info[7 * BN + gi] = last_agent ? pca : 0.0f;
        g.reward_info[8 * BN + gi] = last_agent ? pcl : 0.0f;
        g.reward_info[11 * BN + gi] = last_agent ? r : 0.0f;
        if (has_near) g.reward_info[4 * BN + gi] = near_other;
        float2* gso = reinterpret_cast<float2*>(g.short_term + gi * NS * 2);
#pragma unroll
        for (int k = 0; k < NS; ++k) gso[k] = make_float2(sp[2 * k], sp[2 * k + 1]);
        reinterpret_cast<float2*>(g.prev_pos)[gi] = make_float2(si[0], si[1]);  // state_buffer.add, road_traffic.py:1226-1240
        g.dist_ref[gi] = s.dref[sl];
#pragma unroll
        for (int q = 0; q < 5; ++q) { g.dist_left[gi * 5 + q] = s.dleft[sl * 5 + q]; g.dist_right[gi * 5 + q] = s.dright[sl * 5 + q]; }
        g.dist_bound[gi] = s.dbound[sl];
        g.closest[gi * 3 + 0] = s.cp[sl * 3 + 0]; g.closest[gi * 3 + 1] = s.cp[sl * 3 + 1]; g.closest[gi * 3 + 2] = s.cp[sl * 3 + 2];
      }
    }
    // timer, counters, done(), reset requests (road_traffic.py:954-962,998-1002,1030-1035,1368-1487): per-env reductions by ballot
    const unsigned long long env_mask = ((N >= 64) ? ~0ull : ((1ull << N) - 1ull)) << (e * N);
    const unsigned long long b_ca = __ballot(act && col_a), b_cl = __ballot(act && col_l), b_goal = __ballot(act && goal);
    const unsigned long long b_any = __ballot(act && (col_a | col_l | goal));
    if (act) {
      const int b = t.env0 + e;
      const int step = __float_as_int(s.thr[sl * 3 + 2]) + 1;
      const int max_reached = (step == c.max_steps - 1);
      const int any_ca = (b_ca & env_mask) != 0ull, any_cl = (b_cl & env_mask) != 0ull;
      int fixed = 0;  // reset_agent_fixed_duration: t = step * dt as an fp32 tensor, t % duration == 0 and t != 0 (road_traffic.py:1388-1397)
      if (c.reset_agent_fixed_duration > 0.0f) {
        const float tt = (float)step * c.dt;
        fixed = (remainder_pos(tt, c.reset_agent_fixed_duration) == 0.0f) && (tt != 0.0f);
      }
      const int done = c.is_testing_mode ? (max_reached | fixed) : (max_reached | any_ca | any_cl | fixed);
      int rq = 0;
      if (c.is_testing_mode) rq = col_a | col_l | entry | goal;
      else if (c.has_entry_exit) rq = entry | goal;
      if (last) {
        reinterpret_cast<uchar4*>(g.col_flags)[gi] = make_uchar4((uint8_t)col_l, (uint8_t)entry, (uint8_t)goal, (uint8_t)((rq && !done) ? 1 : 0));
        if (g.fresh) g.fresh[gi] = 0;  // stepped (phase R sets it again for the agents it re-places)
      }
      s.flags[sl * 4 + 3] = (rq && !done) ? 1 : 0;
      if (i == 0) {
        const int tries = s.flags[sl * 4 + 2] + __popcll(b_any & env_mask), succ = s.near[sl * (t.K > 0 ? t.K : 1)] + __popcll(b_goal & env_mask);
        s_tim[e * 4] = step; s_tim[e * 4 + 1] = tries; s_tim[e * 4 + 2] = succ;
        if (last) {
          g.timer[b * 4] = step;
          g.timer[b * 4 + 1] = tries;
          g.timer[b * 4 + 2] = succ;
          g.done[b] = (uint8_t)done;
        }
        s.rew[G * N + e] = done ? 1.0f : 0.0f;
      }
    }
  }
  }
  wave_sync();
  TSW(5);
  {
  STEP_TABLES(m, g);
  STEP_KA(ka_r);
  const int path_first = ka_r->path_first, path_count = ka_r->path_count;
  const uint64_t seed = ka_r->seed, counter = ka_r->counter0 + (uint64_t)step_i;
  float* __restrict__ slab = ka_r->slab_base ? as_global(ka_r->slab_base) + (size_t)step_i * ka_r->slab_stride : nullptr;

  // fused resets: the start candidates of a finished env only depend on the random stream and the map: requested now, the two dependent
  // loads complete behind the observation phase (the first finished env of the tile)
  ResetPrefetch pre;
  pre.have = false;
  pre.path = 0; pre.pt = 3; pre.x = 0.f; pre.y = 0.f;
  if (path_count > 0 && s.rew[G * N + 0] != 0.0f) {
    const int TRp = 64 / N > 0 ? 64 / N : 1;
    const int ca = lane / TRp, ctr = lane - ca * TRp;
    const ResetDraw rd{seed, counter, path_first, path_count, c.is_testing_mode, c.env_index_base};
    if (ca < N) reset_candidate(m, rd, t.env0, ca, ctr, pre.path, pre.pt, pre.x, pre.y);
    pre.have = true;
  }
  // ---- D: observations ---------------------------------------------------------------------------------------------
  if (!SKIP(32)) observe_tile<true, VAR>(c, s, g, t, -1, nullptr, 0, last, s_tim, &dv);
  if (slab) {  // rollout record of this step (observation AFTER the step, reward, done), one contiguous row per env
    const int ND = N * t.D, W = ND + N + 1;
    if (VAR && (c.obs_flags & SIGMAENV_OBS_FULL)) {  // the full observation's rows are composed from the staging area (one [others] block per env)
      const ObsLayout L(c.obs_flags, N, t.K);
      for (int k = lane; k < t.nenv * W; k += 64) {
        const int e = k / W, r = k - e * W;
        float v;
        if (r < ND) { const int i = r / t.D; v = full_obs_value(c, s, t, L, e, i, r - i * t.D, s_tim); }
        else v = (r < ND + N) ? s.rew[e * N + (r - ND)] : s.rew[G * N + e];
        slab[(size_t)(t.env0 + e) * W + r] = v;
      }
    } else if ((ND & 3) == 0) {
      const int Q = ND >> 2;  // float4s per env
      for (int k = lane; k < t.nenv * Q; k += 64) {
        const int e = k / Q, q = k - e * Q;
        const float4 v = reinterpret_cast<const float4*>(s.obs + e * ND)[q];
        *reinterpret_cast<F4u*>(slab + (size_t)(t.env0 + e) * W + 4 * q) = F4u{v.x, v.y, v.z, v.w};
      }
      for (int k = lane; k < t.nenv * (N + 1); k += 64) {  // rewards and the done flag
        const int e = k / (N + 1), r = k - e * (N + 1);
        slab[(size_t)(t.env0 + e) * W + ND + r] = (r < N) ? s.rew[e * N + r] : s.rew[G * N + e];
      }
    } else {
      for (int k = lane; k < t.nenv * W; k += 64) {
        int e = fdiv(k, g.mW), r = k - e * W;
        float v = (r < ND) ? s.obs[e * ND + r] : ((r < ND + N) ? s.rew[e * N + (r - ND)] : s.rew[G * N + e]);
        slab[(size_t)(t.env0 + e) * W + r] = v;
      }
    }
  }
  TSW(6);
  TSRT(13);
  // ---- R: fused device-side resets (sigmaenv_step_autoreset): the tile is still in LDS, the record of this step is written -------
  if (path_count != 0 && !SKIP(64)) {
    wave_sync();  // the slab rows above have read s.obs / s.rew
    int any = 0;
    if (lane < t.nenv) {
      const int dn = s.rew[G * N + lane] != 0.0f;
      unsigned long long rq = 0ull;
      if (!dn && (c.is_testing_mode || c.has_entry_exit)) {
        for (int i = 0; i < N; ++i) rq |= (unsigned long long)(s.flags[(lane * N + i) * 4 + 3] != 0) << i;
      }
      s_mask[lane] = dn ? ((N >= 64) ? ~0ull : ((1ull << N) - 1ull)) : rq;
      s_full[lane] = dn;
      any = (dn || rq) ? 1 : 0;
    }
    const bool any_w = __ballot(any) != 0ull;
    if (lane == 0) *s_any = any_w ? 1 : 0;
    wave_sync();
    if (any_w) {
      // (a restarted env counts its steps from 0: reset_finish_body).  Before the last step of the launch a reset leaves in HBM only what no step writes back -- path rows,
      // the episode counter, the request words -- and in LDS what the next step reads: the last step's phases write the rest of the tile (sigmaenv.hip: fin)
      // (`last` is a run-time, wavefront-uniform switch: two compiled copies of the reset path measured the same and cost 4 KB of code per instantiation)
      auto_reset_tile<true, VAR>(c, m, g, s, t, s_mask, s_full, seed, counter, path_first, path_count, 2, pre, G, s_tim, &dv, last);
    }
  }
  }
  TSW(7);
  TSRT(14);
  wave_sync();  // the next step of this tile continues from LDS
  }  // step_i
#undef STEP_TABLES
#undef STEP_KA
#undef TSW
#undef TSRT
#undef SKIP
}
