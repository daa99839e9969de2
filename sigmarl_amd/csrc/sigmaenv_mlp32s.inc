// sigmaenv_mlp32s.inc -- the fp32 networks of sigmaenv_mlp32.inc on the HALF-PRECISION matrix rate: every fp32 operand as the sum of two fp16 numbers
// (included by sigmaenv_mlp32.inc; mode SIGMAENV_MLP32_SPLIT of a sigmaenv_mlp32 handle).
//
// Why.  gfx950 has no TF32-class instruction: v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate (157 TF), 1/16 of v_mfma_f32_32x32x16_f16 (2.5 PF).  The
// reference's actor / critic (decision_making_module.py:34-52, optimization_module.py:16-32: fp32 torch MLPs) are 18.4 GFLOP per step of the metric's batch:
// 117 us at the fp32 matrix peak against 29 us for the env step they feed.  An fp32 number x (scaled by a power of two) is hi + lo with hi = fp16(x),
// lo = fp16(x - hi): 22 significant bits (fp16 subnormals are preserved by the matrix pipe: tools/mfma_probe/probe_f16_split.hip), so
//     w x = w_hi x_hi + w_hi x_lo + w_lo x_hi + (w_lo x_lo: 2^-22 relative, dropped)
// is three fp16 MFMAs with EXACT products (11 x 11 bits) accumulated in fp32: 3/16 of the fp32 matrix time.  Measured on K = 256 dot products against fp64:
// 3.6e-7 for the split, 6.4e-7 for the exact fp32 fma chain (the fp16 instruction sums its 16 products before it rounds) -- the same error class as
// torch.nn.Linear in fp32, whose summation order differs anyway; tests/test_gpu_actor.py holds both modes to the same 1e-5.
// Scales: weights and hidden activations (|tanh| <= 1) are stored times 2^8, the input rows times 2^4, so that the lo parts of values down to 2^-11 (2^-7 for
// inputs) are fp16 normals; ranges |w| < 255, |input| < 4094 (create falls back to the exact mode when a weight is outside; an input outside is saturated: mlp32s_sat).
// The accumulator carries the product of the two scales (biases are pre-scaled: exact), the epilogue multiplies by its reciprocal (exact).
//
// Mapping: as the exact kernel -- one workgroup (4 wavefronts) owns 64 rows through all layers, wavefront w owns feature tiles 2 w, 2 w + 1 x both row tiles,
// weights stream from L2 as A operands (pre-split, pre-permuted fragments: 2 x 1 KB contiguous per wavefront, tile and k block of 16), the activations live in
// LDS as B-operand fragments [k block][hi | lo][k half][row][8 halves] = 64 KB per 64 rows and K = 256.  Per tile and k block: 2 global 16-byte loads + 4
// ds_read_b128 feed 6 MFMAs (192 matrix cycles).  A hidden layer's outputs go back as whole 16-byte fragments: the k order of the next layer is PERMUTED when its weights are packed (sigmaenv_pack.h) so that the
// 8 accumulator registers (j = 8 hh .. 8 hh + 7) a lane holds for one row are one fragment -- k slot (kb, hh, j8) <-> feature 32 (kb >> 1) + (j & 3) + 8 (j >> 2)
// + 4 (kb & 1), j = 8 hh + j8 (conflict-free ds_write_b128, no transpose).
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

#include "sigmaenv_pack.h"  // the scales MLP32S_SW / SX / SX0 and the packed form of the weights (host: sigmaenv_mlp32_create, device: sigmaenv_load.inc)

struct Mlp32sWeights {
  const f16x8_t* w[MLP32_MAX_LAYERS];  // hidden layer: [F / 32 tiles][KB][hi | lo][64 lanes] fragments; output layer: [KB][hi | lo][64 lanes]
  const float* b[MLP32_MAX_LAYERS];    // [Fp] biases times the layer's accumulator scale
  int KB[MLP32_MAX_LAYERS], F[MLP32_MAX_LAYERS];
  int n_layers;
};

struct Mlp32sW { f16x8_t h, l; };  // one weight fragment (feature tile, k block): hi / lo
// the wavefront's weight stream: fragment pair j = (tile - first tile) KB + kb, 128 fragments apart (tiles 2 w, 2 w + 1 are adjacent: the requests in flight run across the tile boundary)
__device__ __forceinline__ Mlp32sW mlp32s_ldw(const f16x8_t* __restrict__ wa, int j) {
  Mlp32sW a;
  a.h = wa[(size_t)j * 128]; a.l = wa[(size_t)j * 128 + 64];
  return a;
}

// the instruction scheduler may not move anything across a k block: without it the unrolled loops' weight requests are all hoisted to the top (16 x 8 registers)
// and the kernel spills; with it the requests stay two k blocks ahead as written
#define MLP32S_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#ifndef MLP32S_PF
#define MLP32S_PF 2  /* k blocks of weight fragments in flight per wavefront (4 measured: 69.6 against 69.3 us, 32 more registers) */
#endif
#define MLP32S_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0)
// one k block of one feature tile for both row tiles; xk: fragment (kb, hi, h, row tile 0 + m); lo is 128 fragments further, row tile 1 is 32 further.  The small
// products first; the two accumulators alternate
__device__ __forceinline__ void mlp32s_kblock(f32x16_t (&acc)[2], const Mlp32sW& a, const f16x8_t* __restrict__ xk) {
  const f16x8_t x0h = xk[0], x1h = xk[32], x0l = xk[128], x1l = xk[160];
  MLP32S_MFMA(acc[0], a.l, x0h); MLP32S_MFMA(acc[1], a.l, x1h);
  MLP32S_MFMA(acc[0], a.h, x0l); MLP32S_MFMA(acc[1], a.h, x1l);
  MLP32S_MFMA(acc[0], a.h, x0h); MLP32S_MFMA(acc[1], a.h, x1h);
}

// v (already times its scale) -> (hi, lo)
__device__ __forceinline__ void mlp32s_split(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}

// an input row element times its scale, SATURATED at the largest fp16 (|input| >= 4094: the split form would give inf - inf = nan; a saturated element is a wrong
// but finite number -- the range is the caller's contract, include/sigmaenv.h: normalised observations are < 10 in magnitude, the exact mode has no such bound)
__device__ __forceinline__ float mlp32s_sat(float v) { return fminf(fmaxf(v, -65504.0f), 65504.0f); }

// 2^8 tanh(acc / scale) with c = 2 / (ln 2 scale): 2^8 - 2^9 / (exp2(c acc) + 1) on the hardware exp2 / rcp, no branches, no range split (saturates correctly at
// both ends).  Absolute error <= ~3e-7 of the unscaled value (the rounding of e + 1 near e = 1 plus the two 1-ulp hardware functions): the epilogue is this kernel's
// vector work (64 values per lane and layer), and the activations only need absolute accuracy -- they feed dot products held to 1e-5.
__device__ __forceinline__ float mlp32s_tanh_scaled(float acc, float c) {
  const float e = __builtin_amdgcn_exp2f(acc * c);
  return fmaf(-2.0f * MLP32S_SX, __builtin_amdgcn_rcpf(e + 1.0f), MLP32S_SX);
}

// accumulator register j of both row tiles of a feature tile -> activation -> (hi, lo) slots of the next layer's fragments
__device__ __forceinline__ void mlp32s_act(const f32x16_t (&v)[2], int j, float tc, f16x8_t (&oh)[2][2], f16x8_t (&ol)[2][2]) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    _Float16 a16, b16;
    mlp32s_split(mlp32s_tanh_scaled(v[rt][j], tc), a16, b16);
    oh[rt][j >> 3][j & 7] = a16; ol[rt][j >> 3][j & 7] = b16;
  }
}

// The actor's distribution head as the kernel's epilogue (sigmaenv_actor_forward_f32 / sigmaenv_rollout_f32 in split mode): with 4 output features the lane that holds a
// row's feature 0 holds all four -- the same floats the stand-alone head kernel reads back from `out`, without its launch.
// row_map (nullptr: identity): network row r is agent row row_map[r] = env * n_agents + agent of the outputs and of the random draws; a negative entry writes nothing
// (the B-row turn forward of prioritized action propagation, sigmaenv_wrappers.inc)
struct Mlp32sHead {
  int on, n_agents, env_base, deterministic;
  float low0, low1, high0, high1;
  float *actions, *log_prob, *loc_scale;
  uint64_t seed, counter;
  const int32_t* row_map;
};
// ROWS: as sigmaenv_mlp32_kernel -- false: `in` is dense [R][in_dim], 16-byte aligned (rw is not read); true: the rows of a record (sigmaenv_mlp32_forward_rows).
// Only the input-tile staging differs; the dense instantiation compiles to what the kernel was before the strided one existed (216 VGPRs, no scratch).
// PAD (Mlp32Pad, sigmaenv_mlp32.inc): <true, true>, the padded form of the record rows, staged column by column; the other two never read `pd`.
template <bool ROWS, bool PAD = false>
__global__ void __launch_bounds__(256, 2) sigmaenv_mlp32s_kernel(Mlp32sWeights mw, const float* __restrict__ in, int R, int in_dim, float* __restrict__ out, Mlp32sHead hd,
                                                                 Mlp32Rows rw, Mlp32Pad pd MLP32_TS_ARG) {
  sigma_poison_lds();
  MLP32_TS(0);
#ifdef SIGMAENV_PROFILE
  // diagnostic: the workgroup in the odd wave slot of its SIMDs (the second of the two co-resident ones) starts `stagger` x 1024 cycles late
  if (stagger > 0 && (__builtin_amdgcn_s_getreg((3 << 11) | 4) & 1)) {
    for (int q = 0; q < stagger; ++q) __builtin_amdgcn_s_sleep(16);
  }
#endif
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int KB0 = mw.KB[0];
  const int KBA = KB0 > 16 ? KB0 : 16;
  f16x8_t* x = reinterpret_cast<f16x8_t*>(smem_raw);                           // [KBA][hi | lo][2][64] fragments: the activations of the current layer
  float* part = reinterpret_cast<float*>(x + (size_t)KBA * 256);               // [2][16][64]: partial sums of the output layer's second k half
  float* bl = part + 2 * 16 * 64;                                              // [hidden layers][256] + [32]: every layer's (scaled) biases, fetched once
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * MLP32_ROWS;
#define MLP32S_SEL(arr, l) ((l) == 0 ? mw.arr[0] : (l) == 1 ? mw.arr[1] : (l) == 2 ? mw.arr[2] : mw.arr[3])
  // what does not depend on the input rows travels first: layer 0's first two k blocks of weights
  const f16x8_t* wa0 = mw.w[0] + (size_t)(2 * wave) * KB0 * 128 + lane;
  const int J0 = 2 * KB0 - 1;
  Mlp32sW rg[MLP32S_PF];  // the weight fragments in flight: k blocks j .. j + MLP32S_PF - 1 of the wavefront's stream
#pragma unroll
  for (int d = 0; d < MLP32S_PF; ++d) rg[d] = mlp32s_ldw(wa0, d < J0 ? d : J0);  // (KB0 = 2: all of layer 0)
  for (int l = 0; l + 1 < mw.n_layers; ++l) bl[l * MLP32_H + tid] = MLP32S_SEL(b, l)[tid];
  if (tid < 32) bl[(mw.n_layers - 1) * MLP32_H + tid] = MLP32S_SEL(b, mw.n_layers - 1)[tid];
  // ---- input tile: fp32 rows -> split fragments
  if (!PAD && (in_dim & 7) == 0) {
    const int Q0 = KB0 * 2;  // fragments (of 8 columns) per row
    for (int e = tid; e < Q0 * MLP32_ROWS; e += 256) {
      const int r = e / Q0, c8 = e - r * Q0, k = c8 << 3, row = row0 + r;
      f16x8_t vh, vl;
      if (row < R && k < in_dim) {
        float4 lo4, hi4;
        if constexpr (ROWS) {
          const float* src = mlp32_row_ptr<true>(in, row, in_dim, rw) + k;
          if (rw.aligned) { lo4 = reinterpret_cast<const float4*>(src)[0]; hi4 = reinterpret_cast<const float4*>(src)[1]; }
          else mlp32_ld8_realign(src, lo4, hi4);
        } else {
          lo4 = reinterpret_cast<const float4*>(in + (size_t)row * in_dim + k)[0]; hi4 = reinterpret_cast<const float4*>(in + (size_t)row * in_dim + k)[1];
        }
        const float v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) { _Float16 a16, b16; mlp32s_split(mlp32s_sat(v[j] * MLP32S_SX0), a16, b16); vh[j] = a16; vl[j] = b16; }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { vh[j] = (_Float16)0.0f; vl[j] = (_Float16)0.0f; }
      }
      f16x8_t* d = x + (size_t)(c8 >> 1) * 256 + (c8 & 1) * 64 + r;
      d[0] = vh; d[128] = vl;
    }
  } else {
    _Float16* xs = reinterpret_cast<_Float16*>(x);
    const int K0 = KB0 * 16;
    for (int e = tid; e < K0 * MLP32_ROWS; e += 256) {
      const int r = e / K0, k = e - r * K0, row = row0 + r;
      float v = 0.0f;
      if (row < R && k < in_dim) {
        if constexpr (PAD) v = mlp32s_sat(mlp32_pad_load(mlp32_row_ptr<true>(in, row, in_dim, rw), k, pd) * MLP32S_SX0);
        else v = mlp32s_sat(mlp32_row_ptr<ROWS>(in, row, in_dim, rw)[k] * MLP32S_SX0);
      }
      _Float16 a16, b16;
      mlp32s_split(v, a16, b16);
      const size_t f = (size_t)(k >> 4) * 256 + ((k >> 3) & 1) * 64 + r;
      xs[f * 8 + (k & 7)] = a16; xs[(f + 128) * 8 + (k & 7)] = b16;
    }
  }
  __syncthreads();
  MLP32_TS(1);
  const f16x8_t* xb = x + h * 64 + m;
  f16x8_t ow[8][2];  // the output layer's weight fragments of this wavefront's k half (requested at the end of the last hidden layer)
  // One hidden layer.  FIRST (the input layer: any K, its own scale, the deeper request ring) and LAST (the output layer's weights are requested at its end) are
  // compile-time so that the registers only they need (ow) are not carried through the other layers (as one runtime loop the kernel spilled 92 registers).
  auto hidden = [&](const int l, auto first_c, auto last_c) {
    constexpr bool FIRST = decltype(first_c)::value, LAST = decltype(last_c)::value;
    // ---- hidden layer l: feature tiles 2 wave, 2 wave + 1 x row tiles 0, 1
    const int KB = FIRST ? KB0 : 16;
    const float tc = 2.8853900817779268f * (FIRST ? 1.0f / (MLP32S_SW * MLP32S_SX0) : 1.0f / (MLP32S_SW * MLP32S_SX));
    const float* bn = bl + l * MLP32_H;
    f32x16_t acc[2][2];  // [tile][row tile]
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 b4 = reinterpret_cast<const float4*>(bn + (2 * wave + ft) * 32 + 8 * g4 + 4 * h)[0];
        acc[ft][0][4 * g4 + 0] = b4.x; acc[ft][0][4 * g4 + 1] = b4.y; acc[ft][0][4 * g4 + 2] = b4.z; acc[ft][0][4 * g4 + 3] = b4.w;
        acc[ft][1][4 * g4 + 0] = b4.x; acc[ft][1][4 * g4 + 1] = b4.y; acc[ft][1][4 * g4 + 2] = b4.z; acc[ft][1][4 * g4 + 3] = b4.w;
      }
    const f16x8_t* wa = MLP32S_SEL(w, l) + (size_t)(2 * wave) * KB * 128 + lane;
    f16x8_t oh[2][2][2], ol[2][2][2];  // [tile][row tile][hh]
    // Tile by tile: the activation function of the first tile (vector unit: 32 values per lane, ~9 instructions each) is issued between the MFMAs of the second
    // (matrix unit), two values per k block -- with all four accumulators in one stream the two co-resident workgroups run their matrix and vector phases in
    // lockstep and each unit idles while the other works (79 us per 65536 rows against 70 us tile by tile; 66 us with the output layer's weights requested early).
    if (!FIRST || KB == 16) {
#pragma unroll
      for (int kb = 0; kb < 16; ++kb) {
        const Mlp32sW a = rg[kb % MLP32S_PF];
        rg[kb % MLP32S_PF] = mlp32s_ldw(wa, kb + MLP32S_PF);
        mlp32s_kblock(acc[0], a, xb + (size_t)kb * 256);
        MLP32S_SCHED_FENCE();
      }
#pragma unroll
      for (int kb = 0; kb < 16; ++kb) {
        const Mlp32sW a = rg[kb % MLP32S_PF];
        rg[kb % MLP32S_PF] = mlp32s_ldw(wa, 16 + kb + MLP32S_PF < 32 ? 16 + kb + MLP32S_PF : 31);
        mlp32s_kblock(acc[1], a, xb + (size_t)kb * 256);
        mlp32s_act(acc[0], kb, tc, oh[0], ol[0]);
        MLP32S_SCHED_FENCE();
      }
    } else if constexpr (FIRST) {
      for (int j = 0; j < 2 * KB; ++j) {  // (only the input layer: its first four fragment pairs were requested before the rows were staged)
        const Mlp32sW p = mlp32s_ldw(wa, j + MLP32S_PF < 2 * KB ? j + MLP32S_PF : 2 * KB - 1);
        const Mlp32sW a = rg[0];
        if (j < KB) mlp32s_kblock(acc[0], a, xb + (size_t)j * 256);
        else mlp32s_kblock(acc[1], a, xb + (size_t)(j - KB) * 256);
#pragma unroll
        for (int d = 0; d + 1 < MLP32S_PF; ++d) rg[d] = rg[d + 1];
        rg[MLP32S_PF - 1] = p;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) mlp32s_act(acc[0], j, tc, oh[0], ol[0]);
    }
    // the next layer's first weight fragments (the output layer: all 16 of this wavefront's k half) travel during the activation function and the barriers
    if constexpr (!LAST) {
      const f16x8_t* wn = MLP32S_SEL(w, l + 1) + (size_t)(2 * wave) * 16 * 128 + lane;
#pragma unroll
      for (int d = 0; d < MLP32S_PF; ++d) rg[d] = mlp32s_ldw(wn, d);
    } else {
      const f16x8_t* wo = MLP32S_SEL(w, l + 1) + (size_t)(8 * (wave >> 1)) * 128 + lane;
#pragma unroll
      for (int d = 0; d < 8; ++d) { ow[d][0] = wo[(size_t)d * 128]; ow[d][1] = wo[(size_t)d * 128 + 64]; }
    }
    MLP32_TS(2 + 3 * l);
    __syncthreads();  // every wavefront has READ this layer's inputs (the barrier waits for LDS traffic only: the matrix pipe may still be draining)
    MLP32_TS(3 + 3 * l);
    // first tile's outputs go out, the second tile's activation function runs while those writes drain, then its outputs
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      if (ft == 1) {
#pragma unroll
        for (int j = 0; j < 16; ++j) mlp32s_act(acc[1], j, tc, oh[1], ol[1]);
      }
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {  // k block 2 (2 wave + ft) + h of the next layer, k half hh
          f16x8_t* d = x + (size_t)(2 * (2 * wave + ft) + h) * 256 + hh * 64 + rt * 32 + m;
          d[0] = oh[ft][rt][hh]; d[128] = ol[ft][rt][hh];
        }
    }
    __syncthreads();
    MLP32_TS(4 + 3 * l);
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  if (mw.n_layers == 2) hidden(0, T_{}, T_{});
  else {
    hidden(0, T_{}, F_{});
    for (int l = 1; l + 2 < mw.n_layers; ++l) hidden(l, F_{}, F_{});
    hidden(mw.n_layers - 2, F_{}, T_{});
  }
  {
    // ---- output layer (one feature tile, K = 256): wavefront w takes row tile w & 1 and k blocks [8 kh, 8 kh + 8), kh = w >> 1
    const int l = mw.n_layers - 1, Fl = MLP32S_SEL(F, l);
    const int rt = wave & 1, kh = wave >> 1;
    const float* bo = bl + l * MLP32_H;
    f32x16_t acc;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const float4 b4 = reinterpret_cast<const float4*>(bo + 8 * g4 + 4 * h)[0];
      acc[4 * g4 + 0] = kh ? 0.0f : b4.x; acc[4 * g4 + 1] = kh ? 0.0f : b4.y; acc[4 * g4 + 2] = kh ? 0.0f : b4.z; acc[4 * g4 + 3] = kh ? 0.0f : b4.w;
    }
    const f16x8_t* xo = xb + rt * 32 + (size_t)(8 * kh) * 256;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const f16x8_t xh = xo[(size_t)d * 256], xl = xo[(size_t)d * 256 + 128];
      MLP32S_MFMA(acc, ow[d][1], xh);
      MLP32S_MFMA(acc, ow[d][0], xl);
      MLP32S_MFMA(acc, ow[d][0], xh);
    }
    if (kh) {
#pragma unroll
      for (int j = 0; j < 16; ++j) part[(rt * 16 + j) * 64 + lane] = acc[j];
    }
    MLP32_TS(12);
    __syncthreads();
    if (!kh) {
      const float inv = 1.0f / (MLP32S_SW * MLP32S_SX);
      float o4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int f = (j & 3) + 8 * (j >> 2) + 4 * h, row = row0 + rt * 32 + m;
        const float v = (acc[j] + part[(rt * 16 + j) * 64 + lane]) * inv;
        if (j < 4) o4[j] = v;
        if (f < Fl && row < R) out[(size_t)row * Fl + f] = v;
      }
      if (hd.on && h == 0 && row0 + rt * 32 + m < R) {  // (Fl == 4: features 0 .. 3 of the row are this lane's first four)
        const float low[2] = {hd.low0, hd.low1}, high[2] = {hd.high0, hd.high1};
        const int orow = hd.row_map ? hd.row_map[row0 + rt * 32 + m] : row0 + rt * 32 + m;
        if (orow >= 0)
          actor_distribution(low, high, orow, hd.n_agents, hd.env_base, o4[0], o4[1], o4[2], o4[3], hd.actions, hd.log_prob, hd.loc_scale, hd.seed, hd.counter, hd.deterministic);
      }
    }
    MLP32_TS(13);
#ifdef SIGMAENV_PROFILE
    if (ts && threadIdx.x == 0) {  // where the workgroup ran: HW_ID and the XCC id
      ts[(size_t)blockIdx.x * 16 + 14] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
      ts[(size_t)blockIdx.x * 16 + 15] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
#endif
  }
#undef MLP32S_SEL
}
