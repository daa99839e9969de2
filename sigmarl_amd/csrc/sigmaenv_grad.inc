// sigmaenv_grad.inc -- the backward pass of the exact-fp32 MLP (included by sigmaenv.hip after sigmaenv_load.inc; the contracts are in include/sigmaenv.h,
// sigmaenv_mlp32_forward_save / sigmaenv_mlp32_backward).
//
// What it computes.  Layers l = 0 .. n - 1, z_l = W_l a_l + b_l, a_{l+1} = tanh(z_l) for l < n - 1, a_0 the input rows; acts[l] = a_{l+1} is what the saving
// instantiation of the forward kernel (sigmaenv_mlp32.inc, SAVE) wrote.  With g_{n-1} = dout:
//     g_{l-1} = (g_l W_l) (.) (1 - a_l^2)       l = n - 1 .. 1        (sigmaenv_mlp32_delta_kernel)
//     dW_l    = g_l^T a_l,   db_l = sum_rows g_l                       (sigmaenv_mlp32_dw_kernel per layer, then sigmaenv_mlp32_dw_sum_kernel)
// All products are fp32 fma chains on v_mfma_f32_32x32x2_f32, as the forward's.  (A split-fp16 backward needs a scaling rule for g, whose range is not the
// forward's: out of scope, DESIGN.md section 7.)
//     dX      = g_0 W_0                                                 (the DX instantiation of the delta kernel: sigmaenv_mlp32_input_grad / sigmaenv_mlp32_backward_dx)
// the gradient with respect to the input rows, for a handle that holds layer 0's transposed form (sigmaenv_mlp32_create_input_grad).
//
// Mapping.
//  * delta: one workgroup walks a 64-row tile BACKWARDS through all layers in LDS, as the forward walks it forwards: g_l lies in the forward's activation layout
//    (mlp32_act_idx, 64 KB), the weights come from the handle's TRANSPOSED exact form (sigmaenv_pack.h: the forward's fragment layout of W^T, so that g W
//    contracts over the features with one 16-byte load per lane and k block), each wavefront owns two 32-wide tiles of the 256 outputs x both row tiles.  The chain
//    of an element runs over the features f = 0, 1, .. in order.  Epilogue: times fma(-a, a, 1) -- ONE rounding of 1 - a^2, so the factor keeps its relative
//    precision where |a| -> 1 -- one more for the product; rows past R are zeros.
//  * dX (DX): after the l = 1 epilogue g_0 is parked in LDS as every g_l above it is, and contracted with layer 0's transposed exact form [Kp / 32][32][2][32][4],
//    Kp = in_dim padded to 32: the same loop -- one 16-byte weight load per lane and k block, two blocks ahead --, a wavefront owning two 32-wide tiles of the input
//    columns x both row tiles, one pass per 256 columns; tiles at or beyond Kp are skipped (wavefront-uniform; LDS is only read here: no barrier in the passes).  An
//    element is ONE chain over f = 0 .. 255 from zero; no factor.  dX is [rows, in_dim] dense: a lane holds four consecutive columns of a row, stored with one 16-byte
//    store when in_dim is a multiple of 4 and dX 16-byte aligned (launch-uniform), else column by column; columns >= in_dim and rows >= R are never stored.
//  * dW: the contraction runs over the rows, and both operands are stored with the row as the slow index: lane (m, h) of a wavefront loads g[row 2 u + h][f0 + m]
//    and a[row 2 u + h][k0 + m] with 4-byte loads that are coalesced over m -- the operand layout of the matrix instruction as it is, no LDS.  A workgroup owns a
//    128 x 128 block of dW_l (wavefront: 2 x 2 tiles of 32 x 32, 64 accumulators) and one RANGE of rows; tiles beyond F or K are skipped (wavefront-uniform).
//    db_l: the lanes of the k block 0 add up the g values they load anyway (one chain per row parity, the two added at the end).
//  * The partition of the rows (grad::range_len): a function of `rows` alone -- at most 64 ranges, each a multiple of 64 rows and at least 256 --, never of the
//    device.  Every (range, block) writes its partial sums to the workspace; the sum kernel adds a slot's partials in range order.  No atomics: same bits every run.
//  * rows = 0: only the sum kernel runs (zero partials to add: zeros).
//  * sigmaenv_mlp32_forward_save_indexed / sigmaenv_mlp32_backward_indexed: the same kernels on a minibatch of the record's BLOCKS picked by a device index (frames of a
//    shuffled minibatch); only the two places that read input rows differ, each by an instantiation of its own (INDEXED).  Everything above holds unchanged.

namespace grad {

#define GRAD_BLK 128        // the dW kernel's output block: 128 features x 128 inputs
#define GRAD_MIN_RANGE 256  // rows
#define GRAD_MAX_RANGES 64

// the rows of one range: ceil(rows / 64) rounded up to a multiple of 64, at least GRAD_MIN_RANGE; ranges r cover [r len, min(rows, (r + 1) len))
static inline long long range_len(long long rows) {
  const long long per = ((rows + GRAD_MAX_RANGES - 1) / GRAD_MAX_RANGES + 63) / 64 * 64;
  return per < GRAD_MIN_RANGE ? GRAD_MIN_RANGE : per;
}
static inline int n_ranges(long long rows) { return rows > 0 ? (int)((rows + range_len(rows) - 1) / range_len(rows)) : 0; }

struct DeltaNet {
  const float* wt[MLP32_MAX_LAYERS];  // layer l >= 1: the transposed exact form [256 / 32][FQ_l][2][32][4]; DX: layer 0's [Kp / 32][32][2][32][4]
  int n_layers, F_last, FQ_last;      // the output layer's width and its blocks of 8
};

// DX: the instantiation that also writes dx [R][K] = g_0 W_0 (K = in_dim; dx16: K % 4 == 0 and dx 16-byte aligned, decided on the host); the other one ignores the
// last three arguments
template <bool DX>
__global__ void __launch_bounds__(256, 2) sigmaenv_mlp32_delta_kernel(DeltaNet g, const float* __restrict__ dout, const float* __restrict__ acts, float* __restrict__ delta, int R,
                                                                      float* __restrict__ dx, int K, int dx16) {
  sigma_poison_lds();
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* x = reinterpret_cast<float*>(smem_raw);  // [256 / 8][2][64][4]: g_l of the tile (mlp32_act_idx)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, h = lane >> 5;
  const long long row0 = (long long)blockIdx.x * MLP32_ROWS;
  const int FL = g.F_last, CL = g.FQ_last * 8;
  // dout tile: columns >= F_last (the padding of the contraction to 8) and rows >= R are zeros
  for (int e = tid; e < CL * MLP32_ROWS; e += blockDim.x) {
    const int n = e / CL, f = e - n * CL;
    const long long row = row0 + n;
    x[mlp32_act_idx(f, n)] = (row < R && f < FL) ? dout[(size_t)row * FL + f] : 0.0f;
  }
  __syncthreads();
  const float4* x4 = reinterpret_cast<const float4*>(x);
#define GRAD_SEL(l) ((l) == 1 ? g.wt[1] : (l) == 2 ? g.wt[2] : g.wt[3])  /* (no runtime-indexed kernel argument: that would live in scratch) */
  for (int l = g.n_layers - 1; l >= 1; --l) {
    const int KQ = l == g.n_layers - 1 ? g.FQ_last : MLP32_H / 8;
    const float4* wa = reinterpret_cast<const float4*>(GRAD_SEL(l)) + (size_t)(2 * wave) * KQ * 64 + lane;  // output tile 2 wave; 2 wave + 1 is KQ * 64 float4s further
    const float4* xb = x4 + h * MLP32_ROWS + m;                                                             // row tile 0; row tile 1 is 32 float4s further
    f32x16_t acc[2][2];
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[ft][rt][j] = 0.0f;
    const int k1 = KQ > 1 ? 1 : 0;
    float4 a0 = wa[0], a1 = wa[(size_t)KQ * 64], n0 = wa[(size_t)k1 * 64], n1 = wa[(size_t)(KQ + k1) * 64];
    for (int kq = 0; kq < KQ; ++kq) {
      const int kn = kq + 2 < KQ ? kq + 2 : KQ - 1;  // weights two blocks ahead
      const float4 p0 = wa[(size_t)kn * 64], p1 = wa[(size_t)(KQ + kn) * 64];
      const float4 b0 = xb[(size_t)kq * (MLP32_ROWS * 2)], b1 = xb[(size_t)kq * (MLP32_ROWS * 2) + 32];
      mlp32_mfma4(acc[0][0], a0, b0); mlp32_mfma4(acc[0][1], a0, b1);
      mlp32_mfma4(acc[1][0], a1, b0); mlp32_mfma4(acc[1][1], a1, b1);
      a0 = n0; a1 = n1; n0 = p0; n1 = p1;
    }
    // g_{l-1} = acc (.) (1 - a_l^2), a_l = acts[l - 1]: outputs (2 wave + ft) 32 + 8 q + 4 h + {0, 1, 2, 3} of row rt 32 + m (the forward's accumulator layout)
    const size_t layer = (size_t)(l - 1) * (size_t)R;
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const long long row = row0 + rt * 32 + m;
          float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
          if (row < R) {
            const size_t o = (layer + (size_t)row) * MLP32_H + (size_t)((2 * wave + ft) * 32 + 8 * q + 4 * h);
            const float4 a = *reinterpret_cast<const float4*>(acts + o);
            d = make_float4(acc[ft][rt][4 * q + 0] * fmaf(-a.x, a.x, 1.0f), acc[ft][rt][4 * q + 1] * fmaf(-a.y, a.y, 1.0f), acc[ft][rt][4 * q + 2] * fmaf(-a.z, a.z, 1.0f),
                            acc[ft][rt][4 * q + 3] * fmaf(-a.w, a.w, 1.0f));
            *reinterpret_cast<float4*>(delta + o) = d;
          }
          acc[ft][rt][4 * q + 0] = d.x; acc[ft][rt][4 * q + 1] = d.y; acc[ft][rt][4 * q + 2] = d.z; acc[ft][rt][4 * q + 3] = d.w;
        }
    if (l > 1 || DX) {  // (DX: g_0 is parked too)
      __syncthreads();  // every wavefront is done reading g_l
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // as the forward's store: k block kq2, slots (u, parity) = (2 h + (i >> 1), i & 1)
            const int kq2 = (2 * wave + ft) * 4 + q, row = rt * 32 + m;
            float* d = x + ((((size_t)kq2 * 2) * MLP32_ROWS + row) << 2) + 2 * h;
            *reinterpret_cast<float2*>(d) = make_float2(acc[ft][rt][4 * q + 0], acc[ft][rt][4 * q + 2]);
            *reinterpret_cast<float2*>(d + MLP32_ROWS * 4) = make_float2(acc[ft][rt][4 * q + 1], acc[ft][rt][4 * q + 3]);
          }
      __syncthreads();
    }
  }
#undef GRAD_SEL
  if constexpr (DX) {
    // dX = g_0 W_0: column tiles 2 wave, 2 wave + 1 of each pass of 8; LDS is only read from here on
    const int KT = (K + 31) / 32;
    const float4* xb = x4 + h * MLP32_ROWS + m;
    for (int t0 = 2 * wave; t0 < KT; t0 += 8) {
      const bool on1 = t0 + 1 < KT;  // the wavefront's second tile exists (else its fragments are the first tile's again: never beyond the form; not stored)
      const int KQ = MLP32_H / 8;
      const size_t o1 = on1 ? (size_t)KQ * 64 : 0;
      const float4* wa = reinterpret_cast<const float4*>(g.wt[0]) + (size_t)t0 * KQ * 64 + lane;
      f32x16_t acc[2][2];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[ft][rt][j] = 0.0f;
      float4 a0 = wa[0], a1 = wa[o1], n0 = wa[64], n1 = wa[o1 + 64];
      for (int kq = 0; kq < KQ; ++kq) {
        const int kn = kq + 2 < KQ ? kq + 2 : KQ - 1;  // weights two blocks ahead
        const float4 p0 = wa[(size_t)kn * 64], p1 = wa[o1 + (size_t)kn * 64];
        const float4 b0 = xb[(size_t)kq * (MLP32_ROWS * 2)], b1 = xb[(size_t)kq * (MLP32_ROWS * 2) + 32];
        mlp32_mfma4(acc[0][0], a0, b0); mlp32_mfma4(acc[0][1], a0, b1);
        mlp32_mfma4(acc[1][0], a1, b0); mlp32_mfma4(acc[1][1], a1, b1);
        a0 = n0; a1 = n1; n0 = p0; n1 = p1;
      }
      // columns (t0 + ft) 32 + 8 q + 4 h + {0, 1, 2, 3} of row rt 32 + m
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const long long row = row0 + rt * 32 + m;
            const int k = (t0 + ft) * 32 + 8 * q + 4 * h;
            if (row >= R || k >= K) continue;  // (a tile at or beyond Kp lies beyond K)
            float* d = dx + (size_t)row * K + k;
            if (dx16) {
              *reinterpret_cast<float4*>(d) = make_float4(acc[ft][rt][4 * q + 0], acc[ft][rt][4 * q + 1], acc[ft][rt][4 * q + 2], acc[ft][rt][4 * q + 3]);
            } else {
              d[0] = acc[ft][rt][4 * q + 0];
              if (k + 1 < K) d[1] = acc[ft][rt][4 * q + 1];
              if (k + 2 < K) d[2] = acc[ft][rt][4 * q + 2];
              if (k + 3 < K) d[3] = acc[ft][rt][4 * q + 3];
            }
          }
    }
  }
}

// one layer's dW / db partial sums
struct DwLayer {
  const float* g;  // [R][gs]: g_l (delta[l], gs = 256; the output layer: dout, gs = F)
  const float* a;  // a_l: acts[l - 1] [R][256], or (INPUT) the network's input rows
  float *pw, *pb;  // partials [n_ranges][F][K], [n_ranges][F]
  int F, K, gs, R;
  long long len;   // rows per range
};

// INDEXED (INPUT only; sigmaenv_mlp32_backward_indexed): a third instantiation whose input rows are blocks picked by `ix` (Mlp32Index, sigmaenv_mlp32.inc).  A lane loads
// the index entry of each of its rows once (the 32 lanes of a half-wavefront read the same word) and both of its columns from that row; a row whose entry is outside the
// record contributes zeros to dW_0, as a row past the range does.  g, the partition and the order of the chains are those of the other two.
// PAD (with INDEXED; sigmaenv_mlp32_backward_indexed_pad): a fourth instantiation whose input rows are padded (Mlp32Pad, sigmaenv_mlp32.inc): a lane's two columns map
// to their segments' source floats, or are zero in the padding -- dW_0's columns of the padding are exact zeros, as the dense call on the padded copy gives them.
template <bool INPUT, bool INDEXED = false, bool PAD = false>
__global__ void __launch_bounds__(256) sigmaenv_mlp32_dw_kernel(DwLayer p, Mlp32Rows rw, Mlp32Index ix, Mlp32Pad pd) {
  sigma_poison_lds();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, h = lane >> 5;
  const int nkb = (p.K + GRAD_BLK - 1) / GRAD_BLK;
  const int fb = blockIdx.x / nkb, kb = blockIdx.x - fb * nkb, range = blockIdx.y;
  const int f0 = fb * GRAD_BLK + (wave & 1) * 64, k0 = kb * GRAD_BLK + (wave >> 1) * 64;
  if (f0 >= p.F || k0 >= p.K) return;  // (wavefront-uniform; the kernel has no barrier)
  const bool f_on1 = f0 + 32 < p.F, k_on1 = k0 + 32 < p.K;  // the wavefront's second tiles exist
  const bool lf0 = f0 + m < p.F, lf1 = f0 + 32 + m < p.F, lk0 = k0 + m < p.K, lk1 = k0 + 32 + m < p.K;
  const long long r_lo = (long long)range * p.len, r_end = r_lo + p.len < p.R ? r_lo + p.len : p.R;
  f32x16_t acc[2][2];
#pragma unroll
  for (int tf = 0; tf < 2; ++tf)
#pragma unroll
    for (int tk = 0; tk < 2; ++tk)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[tf][tk][j] = 0.0f;
  float bs0 = 0.0f, bs1 = 0.0f;
  for (long long r = r_lo; r < r_end; r += 8) {
    float gv[2][4], av[2][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // rows r + 2 u + h; a row past the range contributes exact zeros (both operands)
      const long long row = r + 2 * u + h;
      const bool ok = row < r_end;
      const float* gp = p.g + (size_t)row * p.gs + f0 + m;
      const float* ap;
      bool a_ok = ok;
      if constexpr (INDEXED) {
        const long long off = ok ? mlp32_indexed_row_offset((int)row, rw, ix) : -1ll;
        a_ok = off >= 0;
        if constexpr (PAD) ap = p.a + (a_ok ? off : 0ll);  // (the row: mlp32_pad_load maps the columns)
        else ap = p.a + (a_ok ? off : 0ll) + k0 + m;
      } else if constexpr (INPUT) ap = mlp32_row_ptr<true>(p.a, ok ? (int)row : 0, 0, rw) + k0 + m;
      else ap = p.a + (size_t)row * MLP32_H + k0 + m;
      gv[0][u] = ok && lf0 ? gp[0] : 0.0f;
      gv[1][u] = ok && lf1 ? gp[32] : 0.0f;
      if constexpr (PAD) {
        av[0][u] = a_ok && lk0 ? mlp32_pad_load(ap, k0 + m, pd) : 0.0f;
        av[1][u] = a_ok && lk1 ? mlp32_pad_load(ap, k0 + 32 + m, pd) : 0.0f;
      } else {
        av[0][u] = a_ok && lk0 ? ap[0] : 0.0f;
        av[1][u] = a_ok && lk1 ? ap[32] : 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[0][u], av[0][u], acc[0][0], 0, 0, 0);
      if (k_on1) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[0][u], av[1][u], acc[0][1], 0, 0, 0);
      if (f_on1) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[1][u], av[0][u], acc[1][0], 0, 0, 0);
      if (f_on1 && k_on1) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[1][u], av[1][u], acc[1][1], 0, 0, 0);
      bs0 = bs0 + gv[0][u];
      bs1 = bs1 + gv[1][u];
    }
  }
  // accumulator j of lane (m, h): feature (j & 3) + 8 (j >> 2) + 4 h of the tile, input column m
#pragma unroll
  for (int tf = 0; tf < 2; ++tf)
#pragma unroll
    for (int tk = 0; tk < 2; ++tk)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int f = f0 + 32 * tf + (j & 3) + 8 * (j >> 2) + 4 * h, k = k0 + 32 * tk + m;
        if (f < p.F && k < p.K) p.pw[((size_t)range * p.F + f) * p.K + k] = acc[tf][tk][j];
      }
  if (k0 == 0) {  // db: even rows' chain + odd rows' chain
    const float s0 = bs0 + __shfl_xor(bs0, 32), s1 = bs1 + __shfl_xor(bs1, 32);
    if (h == 0 && lf0) p.pb[(size_t)range * p.F + f0 + m] = s0;
    if (h == 0 && lf1) p.pb[(size_t)range * p.F + f0 + 32 + m] = s1;
  }
}

// grad[i] = partial[0][i] + partial[1][i] + ... in range order (no range: zero); i over the nw weights, then the nb biases
__global__ void __launch_bounds__(256) sigmaenv_mlp32_dw_sum_kernel(const float* __restrict__ pw, const float* __restrict__ pb, int ranges, int nw, int nb, float* __restrict__ gw,
                                                                    float* __restrict__ gb) {
  sigma_poison_lds();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nw + nb) return;
  const bool bias = i >= nw;
  const float* src = bias ? pb + (i - nw) : pw + i;
  const size_t step = bias ? (size_t)nb : (size_t)nw;
  float s = 0.0f;
  if (ranges > 0) s = src[0];
  for (int r = 1; r < ranges; ++r) s = s + src[(size_t)r * step];
  if (bias) gb[i - nw] = s; else gw[i] = s;
}

// the transposed exact form of one layer, every slot (padding: zeros): the per-slot function of sigmaenv_pack.h, which sigmaenv_mlp32_create runs on the host
__global__ void __launch_bounds__(256) sigmaenv_load_mlp32_t_kernel(const float* __restrict__ w, float* __restrict__ tw, int F, int K, int n) {
  sigma_poison_lds();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) pack_mlp32_t_slot(w, tw, F, K, i);
}

static inline size_t partial_floats(const sigmaenv_mlp32* m) {  // one range's partials of the largest layer, weights then biases
  size_t mx = 0;
  for (int l = 0; l < m->w.n_layers; ++l) { const size_t n = (size_t)m->dims[l] * m->dims[l + 1]; mx = n > mx ? n : mx; }
  return mx + MLP32_H;
}

}  // namespace grad

static int mlp32_grad_load(sigmaenv_t* h, sigmaenv_mlp32* m, const float* const* weights_dev) {
  for (int l = m->wt[0] ? 0 : 1; l < m->w.n_layers; ++l) {  // (layer 0's form: a handle made by sigmaenv_mlp32_create_input_grad)
    const int K = m->dims[l], F = m->dims[l + 1], n = load_exact_t_slots(F, K);
    hipLaunchKernelGGL(grad::sigmaenv_load_mlp32_t_kernel, dim3(load::grid_for(n)), dim3(256), 0, h->stream, weights_dev[l], m->wt[l], F, K, n);
    HIPCHK(h, hipGetLastError());
  }
  return SIGMAENV_OK;
}

// index == nullptr: the rows' blocks are the record's blocks 0 .. n_blocks - 1 (sigmaenv_mlp32_forward_save); else the n_index blocks index[.] of its n_blocks
static int mlp32_forward_save_impl(sigmaenv_t* h, sigmaenv_mlp32* m, const char* what, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                   int64_t block_stride, const int32_t* index, int32_t n_index, float* out, float* acts, const Mlp32Pad* pad = nullptr) {
  if (!h) return SIGMAENV_EINVAL;
  if (!m) { h->err = std::string(what) + ": null network handle"; return SIGMAENV_EINVAL; }
  Mlp32View v;
  if (const int rc = mlp32_view(h, m, what, in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, pad, &v)) return rc;
  if (v.rows > 0 && (!out || !acts || ((uintptr_t)out & 3) || ((uintptr_t)acts & 15))) { h->err = std::string(what) + ": null out / acts, or acts not 16-byte aligned"; return SIGMAENV_EINVAL; }
  return mlp32_launch(h, m, v, out, acts, nullptr, nullptr);  // (no rows: OK, nothing is launched)
}

extern "C" int sigmaenv_mlp32_forward_save(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                           float* out, float* acts) {
  return mlp32_forward_save_impl(h, m, "mlp32_forward_save", in, rows_per_block, row_stride, n_blocks, block_stride, nullptr, 0, out, acts);
}
extern "C" int sigmaenv_mlp32_forward_save_indexed(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                                   int64_t block_stride, const int32_t* index, int32_t n_index, float* out, float* acts) {
  if (h && !index && n_index == 0) return SIGMAENV_OK;  // (an empty minibatch: no row)
  return mlp32_forward_save_impl(h, m, "mlp32_forward_save_indexed", in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, out, acts);
}
// the same on padded rows (Mlp32Pad, sigmaenv_mlp32.inc): the row in memory holds in_dim / seg_dst segments of seg_src floats
extern "C" int sigmaenv_mlp32_forward_save_indexed_pad(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                                       int64_t block_stride, const int32_t* index, int32_t n_index, int32_t seg_src, int32_t seg_dst, float* out, float* acts) {
  if (h && !index && n_index == 0) return SIGMAENV_OK;
  const Mlp32Pad pd{seg_src, seg_dst};
  return mlp32_forward_save_impl(h, m, "mlp32_forward_save_indexed_pad", in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, out, acts, &pd);
}

extern "C" int sigmaenv_mlp32_backward_workspace(const sigmaenv_mlp32* m, int64_t rows, uint64_t* n_floats) {
  if (!m || !n_floats || rows < 0 || rows > INT32_MAX) return SIGMAENV_EINVAL;
  *n_floats = (uint64_t)(m->w.n_layers - 1) * (uint64_t)rows * MLP32_H + (uint64_t)grad::n_ranges(rows) * grad::partial_floats(m);
  return SIGMAENV_OK;
}

// the delta launch: g_l, l = n - 2 .. 0, into delta [n - 1][R][256]; dx (not null: the DX instantiation, the handle holds layer 0's transposed form) [R][in_dim] as well
static int mlp32_delta_launch(sigmaenv_t* h, const sigmaenv_mlp32* m, const float* acts, const float* dout, float* delta, int R, float* dx) {
  const int n = m->w.n_layers;
  grad::DeltaNet g{};
  for (int l = dx ? 0 : 1; l < n; ++l) g.wt[l] = m->wt[l];
  g.n_layers = n; g.F_last = m->out_dim; g.FQ_last = (m->out_dim + 7) / 8;
  const dim3 grid((unsigned)(((int64_t)R + MLP32_ROWS - 1) / MLP32_ROWS));
  const size_t smem = (size_t)MLP32_H * MLP32_ROWS * sizeof(float);
  if (dx) {
    const int dx16 = (m->in_dim & 3) == 0 && ((uintptr_t)dx & 15) == 0;
    hipLaunchKernelGGL(grad::sigmaenv_mlp32_delta_kernel<true>, grid, dim3(256), smem, h->stream, g, dout, acts, delta, R, dx, m->in_dim, dx16);
  } else {
    hipLaunchKernelGGL(grad::sigmaenv_mlp32_delta_kernel<false>, grid, dim3(256), smem, h->stream, g, dout, acts, delta, R, (float*)nullptr, 0, 0);
  }
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

// the refusals of both entry points that write dx, made before any launch
static int mlp32_dx_check(sigmaenv_t* h, const sigmaenv_mlp32* m, const std::string& what, int64_t rows, const float* dx) {
  if (!m->wt[0]) { h->err = what + ": the handle does not hold layer 0's transposed form: create it with sigmaenv_mlp32_create_input_grad"; return SIGMAENV_EINVAL; }
  if (rows > 0 && (!dx || ((uintptr_t)dx & 3))) { h->err = what + ": a null dx or one that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  return SIGMAENV_OK;
}

// dx: nullptr for the entry points without it; want_dx: sigmaenv_mlp32_backward_dx
static int mlp32_backward_impl(sigmaenv_t* h, sigmaenv_mlp32* m, const char* what_c, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                               int64_t block_stride, const int32_t* index, int32_t n_index, const float* acts, const float* dout, float* workspace, float* const* grad_w,
                               float* const* grad_b, const Mlp32Pad* pad = nullptr, bool want_dx = false, float* dx = nullptr) {
  if (!h) return SIGMAENV_EINVAL;
  const std::string what(what_c);
  if (!m) { h->err = what + ": null network handle"; return SIGMAENV_EINVAL; }
  const int n = m->w.n_layers;
  if (!grad_w || !grad_b) { h->err = what + ": null gradient pointer array"; return SIGMAENV_EINVAL; }
  for (int l = 0; l < n; ++l)
    if (!grad_w[l] || !grad_b[l] || ((uintptr_t)grad_w[l] & 3) || ((uintptr_t)grad_b[l] & 3)) {
      h->err = what + ": layer " + std::to_string(l) + ": a null gradient tensor or one that is not 4-byte aligned";
      return SIGMAENV_EINVAL;
    }
  Mlp32View v;
  if (const int rc = mlp32_view(h, m, what_c, in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, pad, &v)) return rc;
  if (v.padded && !v.indexed) { h->err = what + ": padded rows are built for the indexed backward"; return SIGMAENV_EINVAL; }  // (no such dW instantiation)
  const int64_t rows = v.rows;
  if (rows > 0 && (!acts || !dout || !workspace || ((uintptr_t)acts & 15) || ((uintptr_t)dout & 3) || ((uintptr_t)workspace & 15))) {
    h->err = what + ": null acts / dout / workspace, or acts / workspace not 16-byte aligned";
    return SIGMAENV_EINVAL;
  }
  if (want_dx) { if (const int rc = mlp32_dx_check(h, m, what, rows, dx)) return rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const int R = (int)rows, ranges = grad::n_ranges(rows);
  float* delta = workspace;                                            // [n - 1][R][256]
  float* pw = workspace ? workspace + (size_t)(n - 1) * (size_t)R * MLP32_H : nullptr;  // [ranges][F K] then [ranges][F] of the layer in work
  if (R > 0) { if (const int rc = mlp32_delta_launch(h, m, acts, dout, delta, R, want_dx ? dx : nullptr)) return rc; }
  for (int l = n - 1; l >= 0; --l) {
    const int K = m->dims[l], F = m->dims[l + 1];
    float* pb = pw ? pw + (size_t)ranges * F * K : nullptr;
    if (R > 0) {
      grad::DwLayer p{};
      p.g = l == n - 1 ? dout : delta + (size_t)l * (size_t)R * MLP32_H;
      p.gs = l == n - 1 ? F : MLP32_H;
      p.a = l == 0 ? v.in : acts + (size_t)(l - 1) * (size_t)R * MLP32_H;
      p.pw = pw; p.pb = pb; p.F = F; p.K = K; p.R = R; p.len = grad::range_len(rows);
      const dim3 grid((unsigned)(((F + GRAD_BLK - 1) / GRAD_BLK) * ((K + GRAD_BLK - 1) / GRAD_BLK)), (unsigned)ranges);
      // (layer 0 reads the input rows where the view says they are; its three instantiations get the view's structs, zeros where not in force)
      if (l == 0 && v.padded) hipLaunchKernelGGL((grad::sigmaenv_mlp32_dw_kernel<true, true, true>), grid, dim3(256), 0, h->stream, p, v.rw, v.ix, v.pd);
      else if (l == 0 && v.indexed) hipLaunchKernelGGL((grad::sigmaenv_mlp32_dw_kernel<true, true>), grid, dim3(256), 0, h->stream, p, v.rw, v.ix, v.pd);
      else if (l == 0) hipLaunchKernelGGL(grad::sigmaenv_mlp32_dw_kernel<true>, grid, dim3(256), 0, h->stream, p, v.rw, v.ix, v.pd);
      else hipLaunchKernelGGL(grad::sigmaenv_mlp32_dw_kernel<false>, grid, dim3(256), 0, h->stream, p, Mlp32Rows{}, Mlp32Index{}, Mlp32Pad{});
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(grad::sigmaenv_mlp32_dw_sum_kernel, dim3((unsigned)((F * K + F + 255) / 256)), dim3(256), 0, h->stream, pw, pb, ranges, F * K, F, grad_w[l], grad_b[l]);
    HIPCHK(h, hipGetLastError());
  }
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_mlp32_backward(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                       const float* acts, const float* dout, float* workspace, float* const* grad_w, float* const* grad_b) {
  return mlp32_backward_impl(h, m, "mlp32_backward", in, rows_per_block, row_stride, n_blocks, block_stride, nullptr, 0, acts, dout, workspace, grad_w, grad_b);
}
extern "C" int sigmaenv_mlp32_backward_indexed(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                               int64_t block_stride, const int32_t* index, int32_t n_index, const float* acts, const float* dout, float* workspace,
                                               float* const* grad_w, float* const* grad_b) {
  // (an empty minibatch is the rows = 0 case of sigmaenv_mlp32_backward: the gradients are written as zeros)
  if (!index && n_index == 0) return mlp32_backward_impl(h, m, "mlp32_backward_indexed", in, rows_per_block, row_stride, 0, block_stride, nullptr, 0, acts, dout, workspace, grad_w, grad_b);
  return mlp32_backward_impl(h, m, "mlp32_backward_indexed", in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, acts, dout, workspace, grad_w, grad_b);
}
// the same on padded rows (sigmaenv_mlp32_forward_save_indexed_pad's): dW_0's columns of the padding are zeros
extern "C" int sigmaenv_mlp32_backward_indexed_pad(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks,
                                                   int64_t block_stride, const int32_t* index, int32_t n_index, int32_t seg_src, int32_t seg_dst, const float* acts,
                                                   const float* dout, float* workspace, float* const* grad_w, float* const* grad_b) {
  if (!index && n_index == 0) return mlp32_backward_impl(h, m, "mlp32_backward_indexed_pad", in, rows_per_block, row_stride, 0, block_stride, nullptr, 0, acts, dout, workspace, grad_w, grad_b);
  const Mlp32Pad pd{seg_src, seg_dst};
  return mlp32_backward_impl(h, m, "mlp32_backward_indexed_pad", in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, acts, dout, workspace, grad_w, grad_b, &pd);
}

// ---- the gradient with respect to the input rows (contracts: include/sigmaenv.h) ----
extern "C" int sigmaenv_mlp32_input_grad_workspace(const sigmaenv_mlp32* m, int64_t rows, uint64_t* n_floats) {
  if (!m || !n_floats || rows < 0 || rows > INT32_MAX) return SIGMAENV_EINVAL;
  *n_floats = (uint64_t)(m->w.n_layers - 1) * (uint64_t)rows * MLP32_H;  // g_l, l = 0 .. n - 2
  return SIGMAENV_OK;
}
extern "C" int sigmaenv_mlp32_input_grad(sigmaenv_t* h, sigmaenv_mlp32* m, const float* acts, const float* dout, int32_t rows, float* workspace, float* dx) {
  if (!h) return SIGMAENV_EINVAL;
  const std::string what("mlp32_input_grad");
  if (!m) { h->err = what + ": null network handle"; return SIGMAENV_EINVAL; }
  if (rows < 0) { h->err = what + ": a negative row count"; return SIGMAENV_EINVAL; }
  if (rows > 0 && (!acts || !dout || !workspace || ((uintptr_t)acts & 15) || ((uintptr_t)dout & 3) || ((uintptr_t)workspace & 15))) {
    h->err = what + ": null acts / dout / workspace, or acts / workspace not 16-byte aligned";
    return SIGMAENV_EINVAL;
  }
  if (const int rc = mlp32_dx_check(h, m, what, rows, dx)) return rc;
  if (rows == 0) return SIGMAENV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  return mlp32_delta_launch(h, m, acts, dout, workspace, rows, dx);
}
// index == nullptr and n_index == 0: the rows are the record's blocks (sigmaenv_mlp32_backward); seg_src == seg_dst == 0: no padding
extern "C" int sigmaenv_mlp32_backward_dx(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                          const int32_t* index, int32_t n_index, int32_t seg_src, int32_t seg_dst, const float* acts, const float* dout, float* workspace,
                                          float* const* grad_w, float* const* grad_b, float* dx) {
  const Mlp32Pad pd{seg_src, seg_dst};
  return mlp32_backward_impl(h, m, "mlp32_backward_dx", in, rows_per_block, row_stride, n_blocks, block_stride, index, n_index, acts, dout, workspace, grad_w, grad_b,
                             seg_src || seg_dst ? &pd : nullptr, true, dx);
}
