// sigmaenv_mlp32.inc -- exact-fp32 multilayer perceptron on the matrix cores (included by sigmaenv.hip after sigmaenv_actor.inc).
//
// What it restates: torchrl's MultiAgentMLP with shared parameters as the reference instantiates it, in the reference's own precision --
//   actor   decision_making_module.py:34-52  (decentralised: input = the agent's observation, D -> 256 -> 256 -> 256 -> 4, Tanh), fp32
//   critic  optimization_module.py:16-32     (MAPPO, centralised = True: input = the observations of ALL agents of the env concatenated,
//                                             N D -> 256 -> 256 -> 256 -> 1, Tanh; the one value is every agent's state value), fp32
// The bf16 kernel of sigmaenv_actor.inc is the fast inference variant (narrower arithmetic than the reference: opt-in); this one is the
// parity variant: v_mfma_f32_32x32x2_f32 is an exact fp32 fma chain (one rounding per product, k-ordered), i.e. the same arithmetic class as
// torch.nn.Linear on the CPU up to the summation order.
//
// Mapping (round 3).  One workgroup (4 wavefronts) owns MLP32_ROWS = 64 input rows (two MFMA row tiles) through ALL layers.
//  * Operands arrive 128 bits at a time.  v_mfma_f32_32x32x2_f32 takes ONE float per lane for A (lane l: A[m = l & 31][k = l >> 5]) and one for B
//    (B[k = l >> 5][n = l & 31]); a k block of 8 is four such steps, k = 8 kq + 2 u + h with h = l >> 5.  Both operand stores are laid out so that a lane's
//    four values u = 0..3 of a k block are consecutive: the weights on the host ([feature tile][kq][h][m][u], one coalesced global_load_dwordx4 per
//    lane and k block), the activations in LDS ([kq][h][row][u], one ds_read_b128).  One weight fragment feeds both row tiles, one activation fragment
//    both feature tiles of the wavefront: 16 MFMAs per 4 wide loads (the round-2 kernel issued one dword load and one ds_read_b32 per MFMA and
//    reached 47 % of the matrix rate).
//  * A hidden layer is 8 feature tiles of 32: two per wavefront x two row tiles = four independent 32 x 32 accumulator chains (64 VGPRs), K / 2 MFMAs
//    each; the weight fragments of the next two k blocks are in flight while a block is multiplied.
//  * ONE activation buffer: a layer's outputs overwrite its inputs after a workgroup barrier (every wavefront needs all 256 input features until its
//    chains end), 64 KB + 8 KB scratch for 64 rows -> two workgroups per CU, so that one's tanh / store phase overlaps the other's MFMAs.
//  * The output layer has one feature tile: its K is split over the wavefront pairs (wavefront w: row tile w & 1, k half w >> 1), the two partial sums are
//    added through LDS.  (Summation order differs from torch's and from round 2's: the results agree to rounding, tests/test_gpu_actor.py.)
// 65536 rows x 18.4 GFLOP at the 157 TF f32 matrix rate is 0.117 ms.
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#define MLP32_ROWS 64
#define MLP32_MAX_LAYERS 4
#include "sigmaenv_pack.h"  // MLP32_H (the hidden width) and the packed forms of the weights
#define MLP32_KC 256  // layer 0's input columns staged in LDS at a time (a wider input is multiplied chunk by chunk: the LDS per workgroup does not grow with it)

struct Mlp32Weights {
  const float* w[MLP32_MAX_LAYERS];  // layer l packed [Fp_l / 32][K_l / 8][2][32][4] (see above; K padded to a multiple of 8, features to 32, zeros)
  const float* b[MLP32_MAX_LAYERS];  // [Fp_l]
  int K[MLP32_MAX_LAYERS], F[MLP32_MAX_LAYERS], Fp[MLP32_MAX_LAYERS];
  int n_layers;
};

// LDS index of activation (feature k, row) in the packed layout [k >> 3][k & 1][row][(k & 7) >> 1]: the 32 lanes of a half-wavefront read 32 consecutive
// 16-byte fragments (bank-conflict free; with the row in front of the k parity every ds_read_b128 had 2-way conflicts: 64 % conflict cycles)
__device__ __forceinline__ int mlp32_act_idx(int k, int row) { return ((((k >> 3) * 2 + (k & 1)) * MLP32_ROWS + row) << 2) + ((k & 7) >> 1); }

// Where the network's rows are (sigmaenv_mlp32_forward_rows): row r = t * rpb + b at in + t * block_stride + b * row_stride (floats), e.g. the observation part of the
// rows of a [T, B_total, W] rollout record.  aligned (launch-uniform, decided on the host): base and both strides are multiples of 4 floats -- 16-byte loads as in the
// dense kernels; otherwise the rows are only 4-byte aligned (W = N (D + 1) + 1 is odd) and the tile is read through the realigning loads below.
struct Mlp32Rows {
  int rpb, aligned;
  long long row_stride, block_stride;
};
template <bool ROWS>
__device__ __forceinline__ const float* mlp32_row_ptr(const float* __restrict__ in, int row, int in_dim, const Mlp32Rows& rw) {
  if constexpr (ROWS) {
    const int t = row / rw.rpb, b = row - t * rw.rpb;
    return in + (long long)t * rw.block_stride + (long long)b * rw.row_stride;
  } else {
    return in + (size_t)row * in_dim;
  }
}
// Indexed blocks (sigmaenv_mlp32_forward_save_indexed / sigmaenv_mlp32_backward_indexed): block t of the rows is block index[t] of the record, i.e. row r = t * rpb + b
// lies at in + index[t] * block_stride + b * row_stride.  An entry outside [0, n_blocks) is never used as an address: the row is staged as zeros, as a row beyond R is.
struct Mlp32Index {
  const int32_t* index;  // device i32 [rows / rpb]
  int n_blocks;          // the record's block count: the bound on the entries
};
// the float offset of row `row` (< the row count) from `in`, or -1 for an entry outside the record.  ONE load of the entry per row: the callers keep the offset
__device__ __forceinline__ long long mlp32_indexed_row_offset(int row, const Mlp32Rows& rw, const Mlp32Index& ix) {
  const int t = row / rw.rpb, b = row - t * rw.rpb;
  const int f = ix.index[t];
  return (unsigned)f < (unsigned)ix.n_blocks ? (long long)f * rw.block_stride + (long long)b * rw.row_stride : -1ll;
}
// Padded rows (sigmaenv_mlp32_forward_rows_pad / sigmaenv_mlp32_forward_save_indexed_pad / sigmaenv_mlp32_backward_indexed_pad): the network's input row is in_dim / dst
// segments of width dst, the row in memory the same number of segments of width src <= dst: network column k = a * dst + j reads the row's float a * src + j for
// j < src and is zero for j >= src -- the base critic's next rows (per agent the D floats of the record's next observation, then 2 K zeros), staged without a padded
// copy in HBM.  A segment boundary may fall inside a 16-byte granule, so the padded instantiations stage column by column (the loop of an input width that is no
// multiple of 4); what is staged is what a dense call stages from the padded copy, so the results are its bits.
struct Mlp32Pad {
  int src, dst;
};
__device__ __forceinline__ float mlp32_pad_load(const float* __restrict__ row, int k, const Mlp32Pad& pd) {
  const int a = k / pd.dst, j = k - a * pd.dst;
  return j < pd.src ? row[a * pd.src + j] : 0.0f;
}
// Host side: where the rows of one call are -- the three structs above as the kernels get them (zeros where not in force) and which of them are in force.  Every
// row-taking entry point fills one from its raw arguments (mlp32_view, which holds all the checks); the forward's one launch site (mlp32_launch) and the backward's
// choice of the dW kernel read it.  by_rows false: `in` is dense [rows][in_dim], 16-byte aligned (mlp32_forward_impl).
struct Mlp32View {
  const char* what;  // the entry point's name, the prefix of its messages
  const float* in;
  int rows;
  Mlp32Rows rw;
  Mlp32Index ix;
  Mlp32Pad pd;
  bool by_rows, indexed, padded;
};
// Four (eight) floats at a 4-byte-aligned address p from 16-byte-ALIGNED loads: the granule that holds p[0] and the following one (two), each only when it holds
// one of the wanted floats -- so no load touches a granule without a valid float, and an aligned granule never crosses a page --, the wanted floats selected by
// s = the offset of p in its granule.  A row's lanes read consecutive granules: the requests coalesce as those of the aligned path do (3 loads per 8 floats, not 2).
__device__ __forceinline__ float mlp32_sel4(int s, float a, float b, float c, float d) { return s == 0 ? a : s == 1 ? b : s == 2 ? c : d; }
__device__ __forceinline__ float4 mlp32_ld4_realign(const float* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const int s = (int)((a >> 2) & 3);
  const float4* g = reinterpret_cast<const float4*>(a & ~(uintptr_t)15);
  const float4 w0 = g[0];
  const float4 w1 = s ? g[1] : w0;
  return make_float4(mlp32_sel4(s, w0.x, w0.y, w0.z, w0.w), mlp32_sel4(s, w0.y, w0.z, w0.w, w1.x), mlp32_sel4(s, w0.z, w0.w, w1.x, w1.y), mlp32_sel4(s, w0.w, w1.x, w1.y, w1.z));
}
__device__ __forceinline__ void mlp32_ld8_realign(const float* p, float4& lo, float4& hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const int s = (int)((a >> 2) & 3);
  const float4* g = reinterpret_cast<const float4*>(a & ~(uintptr_t)15);
  const float4 w0 = g[0], w1 = g[1];
  const float4 w2 = s ? g[2] : w1;
  lo = make_float4(mlp32_sel4(s, w0.x, w0.y, w0.z, w0.w), mlp32_sel4(s, w0.y, w0.z, w0.w, w1.x), mlp32_sel4(s, w0.z, w0.w, w1.x, w1.y), mlp32_sel4(s, w0.w, w1.x, w1.y, w1.z));
  hi = make_float4(mlp32_sel4(s, w1.x, w1.y, w1.z, w1.w), mlp32_sel4(s, w1.y, w1.z, w1.w, w2.x), mlp32_sel4(s, w1.z, w1.w, w2.x, w2.y), mlp32_sel4(s, w1.w, w2.x, w2.y, w2.z));
}

// tanh without branches (the library tanhf is ~35 instructions with divergent range branches, 192 of them per lane and forward were the kernel's
// vector work): |x| < 0.3: the odd Taylor polynomial through x^9 (truncation < 6e-8 relative); else 1 - 2 / (exp(2 |x|) + 1) with the hardware exp2 /
// rcp (1 ulp each), sign restored.  <= ~4 ulp (1.1e-7 absolute) against the correctly rounded tanh -- torch's own vectorised tanh is a 1-ulp routine --,
// i.e. the outputs move by a few 1e-7 against torch.nn, an order of magnitude inside the 1e-5 bar (tests/test_gpu_actor.py).
__device__ __forceinline__ float mlp32_tanh(float x) {
  const float ax = fabsf(x), s = x * x;
  float p = fmaf(s, 0.021869488536155202f, -0.05396825396825397f);
  p = fmaf(p, s, 0.13333333333333333f);
  p = fmaf(p, s, -0.33333333333333333f);
  const float small = fmaf(x, p * s, x);
  const float e = __builtin_amdgcn_exp2f(ax * 2.8853900817779268f);
  const float t = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
  return ax < 0.3f ? small : copysignf(t, x);
}

__device__ __forceinline__ void mlp32_mfma4(f32x16_t& acc, const float4& a, const float4& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// One feature tile of a K = 256 layer for both row tiles (two accumulator chains over the 32 k blocks).  TANH_PREV: while these MFMAs run, the tanh of the
// PREVIOUS tile's 32 accumulators is taken, one per k block -- vector instructions of the same wavefront issued between its matrix instructions, so the
// activation function costs no matrix-pipe time (the wavefront's other tile hides half of a layer's tanh; the rest overlaps the second workgroup of the CU)
#define MLP32_PF 2  // weight fragments in flight per wavefront (k blocks ahead of the one being multiplied; deeper rings were measured: no gain, 2.4 x the registers)
struct Mlp32Pre { float4 w[MLP32_PF]; };
__device__ __forceinline__ void mlp32_prefetch(Mlp32Pre& pre, const float4* __restrict__ wa) {
#pragma unroll
  for (int d = 0; d < MLP32_PF; ++d) pre.w[d] = wa[(size_t)d * 64];
}
// (the wavefront's two feature tiles are adjacent in the packed weights: k block j = 0 .. 63 of the pair is wa + 64 j, so the fragments in flight run across the tile boundary)
template <bool TANH_PREV, int J0>
__device__ __forceinline__ void mlp32_tile_k256(const float4* __restrict__ wa, const float4* __restrict__ xb, f32x16_t (&acc)[2], f32x16_t (&prev)[2], Mlp32Pre& pre) {
  float4 a = pre.w[0], n = pre.w[1];
#pragma unroll
  for (int kq = 0; kq < 32; ++kq) {
    const float4 p = wa[(size_t)(J0 + kq + 2 < 64 ? J0 + kq + 2 : 63) * 64];
    const float4 b0 = xb[(size_t)kq * (MLP32_ROWS * 2)], b1 = xb[(size_t)kq * (MLP32_ROWS * 2) + 32];
    mlp32_mfma4(acc[0], a, b0);
    if (TANH_PREV) prev[kq >> 4][kq & 15] = mlp32_tanh(prev[kq >> 4][kq & 15]);
    mlp32_mfma4(acc[1], a, b1);
    a = n; n = p;
  }
  pre.w[0] = a; pre.w[1] = n;
}

// in: [R][in_dim] row-major fp32 (in_dim <= the padded K of layer 0); out: [R][F_last]
#ifdef SIGMAENV_PROFILE
#define MLP32_TS_ARG , unsigned long long* __restrict__ ts, int stagger
#define MLP32_TS_PASS , m->ts, stagger  /* what mlp32_launch passes for MLP32_TS_ARG */
#define MLP32_TS(k) do { if (ts && threadIdx.x == 0) ts[(size_t)blockIdx.x * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define MLP32_TS_ARG
#define MLP32_TS_PASS
#define MLP32_TS(k) do { } while (0)
#endif
// ROWS = false: `in` is dense [R][in_dim], 16-byte aligned (sigmaenv_mlp32_forward, the actor forwards, the rollouts; rw is not read); ROWS = true: the rows of a
// record (Mlp32Rows, sigmaenv_mlp32_forward_rows).  Only the row addresses and loads of stage() differ.  Two instantiations of the KERNEL, not one body inlined
// into two kernels: the dense one then compiles to what it was before the strided one existed (236 VGPRs, no scratch; as an inlined body it took 256 VGPRs and
// 128 bytes of scratch per lane -- tools/kernel_resources.sh)
// SAVE (sigmaenv_mlp32_forward_save, sigmaenv_grad.inc): a third instantiation that also writes every hidden layer's post-tanh tile -- the registers the LDS store
// below takes -- to acts [n_layers - 1][R][256]; the other two never read `acts` and compile to what they were (profiles/learn_kernel_resources.txt).
// INDEXED (sigmaenv_mlp32_forward_save_indexed): a fourth instantiation, <true, true, true>, whose rows are blocks picked by `ix` (Mlp32Index).  The 64 row offsets of the
// tile are formed once, by the first 64 lanes, into the LDS words the output layer's partial sums use much later; stage() reads them from there.  The other three never
// read `ix` and keep their figures (profiles/ppo_kernel_resources.txt).
// PAD (Mlp32Pad): <true, false, false, true> and <true, true, true, true>, the padded forms of the record rows and of the indexed saving forward; the others never read `pd`.
// These six and the three of sigmaenv_mlp32s_kernel are chosen and launched in ONE place, mlp32_launch below, from the call's Mlp32View: every launch passes the view's
// rw / ix / pd and the caller's acts, which are zeros / null wherever an instantiation does not read them.
template <bool ROWS, bool SAVE = false, bool INDEXED = false, bool PAD = false>
__global__ void __launch_bounds__(256, 2) sigmaenv_mlp32_kernel(Mlp32Weights mw, const float* __restrict__ in, int R, int in_dim, float* __restrict__ out, Mlp32Rows rw,
                                                                float* __restrict__ acts, Mlp32Index ix, Mlp32Pad pd MLP32_TS_ARG) {
  sigma_poison_lds();
  MLP32_TS(0);
#ifdef SIGMAENV_PROFILE
  if (stagger > 0 && ((blockIdx.x >> 8) & 1)) {  // diagnostic: the second workgroup of every CU (first dispatch wave) starts `stagger` x 8k cycles late
    for (int q = 0; q < stagger; ++q) __builtin_amdgcn_s_sleep(127);
  }
#endif
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* x = reinterpret_cast<float*>(smem_raw);                        // [256 / 8][2][64][4]: the activations of the current layer (layer 0: a chunk of its inputs)
  float* part = x + (size_t)MLP32_H * MLP32_ROWS;                       // [2][32][32]: partial sums of the output layer's second k half
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * MLP32_ROWS;
  const int K0 = mw.K[0];
#define MLP32_SEL(arr, l) ((l) == 0 ? mw.arr[0] : (l) == 1 ? mw.arr[1] : (l) == 2 ? mw.arr[2] : mw.arr[3])  /* (no runtime-indexed kernel argument: that would live in scratch) */
  // What does not depend on the input rows is requested BEFORE they are staged (one global round trip instead of three in a row at the top of layer 0): the first
  // layer's biases and its first weight fragments
  Mlp32Pre pre;  // the first weight fragments of the NEXT layer's first tile (no dependence on the activations)
#pragma unroll
  for (int d = 0; d < MLP32_PF; ++d) pre.w[d] = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 nb[2][4];  // biases of the next hidden layer for this wavefront's two feature tiles: features 32 (2 wave + ft) + 8 g + 4 h + {0, 1, 2, 3}
  float4 l0w[4];    // layer 0, general path: k blocks 0 and 1 of both feature tiles
  const int KQ0 = mw.K[0] >> 3;
#pragma unroll
  for (int ft = 0; ft < 2; ++ft)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) nb[ft][g4] = reinterpret_cast<const float4*>(mw.b[0] + (2 * wave + ft) * 32 + 8 * g4 + 4 * h)[0];
  if (mw.n_layers > 1 && KQ0 == 32) {  // (an input width of exactly 256: the first layer takes the tile-by-tile path as well)
    const float4* wn = reinterpret_cast<const float4*>(mw.w[0]) + (size_t)(2 * wave) * 32 * 64 + lane;
    mlp32_prefetch(pre, wn);
  } else if (mw.n_layers > 1) {
    const float4* wa0 = reinterpret_cast<const float4*>(mw.w[0]) + (size_t)(2 * wave) * KQ0 * 64 + lane;
    const int k1 = KQ0 > 1 ? 1 : 0;
    l0w[0] = wa0[0]; l0w[1] = wa0[(size_t)KQ0 * 64]; l0w[2] = wa0[(size_t)k1 * 64]; l0w[3] = wa0[(size_t)(KQ0 + k1) * 64];
  }
  const long long* row_off = reinterpret_cast<const long long*>(part);  // INDEXED: [64] float offsets of the tile's rows, -1: a row to stage as zeros
  if constexpr (INDEXED) {
    if (tid < MLP32_ROWS) reinterpret_cast<long long*>(part)[tid] = row0 + tid < R ? mlp32_indexed_row_offset(row0 + tid, rw, ix) : -1ll;
    __syncthreads();
  }
  // input tile, columns [c0, c0 + cw) of layer 0 (cw a multiple of 8, at most MLP32_KC; columns >= in_dim are zeros) at LDS columns [0, cw)
  auto stage = [&](const int c0, const int cw) {
    if constexpr (PAD) {
      for (int e = tid; e < cw * MLP32_ROWS; e += blockDim.x) {            // (coalesced along k within a segment)
        const int n = e / cw, kl = e - n * cw, k = c0 + kl;
        const int row = row0 + n;
        float v = 0.0f;
        if constexpr (INDEXED) {
          const long long off = row_off[n];
          if (off >= 0 && k < in_dim) v = mlp32_pad_load(in + off, k, pd);
        } else if (row < R && k < in_dim) {
          v = mlp32_pad_load(mlp32_row_ptr<true>(in, row, in_dim, rw), k, pd);
        }
        x[mlp32_act_idx(kl, n)] = v;
      }
    } else if ((in_dim & 3) == 0) {  // four columns per lane and load (rows are 16-byte aligned: include/sigmaenv.h)
      const int Q = cw >> 2;
      for (int e = tid; e < Q * MLP32_ROWS; e += blockDim.x) {
        const int n = e / Q, kl = (e - n * Q) << 2, k = c0 + kl;
        const int row = row0 + n;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (INDEXED) {
          const long long off = row_off[n];
          if (off >= 0 && k < in_dim) v = rw.aligned ? reinterpret_cast<const float4*>(in + off + k)[0] : mlp32_ld4_realign(in + off + k);
        } else if (row < R && k < in_dim) {
          if constexpr (ROWS) {
            const float* src = mlp32_row_ptr<true>(in, row, in_dim, rw) + k;
            v = rw.aligned ? reinterpret_cast<const float4*>(src)[0] : mlp32_ld4_realign(src);
          } else {
            v = reinterpret_cast<const float4*>(in + (size_t)row * in_dim)[k >> 2];
          }
        }
        // columns k, k + 2 share a fragment (k parity 0), k + 1, k + 3 the one 64 fragments further (mlp32_act_idx)
        float* d = x + mlp32_act_idx(kl, n);
        *reinterpret_cast<float2*>(d) = make_float2(v.x, v.z);
        *reinterpret_cast<float2*>(d + MLP32_ROWS * 4) = make_float2(v.y, v.w);
      }
    } else {
      for (int e = tid; e < cw * MLP32_ROWS; e += blockDim.x) {            // (coalesced along k within a row)
        const int n = e / cw, kl = e - n * cw, k = c0 + kl;
        const int row = row0 + n;
        if constexpr (INDEXED) {
          const long long off = row_off[n];
          x[mlp32_act_idx(kl, n)] = (off >= 0 && k < in_dim) ? in[off + k] : 0.0f;
        } else {
          x[mlp32_act_idx(kl, n)] = (row < R && k < in_dim) ? mlp32_row_ptr<ROWS>(in, row, in_dim, rw)[k] : 0.0f;
        }
      }
    }
  };
  stage(0, K0 < MLP32_KC ? K0 : MLP32_KC);
  __syncthreads();
  MLP32_TS(1);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (int l = 0; l < mw.n_layers; ++l) {
    const int KQ = MLP32_SEL(K, l) >> 3, Fl = MLP32_SEL(F, l);
    const float4* w4 = reinterpret_cast<const float4*>(MLP32_SEL(w, l));
    if (l + 1 < mw.n_layers) {
      // ---- hidden layer: feature tiles 2 wave, 2 wave + 1 x row tiles 0, 1
      f32x16_t acc[2][2];
      if (l > 0) {  // (layer 0's were requested before the input tile was staged)
        const float* bn = MLP32_SEL(b, l);
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) nb[ft][g4] = reinterpret_cast<const float4*>(bn + (2 * wave + ft) * 32 + 8 * g4 + 4 * h)[0];
      }
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float4 b4 = nb[ft][j >> 2];
          const float bj = (j & 3) == 0 ? b4.x : (j & 3) == 1 ? b4.y : (j & 3) == 2 ? b4.z : b4.w;
          acc[ft][0][j] = bj; acc[ft][1][j] = bj;
        }
      const float4* wa = w4 + (size_t)(2 * wave) * KQ * 64 + lane;       // tile 2 wave; tile 2 wave + 1 is KQ * 64 float4s further
      const float4* xb = x4 + h * MLP32_ROWS + m;                         // row tile 0; row tile 1 is 32 float4s further
      if (KQ == 32) {  // the 256 -> 256 layers: tile by tile, the first tile's tanh inside the second tile's MFMA stream
        // (the first weight fragments were requested before the previous layer's barriers: pre)
        mlp32_tile_k256<false, 0>(wa, xb, acc[0], acc[1], pre);
        mlp32_tile_k256<true, 32>(wa, xb, acc[1], acc[0], pre);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[1][rt][j] = mlp32_tanh(acc[1][rt][j]);
      } else {
      const int k1 = KQ > 1 ? 1 : 0;
      float4 a0, a1, n0, n1;
      if (l == 0) { a0 = l0w[0]; a1 = l0w[1]; n0 = l0w[2]; n1 = l0w[3]; }  // (requested before the input tile was staged)
      else { a0 = wa[0]; a1 = wa[(size_t)KQ * 64]; n0 = wa[(size_t)k1 * 64]; n1 = wa[(size_t)(KQ + k1) * 64]; }
      // (only layer 0 comes here: every later layer has K = 256.)  Its inputs arrive in chunks of MLP32_KC columns; the k order of the four chains is that of one
      // pass over all K (the weight requests run across the chunk boundaries), so the results do not depend on the chunking
      for (int c0 = 0; c0 < KQ; c0 += MLP32_KC / 8) {
        if (c0 > 0) {
          __syncthreads();  // every wavefront is done reading the previous chunk
#ifdef SIGMAENV_POISON
          for (int e = tid; e < MLP32_KC * MLP32_ROWS; e += blockDim.x) x[e] = __uint_as_float(0xFFFFFFFFu);  // (a read of a column the new chunk does not stage is a NaN)
#endif
          stage(c0 * 8, KQ - c0 < MLP32_KC / 8 ? (KQ - c0) * 8 : MLP32_KC);
          __syncthreads();
        }
        const int c1 = KQ - c0 < MLP32_KC / 8 ? KQ : c0 + MLP32_KC / 8;
        for (int kq = c0; kq < c1; ++kq) {
          const int kn = kq + 2 < KQ ? kq + 2 : KQ - 1;                  // weights two k blocks ahead
          const float4 p0 = wa[(size_t)kn * 64], p1 = wa[(size_t)(KQ + kn) * 64];
          const float4 b0 = xb[(size_t)(kq - c0) * (MLP32_ROWS * 2)], b1 = xb[(size_t)(kq - c0) * (MLP32_ROWS * 2) + 32];
          mlp32_mfma4(acc[0][0], a0, b0); mlp32_mfma4(acc[0][1], a0, b1);
          mlp32_mfma4(acc[1][0], a1, b0); mlp32_mfma4(acc[1][1], a1, b1);
          a0 = n0; a1 = n1; n0 = p0; n1 = p1;
        }
      }
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[ft][rt][j] = mlp32_tanh(acc[ft][rt][j]);
      }
      if (l + 2 < mw.n_layers && (MLP32_SEL(K, l + 1) >> 3) == 32) {  // next layer is a 256 -> 256 layer: its weights can already travel
        const float4* wn = reinterpret_cast<const float4*>(MLP32_SEL(w, l + 1)) + (size_t)(2 * wave) * 32 * 64 + lane;
        mlp32_prefetch(pre, wn);
      }
      MLP32_TS(2 + 3 * l);  // (wavefront 0's multiplications and activation functions of layer l are done)
      __syncthreads();  // every wavefront is done reading this layer's inputs
      MLP32_TS(3 + 3 * l);
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // features (2 wave + ft) 32 + 8 q + 4 h + {0, 1, 2, 3} = k block kq2, slots (u, hb) = (2 h + (i >> 1), i & 1)
            const int kq2 = (2 * wave + ft) * 4 + q, row = rt * 32 + m;
            float* d = x + ((((size_t)kq2 * 2) * MLP32_ROWS + row) << 2) + 2 * h;  // k parity 0; parity 1 is 64 fragments further
            *reinterpret_cast<float2*>(d) = make_float2(acc[ft][rt][4 * q + 0], acc[ft][rt][4 * q + 2]);
            *reinterpret_cast<float2*>(d + MLP32_ROWS * 4) = make_float2(acc[ft][rt][4 * q + 1], acc[ft][rt][4 * q + 3]);
            if constexpr (SAVE) {  // the same four features, consecutive in the saved row (64-bit row offsets: 2 M rows x 1 KB)
              if (row0 + row < R)
                *reinterpret_cast<float4*>(acts + ((size_t)l * (size_t)R + (size_t)(row0 + row)) * MLP32_H + (size_t)(kq2 * 8 + 4 * h)) =
                    make_float4(acc[ft][rt][4 * q + 0], acc[ft][rt][4 * q + 1], acc[ft][rt][4 * q + 2], acc[ft][rt][4 * q + 3]);
            }
          }
      __syncthreads();
      MLP32_TS(4 + 3 * l);
    } else {
      // ---- output layer (one feature tile): wavefront w takes row tile w & 1 and k blocks [kh KQ / 2, (kh + 1) KQ / 2), kh = w >> 1
      const int rt = wave & 1, kh = wave >> 1;
      const int k_lo = kh ? KQ / 2 : 0, k_hi = kh ? KQ : KQ / 2;
      f32x16_t acc;
      const float4* xb = x4 + h * MLP32_ROWS + rt * 32 + m;
      const float* bo = MLP32_SEL(b, l);
      if (KQ == 32) {  // (always: hidden widths are 256) all 16 weight fragments of this wavefront's k half are requested together -- one round trip, not 16 in a row
        float4 ow[16], ob[4];
        const float4* wo = w4 + lane + (size_t)k_lo * 64;
#pragma unroll
        for (int d = 0; d < 16; ++d) ow[d] = wo[(size_t)d * 64];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) ob[g4] = reinterpret_cast<const float4*>(bo + 8 * g4 + 4 * h)[0];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float4 b4 = ob[j >> 2];
          acc[j] = kh ? 0.0f : ((j & 3) == 0 ? b4.x : (j & 3) == 1 ? b4.y : (j & 3) == 2 ? b4.z : b4.w);
        }
#pragma unroll
        for (int d = 0; d < 16; ++d) mlp32_mfma4(acc, ow[d], xb[(size_t)(k_lo + d) * (MLP32_ROWS * 2)]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = kh ? 0.0f : bo[(j & 3) + 8 * (j >> 2) + 4 * h];
        const float4* wa = w4 + lane;
        for (int kq = k_lo; kq < k_hi; ++kq) mlp32_mfma4(acc, wa[(size_t)kq * 64], xb[(size_t)kq * (MLP32_ROWS * 2)]);
      }
      if (kh) {
#pragma unroll
        for (int j = 0; j < 16; ++j) part[(rt * 16 + j) * 64 + lane] = acc[j];
      }
      MLP32_TS(12);
      __syncthreads();
      if (!kh) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int f = (j & 3) + 8 * (j >> 2) + 4 * h, row = row0 + rt * 32 + m;
          if (f < Fl && row < R) out[(size_t)row * Fl + f] = acc[j] + part[(rt * 16 + j) * 64 + lane];
        }
      }
      MLP32_TS(13);
#ifdef SIGMAENV_PROFILE
      if (ts && threadIdx.x == 0) {  // where the workgroup ran: HW_ID (wave / SIMD / CU / SH / SE fields) and the XCC id
        ts[(size_t)blockIdx.x * 16 + 14] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        ts[(size_t)blockIdx.x * 16 + 15] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);
      }
#endif
    }
  }
#undef MLP32_SEL
}

#include "sigmaenv_mlp32s.inc"  // the same networks on the fp16 matrix rate (every fp32 operand as hi + lo): mode SIGMAENV_MLP32_SPLIT

// the distribution head of the actor on the 4 outputs per row of the exact MLP (same function as the bf16 kernel's epilogue); row_map as Mlp32sHead::row_map
__global__ void sigmaenv_actor_head_kernel(const float* __restrict__ out4, int R, int n_agents, int env_base, float low0, float low1, float high0, float high1, float* __restrict__ actions,
                                           float* __restrict__ log_prob, float* __restrict__ loc_scale, uint64_t seed, uint64_t counter, int deterministic,
                                           const int32_t* __restrict__ row_map) {
  sigma_poison_lds();
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= R) return;
  const int orow = row_map ? row_map[row] : row;
  if (orow < 0) return;
  const float4 o = reinterpret_cast<const float4*>(out4)[row];
  const float low[2] = {low0, low1}, high[2] = {high0, high1};
  actor_distribution(low, high, orow, n_agents, env_base, o.x, o.y, o.z, o.w, actions, log_prob, loc_scale, seed, counter, deterministic);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct sigmaenv_mlp32 {
  Mlp32Weights w{};
  Mlp32sWeights ws{};   // the split-fp16 form of the same network (sigmaenv_mlp32s.inc)
  float* wt[MLP32_MAX_LAYERS] = {};  // the exact form of the TRANSPOSED weights of layers 1 .. n_layers - 1, for the backward pass (sigmaenv_grad.inc); layer 0's only in a
                                     // handle made by sigmaenv_mlp32_create_input_grad (else nullptr): kept current by every path that rewrites weights
  int mode = SIGMAENV_MLP32_SPLIT;       // the mode in force
  int requested = SIGMAENV_MLP32_SPLIT;  // the mode asked for (sigmaenv_mlp32_set_mode): in force again when sigmaenv_mlp32_load_device brings the weights back into range
  bool split_ok = true;    // the split form may run: every weight inside its range and split_fits
  bool split_fits = true;  // the split kernel's LDS takes the input width (dims[0] <= 592)
  int dims[MLP32_MAX_LAYERS + 1] = {};
  uint32_t* range_word = nullptr;  // device word of sigmaenv_mlp32_load_device's range reduction
  size_t smem_s = 0;
  std::vector<void*> allocs;
  int in_dim = 0, out_dim = 0;
  size_t smem = 0;
  unsigned long long* ts = nullptr;  // profile build: [workgroups][16] shader-clock stamps of the last forward
  int ts_groups = 0;
};

extern "C" void sigmaenv_mlp32_destroy(sigmaenv_mlp32* m) {
  if (!m) return;
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
}

// n_layers torch.nn.Linear layers (weights[l]: [dims[l + 1], dims[l]] row-major fp32, biases[l]: [dims[l + 1]]), Tanh between them; hidden widths
// must be 256, dims[n_layers] <= 32.  input_grad: the handle also holds layer 0's transposed form (sigmaenv_mlp32_create_input_grad).
static int mlp32_create_impl(int32_t n_layers, const int32_t* dims, const float* const* weights, const float* const* biases, bool input_grad, sigmaenv_mlp32** out) {
  if (!out || !dims || !weights || !biases || n_layers < 2 || n_layers > MLP32_MAX_LAYERS) return SIGMAENV_EINVAL;
  for (int l = 1; l < n_layers; ++l) if (dims[l] != MLP32_H) return SIGMAENV_EINVAL;
  if (dims[0] < 1 || dims[0] > 4096 || dims[n_layers] < 1 || dims[n_layers] > 32) return SIGMAENV_EINVAL;
  auto* m = new sigmaenv_mlp32();
  m->in_dim = dims[0];
  m->out_dim = dims[n_layers];
  m->w.n_layers = n_layers;
  for (int l = 0; l <= n_layers; ++l) m->dims[l] = dims[l];
  if (hipMalloc((void**)&m->range_word, 4) != hipSuccess) { sigmaenv_mlp32_destroy(m); return SIGMAENV_ENOMEM; }
  m->allocs.push_back(m->range_word);
  m->ws.n_layers = n_layers;
  m->smem = ((size_t)MLP32_H * MLP32_ROWS + 2 * 32 * 32) * sizeof(float);  // 72 KB for every input width (layer 0's inputs are staged MLP32_KC columns at a time)
  // whether the split kernel's LDS takes the input width depends on dims[0] alone: known before the layers are packed
  const int KB0 = load_split_kb(dims[0]);
  m->smem_s = (size_t)(KB0 > 16 ? KB0 : 16) * 256 * 16 + (2 * 16 * 64 + (MLP32_MAX_LAYERS - 1) * MLP32_H + 32) * sizeof(float);
  m->split_fits = m->smem_s <= 160 * 1024;
  // Every form of every layer: the per-slot functions of sigmaenv_pack.h over every lane index, on the host (sigmaenv_mlp32_load_device: the same functions on the
  // device).  The split form is (hi, lo) fp16 fragments of the weights times 2^8 and biases times the accumulator scale of their layer; its buffers exist for a
  // network outside the range as well (never read while split_ok is false: sigmaenv_mlp32_load_device may bring it into range), and with their full size for a
  // network that is exact-only by its width, which neither create nor load packs: they hold zeros, and are never read.
  bool out_of_range = false;
  for (int l = 0; l < n_layers; ++l) {
    Mlp32Layer a = pack_mlp32_layer(dims, l, n_layers, m->split_fits);
    std::vector<float> ew(a.n_exact), eb(a.fp_exact), sb(load_split_biases(a.output_layer != 0), 0.0f), tw(l > 0 || input_grad ? load_exact_t_slots(a.F, a.K) : 0);
    std::vector<uint16_t> sw((size_t)2 * load_split_pairs(a.F, a.K, a.output_layer != 0), 0);
    a.w = weights[l]; a.b = biases[l];
    a.ew = ew.data(); a.eb = eb.data(); a.sw = sw.data(); a.sb = sb.data();
    for (int i = 0, n = pack_mlp32_lanes(a); i < n; ++i) out_of_range |= pack_mlp32_slot(a, i);
    for (int i = 0; i < (int)tw.size(); ++i) pack_mlp32_t_slot(weights[l], tw.data(), a.F, a.K, i);  // the backward pass's form (sigmaenv_grad.inc): layers 1 .. n_layers - 1, layer 0 on request
    int rc = pack_upload(m->allocs, ew.data(), ew.size() * 4, (const void**)&m->w.w[l]);
    if (!rc) rc = pack_upload(m->allocs, eb.data(), eb.size() * 4, (const void**)&m->w.b[l]);
    if (!rc) rc = pack_upload(m->allocs, sw.data(), sw.size() * 2, (const void**)&m->ws.w[l]);
    if (!rc) rc = pack_upload(m->allocs, sb.data(), sb.size() * 4, (const void**)&m->ws.b[l]);
    if (!rc && !tw.empty()) rc = pack_upload(m->allocs, tw.data(), tw.size() * 4, (const void**)&m->wt[l]);
    if (rc) { sigmaenv_mlp32_destroy(m); return rc; }
    m->w.K[l] = load_exact_kp(a.K); m->w.F[l] = a.F; m->w.Fp[l] = a.fp_exact;
    m->ws.KB[l] = load_split_kb(a.K); m->ws.F[l] = a.F;
  }
  m->split_ok = m->split_fits && !out_of_range;
  if (!m->split_ok) m->mode = SIGMAENV_MLP32_EXACT;
  const uint32_t word = out_of_range ? 1u : 0u;  // (what a load of these weights would have reduced: sigmaenv_mlp32_resolve_mode may read it)
  if (hipMemcpy(m->range_word, &word, 4, hipMemcpyHostToDevice) != hipSuccess) { sigmaenv_mlp32_destroy(m); return SIGMAENV_EHIP; }
  *out = m;
  return SIGMAENV_OK;
}
extern "C" int sigmaenv_mlp32_create(int32_t n_layers, const int32_t* dims, const float* const* weights, const float* const* biases, sigmaenv_mlp32** out) {
  return mlp32_create_impl(n_layers, dims, weights, biases, false, out);
}
extern "C" int sigmaenv_mlp32_create_input_grad(int32_t n_layers, const int32_t* dims, const float* const* weights, const float* const* biases, sigmaenv_mlp32** out) {
  return mlp32_create_impl(n_layers, dims, weights, biases, true, out);
}

// SIGMAENV_MLP32_EXACT / SIGMAENV_MLP32_SPLIT (include/sigmaenv.h); a network with a weight outside the split form's range stays exact
extern "C" int sigmaenv_mlp32_set_mode(sigmaenv_mlp32* m, int32_t mode) {
  if (!m || (mode != SIGMAENV_MLP32_EXACT && mode != SIGMAENV_MLP32_SPLIT)) return SIGMAENV_EINVAL;
  if (mode == SIGMAENV_MLP32_SPLIT && !m->split_ok) {
    if (m->split_fits) m->requested = mode;  // (refused for the weights the handle holds: in force with the next sigmaenv_mlp32_load_device inside the range)
    return SIGMAENV_EINVAL;
  }
  m->mode = m->requested = mode;
  return SIGMAENV_OK;
}
extern "C" int sigmaenv_mlp32_get_mode(const sigmaenv_mlp32* m) { return m ? m->mode : SIGMAENV_EINVAL; }

// The rows of a record, from an entry point's raw arguments: row r = t * rows_per_block + b at in + t * block_stride + b * row_stride (floats), 4-byte alignment
// suffices.  index / n_index (nullptr, 0: none): block t of the rows is block index[t] of the record's n_blocks, the minibatch takes the place of the record's blocks
// in the row count.  pad (nullptr: none): the row in memory holds in_dim / dst segments of src floats.  Every refusal is made here, before any launch, with a message
// that starts with `what`; no row is not an error, and then `in` is not looked at.
static int mlp32_view(sigmaenv_t* h, const sigmaenv_mlp32* m, const char* what, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                      const int32_t* index, int32_t n_index, const Mlp32Pad* pad, Mlp32View* v) {
  *v = Mlp32View{};
  v->what = what;
  v->in = in;
  v->by_rows = true;
  if (index || n_index) {
    if (n_blocks < 0 || n_index < 0 || block_stride < 0) { h->err = std::string(what) + ": negative n_blocks, index length or block_stride"; return SIGMAENV_EINVAL; }
    if (n_index > 0 && (!index || ((uintptr_t)index & 3))) { h->err = std::string(what) + ": a null index or one that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
    v->indexed = true;  // (index is not null here)
    v->ix.index = index;
    v->ix.n_blocks = n_blocks;
  }
  const int32_t blocks = v->indexed ? n_index : n_blocks;
  if (rows_per_block < 0 || blocks < 0 || (int64_t)rows_per_block * blocks > INT32_MAX) { h->err = std::string(what) + ": negative counts or more than 2^31 - 1 rows"; return SIGMAENV_EINVAL; }
  if (pad) {
    if (pad->src < 1 || pad->dst < pad->src || m->in_dim % pad->dst) { h->err = std::string(what) + ": 1 <= seg_src <= seg_dst, and seg_dst divides the network's input width"; return SIGMAENV_EINVAL; }
    v->padded = true;
    v->pd = *pad;
  }
  v->rows = rows_per_block * blocks;
  if (v->rows == 0) return SIGMAENV_OK;
  const int64_t width = pad ? (int64_t)(m->in_dim / pad->dst) * pad->src : m->in_dim;  // the row in memory
  if (!in || ((uintptr_t)in & 3) || row_stride < width || (blocks > 1 && block_stride < 0)) {
    h->err = std::string(what) + ": a null input or one that is not 4-byte aligned, row_stride below the row's width in memory or a negative block_stride";
    return SIGMAENV_EINVAL;
  }
  v->rw.rpb = rows_per_block;
  v->rw.row_stride = row_stride;
  v->rw.block_stride = block_stride;
  // (16-byte loads as in the dense kernels; the padded instantiations stage column by column and do not read it)
  v->rw.aligned = !pad && ((uintptr_t)in & 15) == 0 && (row_stride & 3) == 0 && (block_stride & 3) == 0;
  return SIGMAENV_OK;
}

enum {  // the forward's instantiations: a row of the LDS table below each
  MLP32_K_DENSE, MLP32_K_ROWS, MLP32_K_ROWS_PAD, MLP32_K_SAVE, MLP32_K_SAVE_INDEXED, MLP32_K_SAVE_INDEXED_PAD,  // sigmaenv_mlp32_kernel
  MLP32_KS_DENSE, MLP32_KS_ROWS, MLP32_KS_ROWS_PAD,                                                             // sigmaenv_mlp32s_kernel
  MLP32_N_KERNELS
};
// The dynamic-LDS limit is a per-kernel attribute -- PER DEVICE (ADVICE r5: a second GPU driven from the same process never got the opt-in beyond 64 KB): raised
// when a call needs more than what was set for this kernel on this device before (not once per forward; models of different input widths coexist); atomics:
// handles may be driven from several threads
static int mlp32_lds_limit(sigmaenv_t* h, int kernel, const void* kfn, size_t smem) {
  static std::atomic<size_t> s_lds_set[MLP32_N_KERNELS][64];
  std::atomic<size_t>& lds_set = s_lds_set[kernel][h->device >= 0 && h->device < 64 ? h->device : 0];
  if (smem > 64 * 1024 && smem > lds_set.load(std::memory_order_acquire)) {
    HIPCHK(h, hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    size_t cur = lds_set.load(std::memory_order_relaxed);
    while (cur < smem && !lds_set.compare_exchange_weak(cur, smem, std::memory_order_release)) {}
  }
  return SIGMAENV_OK;
}

// The network on the rows of `v`, enqueued on the handle's stream: out [rows, out_dim]; acts: the saving forward (sigmaenv_grad.inc), else nullptr.  The ONE place that
// decides the arithmetic and the instantiation, raises its LDS limit and launches it.
// head: the actor's distribution head, run as the epilogue of the non-padded split kernels (*head_done = true) -- every other kernel leaves it to the caller's head launch
static int mlp32_launch(sigmaenv_t* h, sigmaenv_mlp32* m, const Mlp32View& v, float* out, float* acts, const Mlp32sHead* head, bool* head_done) {
  if (head_done) *head_done = false;
  if (v.rows == 0) return SIGMAENV_OK;
  const bool save = acts != nullptr;
  const bool split = !save && m->mode == SIGMAENV_MLP32_SPLIT;  // (the saving forward is the exact chain whatever mode the network runs in)
  int k;  // a view that no instantiation serves: -1
  if (save) k = !v.by_rows || (v.padded && !v.indexed) ? -1 : v.padded ? MLP32_K_SAVE_INDEXED_PAD : v.indexed ? MLP32_K_SAVE_INDEXED : MLP32_K_SAVE;
  else if (v.indexed) k = -1;
  else if (split) k = v.padded ? MLP32_KS_ROWS_PAD : v.by_rows ? MLP32_KS_ROWS : MLP32_KS_DENSE;
  else k = v.padded ? MLP32_K_ROWS_PAD : v.by_rows ? MLP32_K_ROWS : MLP32_K_DENSE;
  if (k < 0) {
    h->err = std::string(v.what) + (v.indexed ? ": indexed rows are built for the saving forward" : v.padded ? ": padded rows are built for the indexed forward" : ": the saving forward reads record rows");
    return SIGMAENV_EINVAL;
  }
  Mlp32sHead hd{};
  if (head && split && !v.padded && m->out_dim == 4) { hd = *head; hd.on = 1; if (head_done) *head_done = true; }
  HIPCHK(h, hipSetDevice(h->device));
  size_t smem = split ? m->smem_s : m->smem;
  const dim3 grid((v.rows + MLP32_ROWS - 1) / MLP32_ROWS);
#ifdef SIGMAENV_PROFILE
  if (getenv("SIGMAENV_TIMESTAMPS") && m->ts_groups < (int)grid.x) {
    if (m->ts) (void)hipFree(m->ts);
    m->ts = nullptr;
    if (hipMalloc((void**)&m->ts, (size_t)grid.x * 16 * 8) == hipSuccess) { m->ts_groups = (int)grid.x; (void)hipMemsetAsync(m->ts, 0, (size_t)grid.x * 16 * 8, h->stream); }
  }
  if (getenv("SIGMAENV_MLP32_ONE_WG") && smem < 100 * 1024) smem = 100 * 1024;  // diagnostic: one workgroup per CU (more LDS than two can share)
  const int stagger = getenv("SIGMAENV_MLP32_STAGGER") ? atoi(getenv("SIGMAENV_MLP32_STAGGER")) : 0;
#endif
  int slot = -1;  // the SIGMAENV_KERNEL_MLP32 timer brackets the non-saving forwards
#define MLP32_LAUNCH(kernel, id, ...)                                                                     \
  case id:                                                                                                \
    if (const int rc = mlp32_lds_limit(h, id, reinterpret_cast<const void*>(kernel), smem)) return rc;    \
    if (!save) slot = timer_begin(h, SIGMAENV_KERNEL_MLP32);                                              \
    hipLaunchKernelGGL(kernel, grid, dim3(256), smem, h->stream, __VA_ARGS__ MLP32_TS_PASS);              \
    break;
#define MLP32_EXACT(kernel, id) MLP32_LAUNCH(kernel, id, m->w, v.in, v.rows, m->in_dim, out, v.rw, acts, v.ix, v.pd)
#define MLP32_SPLIT(kernel, id) MLP32_LAUNCH(kernel, id, m->ws, v.in, v.rows, m->in_dim, out, hd, v.rw, v.pd)
  switch (k) {  // (the cases' order is the kernels' order in the code object: kept, so that tools/kernel_isa_diff.sh compares a build with an older one kernel by kernel)
    MLP32_SPLIT((sigmaenv_mlp32s_kernel<true, true>), MLP32_KS_ROWS_PAD)
    MLP32_EXACT((sigmaenv_mlp32_kernel<true, false, false, true>), MLP32_K_ROWS_PAD)
    MLP32_SPLIT((sigmaenv_mlp32s_kernel<true>), MLP32_KS_ROWS)
    MLP32_SPLIT((sigmaenv_mlp32s_kernel<false>), MLP32_KS_DENSE)
    MLP32_EXACT((sigmaenv_mlp32_kernel<true>), MLP32_K_ROWS)
    MLP32_EXACT((sigmaenv_mlp32_kernel<false>), MLP32_K_DENSE)
    MLP32_EXACT((sigmaenv_mlp32_kernel<true, true, true, true>), MLP32_K_SAVE_INDEXED_PAD)
    MLP32_EXACT((sigmaenv_mlp32_kernel<true, true, true>), MLP32_K_SAVE_INDEXED)
    MLP32_EXACT((sigmaenv_mlp32_kernel<true, true>), MLP32_K_SAVE)
  }
#undef MLP32_SPLIT
#undef MLP32_EXACT
#undef MLP32_LAUNCH
  HIPCHK(h, hipGetLastError());
  timer_end(h, SIGMAENV_KERNEL_MLP32, slot);
  return SIGMAENV_OK;
}

// out[rows, out_dim] := mlp(in[rows, in_dim]) in fp32 (device pointers, `in` dense and 16-byte aligned)
static int mlp32_forward_impl(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows, float* out, const Mlp32sHead* head, bool* head_done) {
  if (head_done) *head_done = false;
  if (!h || !m || !in || !out || rows < 0) return SIGMAENV_EINVAL;
  Mlp32View v{};
  v.what = "mlp32_forward";
  v.in = in;
  v.rows = rows;
  return mlp32_launch(h, m, v, out, nullptr, head, head_done);
}
extern "C" int sigmaenv_mlp32_forward(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows, float* out) { return mlp32_forward_impl(h, m, in, rows, out, nullptr, nullptr); }
// The network on rows that are not dense (mlp32_view); out is dense.  The staging of the input tile is the only difference to sigmaenv_mlp32_forward: same bits per
// row in both modes.
extern "C" int sigmaenv_mlp32_forward_rows(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                           float* out) {
  if (!h || !m || !in || !out || rows_per_block < 0 || n_blocks < 0) return SIGMAENV_EINVAL;  // (this entry point's own: before anything else, without a message, whatever the row count)
  Mlp32View v;
  if (const int rc = mlp32_view(h, m, "mlp32_forward_rows", in, rows_per_block, row_stride, n_blocks, block_stride, nullptr, 0, nullptr, &v)) return rc;
  return mlp32_launch(h, m, v, out, nullptr, nullptr, nullptr);
}
// sigmaenv_mlp32_forward_rows on padded rows (Mlp32Pad): the row in memory holds in_dim / seg_dst segments of seg_src floats.  Both modes; no distribution head.
extern "C" int sigmaenv_mlp32_forward_rows_pad(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int32_t rows_per_block, int64_t row_stride, int32_t n_blocks, int64_t block_stride,
                                               int32_t seg_src, int32_t seg_dst, float* out) {
  if (!h || !m || !in || !out || rows_per_block < 0 || n_blocks < 0) return SIGMAENV_EINVAL;  // (as sigmaenv_mlp32_forward_rows)
  const Mlp32Pad pd{seg_src, seg_dst};
  Mlp32View v;
  if (const int rc = mlp32_view(h, m, "mlp32_forward_rows_pad", in, rows_per_block, row_stride, n_blocks, block_stride, nullptr, 0, &pd, &v)) return rc;
  return mlp32_launch(h, m, v, out, nullptr, nullptr, nullptr);
}

// The actor in the reference's precision: exact-fp32 MLP (obs_dim -> 256 -> 256 -> 256 -> 4) + the distribution head.  Same outputs as
// sigmaenv_actor_forward; `scratch`: device f32 [B * N * 4].
// R network rows `in` [R, in_dim] -> the actor's outputs of agent rows row_map[r] (nullptr: R = B * N, identity); scratch: device f32 [R * 4]
static int actor_rows_f32(sigmaenv_t* h, sigmaenv_mlp32* m, const float* in, int R, const int32_t* row_map, float* scratch, const float* low, const float* high, float* actions,
                          float* log_prob, float* loc_scale, uint64_t seed, uint64_t counter, int32_t deterministic) {
  Mlp32sHead hd{};
  hd.n_agents = h->N; hd.env_base = h->cfg.env_index_base; hd.deterministic = (int)deterministic;
  hd.low0 = low[0]; hd.low1 = low[1]; hd.high0 = high[0]; hd.high1 = high[1];
  hd.actions = actions; hd.log_prob = log_prob; hd.loc_scale = loc_scale; hd.seed = seed; hd.counter = counter; hd.row_map = row_map;
  bool head_done = false;
  int rc = mlp32_forward_impl(h, m, in, R, scratch, &hd, &head_done);
  if (rc) return rc;
  if (head_done) return SIGMAENV_OK;  // (split mode: the head ran as the network kernel's epilogue)
  hipLaunchKernelGGL(sigmaenv_actor_head_kernel, dim3((R + 255) / 256), dim3(256), 0, h->stream, scratch, R, h->N, h->cfg.env_index_base, low[0], low[1], high[0], high[1], actions, log_prob,
                     loc_scale, seed, counter, (int)deterministic, row_map);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_actor_forward_f32(sigmaenv_t* h, sigmaenv_mlp32* m, const float* obs, float* scratch, const float* low, const float* high, float* actions,
                                          float* log_prob, float* loc_scale, uint64_t seed, uint64_t counter, int32_t deterministic) {
  if (!h || !m || !scratch || !actions || !low || !high || m->out_dim != 4 || (!obs && m->in_dim != h->D)) return SIGMAENV_EINVAL;
  return actor_rows_f32(h, m, obs ? obs : h->buf.obs, h->B * h->N, nullptr, scratch, low, high, actions, log_prob, loc_scale, seed, counter, deterministic);
}

// sigmaenv_rollout in the reference's precision (decision_making_module.py:34-82: an fp32 torch MLP): n_steps x (exact-fp32 actor forward + distribution
// head -> [CBF launch] -> fused step + record + resets), enqueued back to back without returning to the caller.  The plain policy only: the
// opponent-modelling and prioritized wrappers of the collector run through sigmaenv_rollout_f32_ex (sigmaenv_wrappers.inc).  Step t is exactly
// sigmaenv_actor_forward_f32(..., seed, counter0 + t, ...) followed by sigmaenv_step_autoreset(..., seed, counter0 + t, ...) with the record row t.
// scratch: device f32 [B * N * 4]; the other arguments as sigmaenv_rollout.
extern "C" int sigmaenv_rollout_f32(sigmaenv_t* h, sigmaenv_mlp32* m, const float* low, const float* high, float* scratch, int32_t n_steps, float* actions_buf,
                                    float* slab_base, float* logp_base, float* actions_rec, uint64_t seed, uint64_t counter0, int32_t path_first, int32_t path_count,
                                    int32_t deterministic) {
  if (!h || !m || !low || !high || !scratch) return SIGMAENV_EINVAL;
  return rollout_loop(h, [&](int t, float* act, float* logp) {
    return sigmaenv_actor_forward_f32(h, m, nullptr, scratch, low, high, act, logp, nullptr, seed, counter0 + (uint64_t)t, deterministic);
  }, n_steps, actions_buf, slab_base, logp_base, actions_rec, seed, counter0, path_first, path_count);
}

#ifdef SIGMAENV_PROFILE
// profile build only: the stamps of the last forward ([workgroups][16] u64); returns the number of workgroups
extern "C" int sigmaenv_mlp32_debug_timestamps(sigmaenv_mlp32* m, unsigned long long* out, int32_t max_groups) {
  if (!m || !out || !m->ts) return 0;
  const int n = m->ts_groups < max_groups ? m->ts_groups : max_groups;
  if (hipDeviceSynchronize() != hipSuccess) return 0;
  if (hipMemcpy(out, m->ts, (size_t)n * 16 * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}
#endif
