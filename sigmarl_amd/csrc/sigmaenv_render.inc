// sigmaenv_render.inc -- top-down frames of selected envs on the device: map, short-term paths and vehicles as uint8 RGB (included by sigmaenv.hip after
// sigmaenv_render.h, which states the picture; the contract is in include/sigmaenv.h, sigmaenv_render_*).
//
// What it restates: the drawing LIST of sigmarl/scenarios/road_traffic.py:1637-1800 (extra_render) and of the vehicle shapes (:560-600), not its pyglet scene graph.
//
// Background kernel (once, at create): one workgroup per tile of RND_TILE_W x RND_TILE_H pixels walks every boundary segment of the map table in chunks of 256 staged
// in LDS in pixel coordinates, a lane ORs the coverage bits of its four pixels, writes the coverage words and the resolved colours.  Not the hot path.
// Frame kernel (one launch per frame, grid = strips of RND_STRIP tiles x selected envs): the workgroup stages the env's P primitives in LDS in pixel coordinates with their boxes
// (rnd_env_prim), compacts the ones whose box meets the tile into the tile's ordered list with a ballot per wavefront and the four wavefronts' counts through LDS,
// and then either copies the background's resolved colours (empty list: 16-byte loads and stores where W is a multiple of 16, dwords otherwise) or shades: a lane
// owns four horizontally adjacent pixels, runs rnd_pixel on each and writes their 12 bytes as three dword stores.  A list beyond RND_LIST_CAP: the tile walks all P
// primitives.  No atomics, no host wait; every launch is on the handle's stream.  All LDS is dynamic and carved at multiples of 16 bytes.

namespace render {

static_assert(RND_FLAG_SHORT_TERM == SIGMAENV_RENDER_SHORT_TERM, "the header's flag and the C-ABI's are one");

struct FrameArgs {
  rnd_view_t view;
  int W, H, N, flags, P, tiles_x, vec16;
  float h_p, r_disc;
  const uint16_t* mask;   // [H, W] coverage of the boundaries
  const uint8_t* bg_rgb;  // [H, W, 3] the map alone
  const uint8_t* pal;     // [4 + N, 3]
  const int32_t* sel;     // [n_sel]
  const float *vertices, *short_term, *state;
  const uint8_t *col_agents, *col_flags;
  uint8_t* out;           // [n_sel, H, W, 3]
};

__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t frame_lds(int P, int N) { return align16((size_t)P * sizeof(rnd_prim_t)) + align16(RND_LIST_CAP * sizeof(uint16_t)) + align16((size_t)(4 + N) * 3) + 16; }

// the lane's four pixels (r, c .. c + 3), 12 bytes, as three dwords at rgb + (r W + c) 3: a multiple of 12 bytes from a 4-byte aligned base
__device__ __forceinline__ void store_px4(uint8_t* rgb, int W, int r, int c, const uint32_t* w) {
  uint32_t* o = reinterpret_cast<uint32_t*>(rgb + ((size_t)r * W + c) * 3);
  o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
}

// pixel p (0 .. 3) of the lane's four: rnd_pixel, then its three bytes into the lane's three dwords (p is a constant or uniform: the selects below are scalar)
template <int S>
__device__ __forceinline__ void shade_px(const rnd_prim_t* prims, const uint16_t* list, int n, int r, int c, int p, uint2 mw, const uint8_t* pal, uint32_t* w) {
  const uint32_t word = p < 2 ? mw.x : mw.y;
  uint8_t o[3];
  rnd_pixel(prims, list, n, r, c + p, S, (p & 1) ? word >> 16 : word & 0xffffu, pal, o);
  const uint32_t v = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
  if (p == 0) w[0] = v;
  else if (p == 1) { w[0] |= v << 24; w[1] = v >> 8; }
  else if (p == 2) { w[1] |= v << 16; w[2] = v >> 16; }
  else w[2] |= v << 8;
}

// vertically adjacent tiles ONE workgroup walks after staging the env's primitives once: the staging (P primitives from five buffers) costs more than an empty tile's
// copy, and most tiles are empty; 512 x 512 x 64 envs are still 4096 workgroups
#define RND_STRIP 4

template <int S>
__global__ void __launch_bounds__(RND_BLOCK) sigmaenv_render_frame_kernel(FrameArgs a) {
  sigma_poison_lds();
  extern __shared__ __attribute__((aligned(16))) unsigned char rnd_smem[];
  rnd_prim_t* prims = reinterpret_cast<rnd_prim_t*>(rnd_smem);
  uint16_t* list = reinterpret_cast<uint16_t*>(rnd_smem + align16((size_t)a.P * sizeof(rnd_prim_t)));
  uint8_t* pal = reinterpret_cast<uint8_t*>(list) + align16(RND_LIST_CAP * sizeof(uint16_t));
  int* cnt = reinterpret_cast<int*>(pal + align16((size_t)(4 + a.N) * 3));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, W = a.W, H = a.H;
  const size_t b = (size_t)a.sel[blockIdx.y];  // checked against [0, B) at create
  const int strip = blockIdx.x / a.tiles_x, tx = blockIdx.x - strip * a.tiles_x;
  const int tiles_y = (H + RND_TILE_H - 1) / RND_TILE_H;
  const int tc0 = tx * RND_TILE_W, tc1 = min(tc0 + RND_TILE_W, W) - 1;
  for (int k = tid; k < a.P; k += RND_BLOCK)
    rnd_env_prim(k, N, NS, a.flags, a.view, W, H, a.h_p, a.r_disc, a.vertices + b * N * 10, a.short_term + b * N * NS * 2, a.state + b * N * 8, a.col_agents + b * N * N,
                 a.col_flags + b * N * 4, prims + k);
  for (int k = tid; k < (4 + N) * 3; k += RND_BLOCK) pal[k] = a.pal[k];
  __syncthreads();
  uint8_t* out = a.out + (size_t)blockIdx.y * H * W * 3;
  for (int ty = strip * RND_STRIP; ty < min((strip + 1) * RND_STRIP, tiles_y); ++ty) {  // (the same trip count for every lane: the barriers below are met by all)
    const int tr0 = ty * RND_TILE_H, tr1 = min(tr0 + RND_TILE_H, H) - 1;
    // the tile's list: the primitives whose box meets the tile, in their order.  (The first barrier of a tile is also what ends the previous tile's reads of the list.)
    int n = 0;
    for (int k0 = 0; k0 < a.P; k0 += RND_BLOCK) {
      const int k = k0 + tid;
      const bool hit = k < a.P && rnd_box_hits(prims + k, tc0, tc1, tr0, tr1);
      const unsigned long long bal = __ballot(hit);
      if (lane == 0) cnt[wave] = __popcll(bal);
      __syncthreads();
      int before = n;
      for (int w = 0; w < wave; ++w) before += cnt[w];
      if (hit) {
        const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
        if (pos < RND_LIST_CAP) list[pos] = (uint16_t)k;
      }
      n += cnt[0] + cnt[1] + cnt[2] + cnt[3];
      __syncthreads();
    }
    if (n == 0) {  // the background's colours, nothing per sample
      const int row_bytes = (tc1 - tc0 + 1) * 3, rows = tr1 - tr0 + 1;
      if (a.vec16) {
        const int per = row_bytes >> 4;
        for (int k = tid; k < rows * per; k += RND_BLOCK) {
          const int rr = k / per, q = k - rr * per;
          const size_t off = ((size_t)(tr0 + rr) * W + tc0) * 3 + (size_t)q * 16;
          *reinterpret_cast<uint4*>(out + off) = *reinterpret_cast<const uint4*>(a.bg_rgb + off);
        }
      } else {
        const int per = row_bytes >> 2;
        for (int k = tid; k < rows * per; k += RND_BLOCK) {
          const int rr = k / per, q = k - rr * per;
          const size_t off = ((size_t)(tr0 + rr) * W + tc0) * 3 + (size_t)q * 4;
          *reinterpret_cast<uint32_t*>(out + off) = *reinterpret_cast<const uint32_t*>(a.bg_rgb + off);
        }
      }
      continue;
    }
    const int r = tr0 + (tid >> 4), c = tc0 + RND_LANE_PX * (tid & 15);
    if (r <= tr1 && c <= tc1) {  // (W is a multiple of 4: c <= tc1 means c + 3 <= tc1)
      const uint2 mw = *reinterpret_cast<const uint2*>(a.mask + (size_t)r * W + c);  // four u16, 8-byte aligned
      const bool all = n > RND_LIST_CAP;
      uint32_t w[3] = {0u, 0u, 0u};  // the four pixels' 12 bytes
      const uint16_t* ls = all ? (const uint16_t*)nullptr : list;
      const int nl = all ? a.P : n;
      if (S <= 2) {  // the four pixels side by side: their chains are independent
#pragma unroll
        for (int p = 0; p < RND_LANE_PX; ++p) shade_px<S>(prims, ls, nl, r, c, p, mw, pal, w);
      } else {       // S = 4: one pixel at a time, so that the 16 sample indices of ONE pixel are in registers (180 VGPRs unrolled, 75 so)
#pragma unroll 1
        for (int p = 0; p < RND_LANE_PX; ++p) shade_px<S>(prims, ls, nl, r, c, p, mw, pal, w);
      }
      store_px4(out, W, r, c, w);
    }
  }
}

struct BackgroundArgs {
  rnd_view_t view;
  int W, H, tiles_x, n_paths, stride;
  float h_b;
  const float *left, *right;
  const int32_t *n_left, *n_right;
  const uint8_t* pal;
  uint16_t* mask;
  uint8_t* bg_rgb;
};

template <int S>
__global__ void __launch_bounds__(RND_BLOCK) sigmaenv_render_background_kernel(BackgroundArgs a) {
  sigma_poison_lds();
  extern __shared__ __attribute__((aligned(16))) unsigned char rnd_smem[];
  rnd_prim_t* prims = reinterpret_cast<rnd_prim_t*>(rnd_smem);  // RND_BLOCK of them
  const int tid = threadIdx.x, W = a.W, H = a.H;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int tc0 = tx * RND_TILE_W, tr0 = ty * RND_TILE_H;
  const int tc1 = min(tc0 + RND_TILE_W, W) - 1, tr1 = min(tr0 + RND_TILE_H, H) - 1;
  const int r = tr0 + (tid >> 4), c = tc0 + RND_LANE_PX * (tid & 15);
  const bool mine = r <= tr1 && c <= tc1;
  uint32_t m[RND_LANE_PX] = {0u, 0u, 0u, 0u};
  const long total = a.stride > 1 ? (long)a.n_paths * 2 * (a.stride - 1) : 0;
  for (long g0 = 0; g0 < total; g0 += RND_BLOCK) {
    if (g0 + tid < total) rnd_boundary_prim(g0 + tid, a.view, W, H, a.h_b, a.left, a.right, a.n_left, a.n_right, a.stride, prims + tid);
    else rnd_none(prims + tid);
    __syncthreads();
    for (int t = 0; t < RND_BLOCK; ++t) {
      const rnd_prim_t* q = prims + t;
      if (!rnd_box_hits(q, tc0, tc1, tr0, tr1)) continue;  // (the same for every lane)
      if (!mine || r < q->r0 || r > q->r1 || c + RND_LANE_PX - 1 < q->c0 || c > q->c1) continue;
#pragma unroll
      for (int p = 0; p < RND_LANE_PX; ++p) {
        if (c + p < q->c0 || c + p > q->c1) continue;
#pragma unroll
        for (int j = 0; j < S; ++j)
#pragma unroll
          for (int i = 0; i < S; ++i)
            if (rnd_covers(q, rnd_sample(c + p, i, S), rnd_sample(r, j, S))) m[p] |= 1u << (j * S + i);
      }
    }
    __syncthreads();
  }
  if (!mine) return;
  const uint2 mw = make_uint2(m[0] | (m[1] << 16), m[2] | (m[3] << 16));
  *reinterpret_cast<uint2*>(a.mask + (size_t)r * W + c) = mw;
  uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
  for (int p = 0; p < RND_LANE_PX; ++p) shade_px<S>((const rnd_prim_t*)nullptr, (const uint16_t*)nullptr, 0, r, c, p, mw, a.pal, w);  // the map alone: no primitive
  store_px4(a.bg_rgb, W, r, c, w);
}

}  // namespace render

struct sigmaenv_render {
  sigmaenv* owner = nullptr;  // the handle it was created on (null once that handle is destroyed)
  int B = 0, N = 0, W = 0, H = 0, S = 1, flags = 0, n_sel = 0, ring_frames = 0, P = 0;
  rnd_view_t view{};
  float h_b = 0.0f, h_p = 0.0f;
  void* mem = nullptr;        // coverage u16 [H,W], colours u8 [H,W,3], palette u8 [4+N,3], selection i32 [n_sel]: one allocation, every part at a multiple of 16 bytes
  uint16_t* mask = nullptr;
  uint8_t* bg_rgb = nullptr;
  uint8_t* pal = nullptr;
  int32_t* sel = nullptr;
  uint8_t* ring = nullptr;    // [ring_frames, n_sel, H, W, 3] or null
  uint64_t frames = 0;        // frames drawn so far (host count), into the ring or into a caller's tensor
  int32_t newest = -1;        // the ring slot of the newest ring frame, -1 before the first
  uint64_t ring_drawn = 0;    // frames drawn into the ring
  size_t frame_bytes() const { return (size_t)n_sel * H * W * 3; }
};

static bool render_owned(sigmaenv* h, const sigmaenv_render* r, const char* what) {
  if (!r) { h->err = std::string(what) + ": null renderer"; return false; }
  if (r->owner != h) { h->err = std::string(what) + ": the renderer belongs to another handle"; return false; }
  return true;
}

// sigmaenv_destroy: the handle's renderers stay valid for sigmaenv_render_destroy alone
static void render_orphan(sigmaenv* h) {
  for (sigmaenv_render* r : h->renders) r->owner = nullptr;
  h->renders.clear();
  h->render_attached = nullptr;
}

extern "C" void sigmaenv_render_destroy(sigmaenv_render* r) {
  if (!r) return;
  if (sigmaenv* h = r->owner) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);  // launches that still read or write its memory
    if (h->render_attached == r) h->render_attached = nullptr;
    for (size_t k = 0; k < h->renders.size(); ++k)
      if (h->renders[k] == r) { h->renders.erase(h->renders.begin() + (long)k); break; }
  }
  if (r->mem) (void)hipFree(r->mem);
  if (r->ring) (void)hipFree(r->ring);
  delete r;
}

extern "C" int sigmaenv_render_create(sigmaenv_t* h, const sigmaenv_render_args_t* args, sigmaenv_render** out) {
  if (!h || !out) return SIGMAENV_EINVAL;
  *out = nullptr;
  if (!args || !args->palette || !args->selection) { h->err = "render_create: arguments, palette and selection are required"; return SIGMAENV_EINVAL; }
  const int W = args->width, H = args->height, S = args->samples;
  if (W < 4 || W > RND_MAX_DIM || (W & 3) || H < 1 || H > RND_MAX_DIM) {
    h->err = "render_create: width must be a multiple of 4 (a lane writes four pixels as three dwords), width and height within [1, 16384]";
    return SIGMAENV_EINVAL;
  }
  if (!rnd_samples_ok(S)) { h->err = "render_create: samples per axis must be 1, 2 or 4"; return SIGMAENV_EINVAL; }
  if (!(rnd_finite(args->scale) && args->scale > 0.0f && rnd_finite(args->x0) && rnd_finite(args->y1) && rnd_finite(args->h_boundary) && args->h_boundary >= 0.0f &&
        rnd_finite(args->h_path) && args->h_path >= 0.0f)) {
    h->err = "render_create: the view must be finite with a positive scale, the half-widths finite and >= 0";
    return SIGMAENV_EINVAL;
  }
  if (args->n_sel < 1 || args->n_sel > 65535 || args->ring_frames < 0 || (args->flags & ~RND_FLAG_SHORT_TERM)) {
    h->err = "render_create: 1 <= n_sel <= 65535, ring_frames >= 0, flags within SIGMAENV_RENDER_SHORT_TERM";
    return SIGMAENV_EINVAL;
  }
  for (int k = 0; k < args->n_sel; ++k)
    if (args->selection[k] < 0 || args->selection[k] >= h->B) {
      h->err = "render_create: selection[" + std::to_string(k) + "] = " + std::to_string(args->selection[k]) + " is outside [0, n_envs)";
      return SIGMAENV_EINVAL;
    }
  const size_t frame = (size_t)args->n_sel * H * W * 3;
  if (frame >= ((size_t)1 << 40) || (args->ring_frames > 0 && frame * (size_t)args->ring_frames >= ((size_t)1 << 40))) {
    h->err = "render_create: the frames [ring_frames, n_sel, H, W, 3] must stay below 2^40 bytes";
    return SIGMAENV_EINVAL;
  }
  HIPCHK(h, hipSetDevice(h->device));
  auto* r = new sigmaenv_render();
  r->B = h->B; r->N = h->N; r->W = W; r->H = H; r->S = S; r->flags = args->flags; r->n_sel = args->n_sel; r->ring_frames = args->ring_frames;
  r->view.s = args->scale; r->view.x0 = args->x0; r->view.y1 = args->y1;
  r->h_b = args->h_boundary; r->h_p = args->h_path;
  r->P = rnd_prim_count(h->N, NS, r->flags);
  const size_t px = (size_t)H * W, o_rgb = render::align16(px * 2), o_pal = o_rgb + render::align16(px * 3), o_sel = o_pal + render::align16((size_t)(4 + h->N) * 3);
  const size_t bytes = o_sel + render::align16((size_t)r->n_sel * 4);
  hipError_t e = hipMalloc(&r->mem, bytes);
  if (e == hipSuccess && r->ring_frames > 0) e = hipMalloc((void**)&r->ring, frame * (size_t)r->ring_frames);
  if (e != hipSuccess) {
    h->err = std::string("render_create: hipMalloc: ") + hipGetErrorString(e);
    sigmaenv_render_destroy(r);
    return SIGMAENV_ENOMEM;
  }
  r->mask = (uint16_t*)r->mem;
  r->bg_rgb = (uint8_t*)r->mem + o_rgb;
  r->pal = (uint8_t*)r->mem + o_pal;
  r->sel = (int32_t*)((uint8_t*)r->mem + o_sel);
  r->owner = h;
  h->renders.push_back(r);
  std::vector<uint8_t> pal((size_t)(4 + h->N) * 3);
  rnd_palette_fill(args->palette, h->N, pal.data());
  int rc = SIGMAENV_OK;
  // (pageable host memory: both copies have left the host buffers when the calls return)
  if (hipMemcpyAsync(r->pal, pal.data(), pal.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(r->sel, args->selection, (size_t)r->n_sel * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess) {
    h->err = "render_create: copying palette and selection failed";
    rc = SIGMAENV_EHIP;
  }
  if (!rc && r->ring && hipMemsetAsync(r->ring, 0, frame * (size_t)r->ring_frames, h->stream) != hipSuccess) { h->err = "render_create: hipMemsetAsync"; rc = SIGMAENV_EHIP; }
  if (!rc) {
    render::BackgroundArgs a{};
    a.view = r->view; a.W = W; a.H = H; a.tiles_x = (W + RND_TILE_W - 1) / RND_TILE_W; a.n_paths = h->map.n_paths; a.stride = h->map.P; a.h_b = r->h_b;
    a.left = h->map.left; a.right = h->map.right; a.n_left = h->map.n_left; a.n_right = h->map.n_right; a.pal = r->pal; a.mask = r->mask; a.bg_rgb = r->bg_rgb;
    const dim3 grid((unsigned)(a.tiles_x * ((H + RND_TILE_H - 1) / RND_TILE_H)));
    const size_t lds = RND_BLOCK * sizeof(rnd_prim_t);
    if (S == 1) hipLaunchKernelGGL(render::sigmaenv_render_background_kernel<1>, grid, dim3(RND_BLOCK), lds, h->stream, a);
    else if (S == 2) hipLaunchKernelGGL(render::sigmaenv_render_background_kernel<2>, grid, dim3(RND_BLOCK), lds, h->stream, a);
    else hipLaunchKernelGGL(render::sigmaenv_render_background_kernel<4>, grid, dim3(RND_BLOCK), lds, h->stream, a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { h->err = std::string("render_create: background launch: ") + hipGetErrorString(le); rc = SIGMAENV_EHIP; }
  }
  if (rc) { sigmaenv_render_destroy(r); return rc; }
  *out = r;
  return SIGMAENV_OK;
}

static int render_frame_impl(sigmaenv* h, sigmaenv_render* r, const sigmaenv_render_src_t* src, uint8_t* out) {
  render::FrameArgs a{};
  a.vertices = src && src->vertices ? src->vertices : (const float*)h->buf.vertices;
  a.short_term = src && src->short_term ? src->short_term : (const float*)h->buf.short_term;
  a.state = src && src->state ? src->state : (const float*)h->buf.state;
  a.col_agents = src && src->col_agents ? src->col_agents : (const uint8_t*)h->buf.col_agents;
  a.col_flags = src && src->col_flags ? src->col_flags : (const uint8_t*)h->buf.col_flags;
  const void* ptrs[] = {a.vertices, a.short_term, a.state, a.col_agents, a.col_flags};
  for (const void* p : ptrs)
    if ((uintptr_t)p & 3) { h->err = "render_frame: an override that is not 4-byte aligned"; return SIGMAENV_EINVAL; }
  if ((uintptr_t)out & 15) { h->err = "render_frame: out must be 16-byte aligned"; return SIGMAENV_EINVAL; }
  int32_t slot = -1;
  if (!out) {
    if (!r->ring) { h->err = "render_frame: no destination and the renderer was created without a ring (ring_frames = 0)"; return SIGMAENV_EINVAL; }
    slot = (int32_t)(r->ring_drawn % (uint64_t)r->ring_frames);
    out = r->ring + (size_t)slot * r->frame_bytes();
  }
  HIPCHK(h, hipSetDevice(h->device));
  a.view = r->view; a.W = r->W; a.H = r->H; a.N = r->N; a.flags = r->flags; a.P = r->P; a.tiles_x = (r->W + RND_TILE_W - 1) / RND_TILE_W; a.vec16 = (r->W & 15) == 0;
  a.h_p = r->h_p; a.r_disc = rnd_disc_radius(r->view.s);
  a.mask = r->mask; a.bg_rgb = r->bg_rgb; a.pal = r->pal; a.sel = r->sel; a.out = out;
  const int tiles_y = (r->H + RND_TILE_H - 1) / RND_TILE_H;
  const dim3 grid((unsigned)(a.tiles_x * ((tiles_y + RND_STRIP - 1) / RND_STRIP)), (unsigned)r->n_sel);
  const size_t lds = render::frame_lds(r->P, r->N);
  if (r->S == 1) hipLaunchKernelGGL(render::sigmaenv_render_frame_kernel<1>, grid, dim3(RND_BLOCK), lds, h->stream, a);
  else if (r->S == 2) hipLaunchKernelGGL(render::sigmaenv_render_frame_kernel<2>, grid, dim3(RND_BLOCK), lds, h->stream, a);
  else hipLaunchKernelGGL(render::sigmaenv_render_frame_kernel<4>, grid, dim3(RND_BLOCK), lds, h->stream, a);
  HIPCHK(h, hipGetLastError());
  r->frames += 1;
  if (slot >= 0) { r->newest = slot; r->ring_drawn += 1; }
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_render_frame(sigmaenv_t* h, sigmaenv_render* r, const sigmaenv_render_src_t* src, uint8_t* out) {
  if (!h) return SIGMAENV_EINVAL;
  if (!render_owned(h, r, "render_frame")) return SIGMAENV_EINVAL;
  return render_frame_impl(h, r, src, out);
}

extern "C" int sigmaenv_render_attach(sigmaenv_t* h, sigmaenv_render* r, int32_t every) {
  if (!h) return SIGMAENV_EINVAL;
  if (r) {
    if (!render_owned(h, r, "render_attach")) return SIGMAENV_EINVAL;
    if (every < 1) { h->err = "render_attach: every must be >= 1"; return SIGMAENV_EINVAL; }
    if (!r->ring) { h->err = "render_attach: the renderer was created without a ring (ring_frames = 0)"; return SIGMAENV_EINVAL; }
  }
  h->render_attached = r;
  h->render_every = r ? every : 1;
  h->render_steps = 0;
  return SIGMAENV_OK;
}

// one step of an attached rollout is over (launch_cbf_then_step): the frame of every `every`-th step since the attachment
static int render_attached_step(sigmaenv* h) {
  h->render_steps += 1;
  if (h->render_steps % (uint64_t)h->render_every) return SIGMAENV_OK;
  return render_frame_impl(h, h->render_attached, nullptr, nullptr);
}

extern "C" int sigmaenv_render_get(sigmaenv_t* h, sigmaenv_render* r, void** ring, uint64_t* frames, uint64_t* ring_drawn, int32_t* newest_slot) {
  if (!h) return SIGMAENV_EINVAL;
  if (!render_owned(h, r, "render_get")) return SIGMAENV_EINVAL;
  if (ring) *ring = r->ring;
  if (frames) *frames = r->frames;
  if (ring_drawn) *ring_drawn = r->ring_drawn;
  if (newest_slot) *newest_slot = r->newest;
  return SIGMAENV_OK;
}
