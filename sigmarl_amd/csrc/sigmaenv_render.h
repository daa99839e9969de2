// sigmaenv_render.h -- the picture of an env, stated ONCE: a top-down frame of map, short-term paths and vehicles as uint8 RGB, a function of the per-step output
// buffers, the map table's boundary polylines, a view and a palette alone.  The reference draws the same list of things through a pyglet scene graph
// (sigmarl/scenarios/road_traffic.py:1637-1800, extra_render: the lane boundaries :1700-1730 behind is_visualize_lane_boundary, the short-term reference paths with a
// dot per point :1660-1698 behind is_visualize_short_term_path; the vehicle rectangles and their colours are the agents' own shapes, :560-600); it supplies the LIST,
// this header is the specification of the pixels.  The kernels of sigmaenv_render.inc run these functions on the device; a host program runs them on the host
// (tests/test_render_check.py holds them bit for bit to the float32 twin of tests/render_check.py, which a float64 bracket checks independently).
//
// Plain C++: no HIP include and no other file of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.  As in include/sigma_trig_f32.h, both sides are compiled with -ffp-contract=off and every product and every
// sum below is a statement of its own, so every operator is ONE IEEE fp32 operation in the order written: neither compiler may fuse a product into a sum.
//
// VIEW.  Three floats: the scale s in pixels per metre and (x0, y1), the world point of the image's top-left corner.  px = (x - x0) * s, py = (y1 - y) * s: one
// subtraction, then one multiplication (rnd_px, rnd_py); row 0 is the top of the image.  Pixel (r, c) with S samples per axis, S in {1, 2, 4}, has the S * S sample
// points (c + (2 i + 1) / (2 S), r + (2 j + 1) / (2 S)), i, j = 0 .. S-1 (rnd_sample: the offset is an exact fp32 number, the sum is exact below 2^20), sample (j, i)
// has the number j * S + i.
//
// PREDICATES, fp32 on pixel coordinates:
//   quad (rnd_in_quad): the four edge functions (bx - ax) * (py - ay) - (by - ay) * (px - ax) of the edges 0-1, 1-2, 2-3, 3-0 are all >= 0 or all <= 0 (either
//     winding).  A quad whose doubled signed area (x2 - x0) * (y3 - y1) - (x3 - x1) * (y2 - y0) is 0, or with a non-finite vertex, draws nothing.
//   thick segment a -> b with half-width h (rnd_in_segment), no division: d = b - a, w = p - a, q = wx * dx + wy * dy, dd = dx * dx + dy * dy, hh = h * h;
//     q <= 0: wx * wx + wy * wy <= hh;  q >= dd: |p - b|^2 <= hh;  else (wx * dy - wy * dx)^2 <= hh * dd.  A segment with a non-finite end draws nothing.
//   disc (rnd_in_disc): (px - cx)^2 + (py - cy)^2 <= r * r.  A non-finite centre draws nothing.
//
// BOX.  Every primitive has a box of pixels [c0, c1] x [r0, r1] (rnd_box): the extent of its points in pixel coordinates, inflated by its half-width (radius),
// clamped to [0, W] x [0, H] IN FLOATING POINT and only then converted -- c0 = (int)lo, c1 = min((int)hi, W - 1) -- so that no NaN, infinity or huge coordinate is
// ever converted to an integer; a primitive that draws nothing, or whose clamped extent is empty, has the empty box (c0 > c1).  The box is part of the picture: the
// samples of a pixel are tested against a primitive only if the pixel lies in its box.  (A sample is >= 1/8 pixel away from every pixel border, the roundings of
// the box are ~2^-24 of a coordinate: for coordinates below 2^16 pixels the box removes nothing the predicates would draw.)
//
// LAYERS.  A sample takes the colour of the LAST primitive that covers it, in this order:
//   0  the background colour (palette entry 0);
//   1  lane boundaries (entry 1): the segments k -> k + 1 of the `left` and `right` polylines of EVERY path of the map table (n_left / n_right points), half-width h_b;
//   2  only with RND_FLAG_SHORT_TERM: per agent i ascending, in its colour (entry 3 + i): the n_st - 1 segments through its n_st short-term points, half-width h_p,
//      then a disc of radius RND_DISC_M * s (ONE fp32 product, rnd_disc_radius) on each of the n_st points;
//   3  per agent i ascending: the quad of vertices[b, i, 0:4] in its colour, or in the collision colour (entry 2) when any byte of col_agents[b, i, :] or byte 0 of
//      col_flags[b, i, :] is set; then the heading mark, black: the segment from state[b, i, 0:2] to the midpoint of the front edge, half-width h_p.  The front edge is
//      vertices 0 and 1 (rect_vertices, sigmaenv_device.h: the body-frame corners (+l/2, +w/2), (+l/2, -w/2) come first); the midpoint is formed in pixel
//      coordinates, (p0 + p1) * 0.5f per axis: one sum, one exact halving.
// An env's primitives of layers 2 and 3 in that order are numbered 0 .. P-1 (rnd_prim_count, rnd_env_prim); n_st is the build's n_points_short_term.
//
// PIXEL.  Per channel (sum of the S * S sample colours + S * S / 2) / (S * S) in integer arithmetic (rnd_pixel).
//
// PALETTE.  u8 [3 + N, 3]: background, boundary, collision, then the agents.  The mark colour is fixed black: the functions below take the palette with one more
// entry, index 3 + N = (0, 0, 0), appended (rnd_palette_fill).
//
// BACKGROUND.  Layers 0 and 1 do not change with the step: they are rasterised once into a coverage image u16 [H, W] -- bit j * S + i of pixel (r, c) is set when
// a boundary segment covers sample (j, i); the low S * S bits are used -- and into the resolved colours u8 [H, W, 3] of the map alone (rnd_pixel with no primitive).
// (Chosen over the supersampled index image: 2 bytes per pixel for every S instead of S * S.)
//
// TILE WALK.  The image is cut into tiles of RND_TILE_W x RND_TILE_H pixels; a lane of the kernel owns RND_LANE_PX horizontally adjacent pixels, so W must be a
// multiple of 4.  A primitive is LISTED for a tile when its box meets the tile's pixels (rnd_box_hits); the list keeps the primitives' order and holds up to
// RND_LIST_CAP; a tile with more walks ALL P primitives instead (each still behind its own box: nothing is dropped and nothing changes).  A tile with an empty
// list is the background's resolved colours.  rnd_frame_env below is that walk on a host, rnd_background the background.
#ifndef SIGMAENV_RENDER_H
#define SIGMAENV_RENDER_H
#include <math.h>
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define RND_TILE_W 64
#define RND_TILE_H 16
#define RND_LANE_PX 4
#define RND_BLOCK 256    /* (RND_TILE_W / RND_LANE_PX) * RND_TILE_H lanes */
#define RND_LIST_CAP 48  /* primitives listed per tile; more: the tile walks all of them */
#define RND_MAX_DIM 16384 /* H, W <= this: a box fits int16 */
#define RND_MAX_SAMPLES 4
#define RND_FLAG_SHORT_TERM 1
#define RND_PAL_BACKGROUND 0
#define RND_PAL_BOUNDARY 1
#define RND_PAL_COLLISION 2
#define RND_PAL_AGENT0 3
#define RND_KIND_NONE 0
#define RND_KIND_QUAD 1
#define RND_KIND_SEGMENT 2
#define RND_KIND_DISC 3
#define RND_DISC_M 0.01f
#define RND_FLT_MAX 3.402823466e+38f

typedef struct rnd_view {
  float s, x0, y1;
} rnd_view_t;

/* quad: p[0..7] = four points (x, y);  segment: p[0..3] = a, b, p[4] = h;  disc: p[0..1] = c, p[2] = r.  All in pixel coordinates. */
typedef struct rnd_prim {
  float p[8];
  int16_t c0, c1, r0, r1;
  uint16_t kind, colour;
} rnd_prim_t;

SIGMA_HD float rnd_px(rnd_view_t v, float x) {
  const float d = x - v.x0;
  return d * v.s;
}
SIGMA_HD float rnd_py(rnd_view_t v, float y) {
  const float d = v.y1 - y;
  return d * v.s;
}
SIGMA_HD float rnd_sample(int c, int i, int S) {
  const float o = (float)(2 * i + 1) / (float)(2 * S);
  return (float)c + o;
}
SIGMA_HD float rnd_disc_radius(float s) { return RND_DISC_M * s; }
SIGMA_HD int rnd_finite(float x) { return fabsf(x) <= RND_FLT_MAX; } /* 0 for NaN and the infinities */
SIGMA_HD float rnd_min(float a, float b) { return a < b ? a : b; }
SIGMA_HD float rnd_max(float a, float b) { return a > b ? a : b; }
SIGMA_HD int rnd_samples_ok(int S) { return S == 1 || S == 2 || S == 4; }

SIGMA_HD void rnd_none(rnd_prim_t* q) {
  for (int k = 0; k < 8; ++k) q->p[k] = 0.0f;
  q->c0 = 32767; q->c1 = -1; q->r0 = 32767; q->r1 = -1;
  q->kind = RND_KIND_NONE; q->colour = 0;
}

/* one axis of the box: FINITE extent [mn, mx], finite inflation h >= 0, n = W or H.  Returns 0 for an empty range. */
SIGMA_HD int rnd_box_axis(float mn, float mx, float h, int n, int16_t* i0, int16_t* i1) {
  float lo = mn - h;
  float hi = mx + h;
  lo = lo > 0.0f ? lo : 0.0f;
  hi = hi < (float)n ? hi : (float)n;
  if (!(lo <= hi) || !(lo < (float)n)) return 0; /* (also what a NaN would end as) */
  int a = (int)lo, b = (int)hi;                  /* both in [0, n] */
  if (b > n - 1) b = n - 1;
  *i0 = (int16_t)a; *i1 = (int16_t)b;
  return 1;
}
SIGMA_HD void rnd_box(float mnx, float mxx, float mny, float mxy, float h, int W, int H, rnd_prim_t* q) {
  if (!rnd_box_axis(mnx, mxx, h, W, &q->c0, &q->c1) || !rnd_box_axis(mny, mxy, h, H, &q->r0, &q->r1)) rnd_none(q);
}
SIGMA_HD int rnd_box_hits(const rnd_prim_t* q, int c0, int c1, int r0, int r1) { return q->c0 <= c1 && q->c1 >= c0 && q->r0 <= r1 && q->r1 >= r0; }

/* v: four points (x, y) in pixel coordinates */
SIGMA_HD void rnd_make_quad(const float* v, int colour, int W, int H, rnd_prim_t* q) {
  int ok = 1;
  for (int k = 0; k < 8; ++k) ok &= rnd_finite(v[k]);
  if (!ok) { rnd_none(q); return; }
  const float d1x = v[4] - v[0], d1y = v[7] - v[3], d2x = v[6] - v[2], d2y = v[5] - v[1];
  const float m1 = d1x * d1y;
  const float m2 = d2x * d2y;
  const float area2 = m1 - m2;
  if (area2 == 0.0f) { rnd_none(q); return; }
  for (int k = 0; k < 8; ++k) q->p[k] = v[k];
  q->kind = RND_KIND_QUAD; q->colour = (uint16_t)colour;
  rnd_box(rnd_min(rnd_min(v[0], v[2]), rnd_min(v[4], v[6])), rnd_max(rnd_max(v[0], v[2]), rnd_max(v[4], v[6])), rnd_min(rnd_min(v[1], v[3]), rnd_min(v[5], v[7])),
          rnd_max(rnd_max(v[1], v[3]), rnd_max(v[5], v[7])), 0.0f, W, H, q);
}
SIGMA_HD void rnd_make_segment(float ax, float ay, float bx, float by, float h, int colour, int W, int H, rnd_prim_t* q) {
  if (!(rnd_finite(ax) && rnd_finite(ay) && rnd_finite(bx) && rnd_finite(by))) { rnd_none(q); return; }
  q->p[0] = ax; q->p[1] = ay; q->p[2] = bx; q->p[3] = by; q->p[4] = h; q->p[5] = 0.0f; q->p[6] = 0.0f; q->p[7] = 0.0f;
  q->kind = RND_KIND_SEGMENT; q->colour = (uint16_t)colour;
  rnd_box(rnd_min(ax, bx), rnd_max(ax, bx), rnd_min(ay, by), rnd_max(ay, by), h, W, H, q);
}
SIGMA_HD void rnd_make_disc(float cx, float cy, float r, int colour, int W, int H, rnd_prim_t* q) {
  if (!(rnd_finite(cx) && rnd_finite(cy))) { rnd_none(q); return; }
  q->p[0] = cx; q->p[1] = cy; q->p[2] = r;
  for (int k = 3; k < 8; ++k) q->p[k] = 0.0f;
  q->kind = RND_KIND_DISC; q->colour = (uint16_t)colour;
  rnd_box(cx, cx, cy, cy, r, W, H, q);
}

SIGMA_HD int rnd_in_quad(const float* p, float x, float y) {
  int pos = 1, neg = 1;
  for (int k = 0; k < 4; ++k) {
    const int n = (k + 1) & 3;
    const float ex = p[2 * n] - p[2 * k], ey = p[2 * n + 1] - p[2 * k + 1];
    const float wx = x - p[2 * k], wy = y - p[2 * k + 1];
    const float m1 = ex * wy;
    const float m2 = ey * wx;
    const float e = m1 - m2;
    pos &= e >= 0.0f;
    neg &= e <= 0.0f;
  }
  return pos | neg;
}
SIGMA_HD int rnd_in_segment(const float* p, float x, float y) {
  const float dx = p[2] - p[0], dy = p[3] - p[1];
  const float wx = x - p[0], wy = y - p[1];
  const float q1 = wx * dx;
  const float q2 = wy * dy;
  const float q = q1 + q2;
  const float d1 = dx * dx;
  const float d2 = dy * dy;
  const float dd = d1 + d2;
  const float hh = p[4] * p[4];
  if (q <= 0.0f) {
    const float w1 = wx * wx;
    const float w2 = wy * wy;
    const float ww = w1 + w2;
    return ww <= hh;
  }
  if (q >= dd) {
    const float ux = x - p[2], uy = y - p[3];
    const float u1 = ux * ux;
    const float u2 = uy * uy;
    const float uu = u1 + u2;
    return uu <= hh;
  }
  const float c1 = wx * dy;
  const float c2 = wy * dx;
  const float cr = c1 - c2;
  const float cc = cr * cr;
  const float lim = hh * dd;
  return cc <= lim;
}
SIGMA_HD int rnd_in_disc(const float* p, float x, float y) {
  const float ux = x - p[0], uy = y - p[1];
  const float u1 = ux * ux;
  const float u2 = uy * uy;
  const float uu = u1 + u2;
  const float rr = p[2] * p[2];
  return uu <= rr;
}
SIGMA_HD int rnd_covers(const rnd_prim_t* q, float x, float y) {
  if (q->kind == RND_KIND_QUAD) return rnd_in_quad(q->p, x, y);
  if (q->kind == RND_KIND_SEGMENT) return rnd_in_segment(q->p, x, y);
  if (q->kind == RND_KIND_DISC) return rnd_in_disc(q->p, x, y);
  return 0;
}

/* ---- the primitives of one env ------------------------------------------------------------------------------------------------------------------------------- */
SIGMA_HD int rnd_prim_count(int N, int n_st, int flags) { return ((flags & RND_FLAG_SHORT_TERM) ? N * (2 * n_st - 1) : 0) + 2 * N; }

/* primitive k of an env, from the env's rows: vertices [N,5,2], short_term [N,n_st,2], state [N,8], col_agents [N,N] u8, col_flags [N,4] u8 */
SIGMA_HD void rnd_env_prim(int k, int N, int n_st, int flags, rnd_view_t v, int W, int H, float h_p, float r_disc, const float* vertices, const float* short_term,
                           const float* state, const uint8_t* col_agents, const uint8_t* col_flags, rnd_prim_t* q) {
  const int per = 2 * n_st - 1;
  const int n2 = (flags & RND_FLAG_SHORT_TERM) ? N * per : 0;
  if (k < n2) {  /* layer 2 */
    const int i = k / per, m = k - i * per;
    const float* st = short_term + (long)i * n_st * 2;
    if (m < n_st - 1)
      rnd_make_segment(rnd_px(v, st[2 * m]), rnd_py(v, st[2 * m + 1]), rnd_px(v, st[2 * m + 2]), rnd_py(v, st[2 * m + 3]), h_p, RND_PAL_AGENT0 + i, W, H, q);
    else
      rnd_make_disc(rnd_px(v, st[2 * (m - (n_st - 1))]), rnd_py(v, st[2 * (m - (n_st - 1)) + 1]), r_disc, RND_PAL_AGENT0 + i, W, H, q);
    return;
  }
  const int k3 = k - n2, i = k3 >> 1;  /* layer 3 */
  const float* vt = vertices + (long)i * 10;
  float pv[8];
  for (int c = 0; c < 4; ++c) { pv[2 * c] = rnd_px(v, vt[2 * c]); pv[2 * c + 1] = rnd_py(v, vt[2 * c + 1]); }
  if (!(k3 & 1)) {
    int hit = col_flags[i * 4] != 0;
    for (int j = 0; j < N; ++j) hit |= col_agents[(long)i * N + j] != 0;
    rnd_make_quad(pv, hit ? RND_PAL_COLLISION : RND_PAL_AGENT0 + i, W, H, q);
  } else {
    const float sx = pv[0] + pv[2];
    const float sy = pv[1] + pv[3];
    rnd_make_segment(rnd_px(v, state[i * 8]), rnd_py(v, state[i * 8 + 1]), sx * 0.5f, sy * 0.5f, h_p, RND_PAL_AGENT0 + N, W, H, q);
  }
}

/* ---- one pixel --------------------------------------------------------------------------------------------------------------------------------------------------
 * prims: the env's primitives; list: n indices in order, or NULL for the primitives 0 .. n-1 themselves; mask: the pixel's word of the coverage image;
 * pal: u8 [(4 + N), 3], black appended.  rgb[0..2]. */
SIGMA_HD void rnd_pixel(const rnd_prim_t* prims, const uint16_t* list, int n, int r, int c, int S, uint32_t mask, const uint8_t* pal, uint8_t* rgb) {
  uint16_t idx[RND_MAX_SAMPLES * RND_MAX_SAMPLES];
  const int SS = S * S;
  for (int t = 0; t < SS; ++t) idx[t] = ((mask >> t) & 1u) ? RND_PAL_BOUNDARY : RND_PAL_BACKGROUND;
  for (int t = 0; t < n; ++t) {
    const rnd_prim_t* q = prims + (list ? list[t] : t);
    if (r < q->r0 || r > q->r1 || c < q->c0 || c > q->c1) continue;
    for (int j = 0; j < S; ++j)
      for (int i = 0; i < S; ++i)
        if (rnd_covers(q, rnd_sample(c, i, S), rnd_sample(r, j, S))) idx[j * S + i] = q->colour;
  }
  for (int ch = 0; ch < 3; ++ch) {
    uint32_t sum = 0;
    for (int t = 0; t < SS; ++t) sum += pal[idx[t] * 3 + ch];
    rgb[ch] = (uint8_t)((sum + (uint32_t)(SS / 2)) / (uint32_t)SS);
  }
}

/* ---- the same on a host: palette, background, one env's frame ------------------------------------------------------------------------------------------------------ */
static inline void rnd_palette_fill(const uint8_t* palette /*[3 + N, 3]*/, int N, uint8_t* pal /*[4 + N, 3]*/) {
  for (int k = 0; k < (3 + N) * 3; ++k) pal[k] = palette[k];
  pal[(3 + N) * 3] = 0; pal[(3 + N) * 3 + 1] = 0; pal[(3 + N) * 3 + 2] = 0;
}

/* boundary segment number g of the map table (left / right [n_paths, stride, 2], n_left / n_right [n_paths]): path g / (2 (stride - 1)), then side, then k -> k + 1;
 * a number beyond the polyline's last segment is no primitive */
SIGMA_HD void rnd_boundary_prim(long g, rnd_view_t v, int W, int H, float h_b, const float* left, const float* right, const int32_t* n_left, const int32_t* n_right, int stride,
                                rnd_prim_t* q) {
  const int per = stride - 1;
  const long ps = g / per;
  const int k = (int)(g - ps * per), p = (int)(ps >> 1), side = (int)(ps & 1);
  const int n = side ? n_right[p] : n_left[p];
  if (k + 1 >= n) { rnd_none(q); return; }
  const float* a = (side ? right : left) + ((long)p * stride + k) * 2;
  rnd_make_segment(rnd_px(v, a[0]), rnd_py(v, a[1]), rnd_px(v, a[2]), rnd_py(v, a[3]), h_b, RND_PAL_BOUNDARY, W, H, q);
}

static inline void rnd_background(rnd_view_t v, int W, int H, int S, float h_b, const float* left, const float* right, const int32_t* n_left, const int32_t* n_right, int n_paths,
                                  int stride, const uint8_t* pal, uint16_t* mask /*[H, W]*/, uint8_t* rgb /*[H, W, 3]*/) {
  for (long k = 0; k < (long)H * W; ++k) mask[k] = 0;
  const long total = stride > 1 ? (long)n_paths * 2 * (stride - 1) : 0;
  for (long g = 0; g < total; ++g) {
    rnd_prim_t q;
    rnd_boundary_prim(g, v, W, H, h_b, left, right, n_left, n_right, stride, &q);
    for (int r = q.r0; r <= q.r1; ++r)
      for (int c = q.c0; c <= q.c1; ++c)
        for (int j = 0; j < S; ++j)
          for (int i = 0; i < S; ++i)
            if (rnd_covers(&q, rnd_sample(c, i, S), rnd_sample(r, j, S))) mask[(long)r * W + c] |= (uint16_t)(1u << (j * S + i));
  }
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) rnd_pixel((const rnd_prim_t*)0, (const uint16_t*)0, 0, r, c, S, mask[(long)r * W + c], pal, rgb + ((long)r * W + c) * 3);
}

/* one frame of one env: prims = scratch for rnd_prim_count primitives; out [H, W, 3] */
static inline void rnd_frame_env(rnd_view_t v, int W, int H, int S, int N, int n_st, int flags, float h_p, const uint16_t* mask, const uint8_t* bg_rgb, const uint8_t* pal,
                                 const float* vertices, const float* short_term, const float* state, const uint8_t* col_agents, const uint8_t* col_flags, rnd_prim_t* prims,
                                 uint8_t* out) {
  const int P = rnd_prim_count(N, n_st, flags);
  const float r_disc = rnd_disc_radius(v.s);
  for (int k = 0; k < P; ++k) rnd_env_prim(k, N, n_st, flags, v, W, H, h_p, r_disc, vertices, short_term, state, col_agents, col_flags, prims + k);
  for (int tr0 = 0; tr0 < H; tr0 += RND_TILE_H)
    for (int tc0 = 0; tc0 < W; tc0 += RND_TILE_W) {
      const int tr1 = (tr0 + RND_TILE_H < H ? tr0 + RND_TILE_H : H) - 1, tc1 = (tc0 + RND_TILE_W < W ? tc0 + RND_TILE_W : W) - 1;
      uint16_t list[RND_LIST_CAP];
      int n = 0;
      for (int k = 0; k < P; ++k)
        if (rnd_box_hits(prims + k, tc0, tc1, tr0, tr1)) {
          if (n < RND_LIST_CAP) list[n] = (uint16_t)k;
          ++n;
        }
      for (int r = tr0; r <= tr1; ++r)
        for (int c = tc0; c <= tc1; ++c) {
          uint8_t* o = out + ((long)r * W + c) * 3;
          if (n == 0) { o[0] = bg_rgb[((long)r * W + c) * 3]; o[1] = bg_rgb[((long)r * W + c) * 3 + 1]; o[2] = bg_rgb[((long)r * W + c) * 3 + 2]; }
          else if (n <= RND_LIST_CAP) rnd_pixel(prims, list, n, r, c, S, mask[(long)r * W + c], pal, o);
          else rnd_pixel(prims, (const uint16_t*)0, P, r, c, S, mask[(long)r * W + c], pal, o);
        }
    }
}
#endif  // SIGMAENV_RENDER_H
