// sigmaenv_snapshot.h -- the state of an env handle, stated ONCE: which device buffers a snapshot holds, where each lies in the blob, and the index arithmetic that
// takes one piece of the flat copy grid to its (segment, block, env) and to its byte offsets in the live buffer and in the blob.  The kernel of
// sigmaenv_snapshot.inc and the host side of sigmaenv_state_layout / _save / _restore run these functions; tests/test_snapshot_check.py compiles this header alone and
// holds it to the numpy twin tests/snapshot_check.py.
//
// Plain C++: no HIP include and nothing else of the library.  The library compiles it as __host__ __device__ __forceinline__; a host program defines SIGMA_HD as
// `static inline` first and includes this header alone.
//
// STATE is every device buffer whose content at the start of a call can change a later result:
//   ids 0 .. 20   the 21 SIGMAENV_BUF_* of sigmaenv_get, in that order (shapes: include/sigmaenv.h)
//   id 21         reset_mask  u64 [B]      per-agent reset requests of the stand-alone reset launches
//   id 22         reset_full  u8  [B]
//   id 23         fresh       u8  [B,N]    only with SIGMAENV_OBS_BOUNDARY_POINTS: agents re-placed since their last step (their boundary points)
//   id 24         cbf_groups  i32 [B,N]    only when CBF tables are attached with is_grouping: the partition the first sigmaenv_cbf_qp formed (use_fixed_groups)
// and two host words of the handle: observe_calls (the salt of the next stand-alone observation's sensor noise) and cbf_groups_valid.
// Of the CBF module nothing else carries over from one sigmaenv_cbf_qp / sigmaenv_cbf_rewards call to the next: cbf_cxy / cbf_u / cbf_kin / cbf_clf / cbf_safe are
// written by a call before it reads them, cbf_cand_big is a per-call candidate list, and cbf_defer is all zero between calls (the lean launch sets a byte, the
// full-layout launch of the same call clears it).  SIGMAENV_BUF_CBF_NOMINAL and the margin columns of SIGMAENV_BUF_REWARD_INFO are among the 21.
// NOT state: scratch and staging (the reset entries, wrap_ws, learn_minmax, episode_ws), the timing pools, the map and CBF tables (functions of the configuration),
// and the caller's settings -- the slab pointer and the rollout strides, the observation record, an attached evaluator or bank, the lanelet and scenario lists.
//
// A SEGMENT is one buffer: [blocks][B][w] bytes with w = bytes per env, `blocks` outer blocks (1 for every [B, ...] buffer, 12 for SIGMAENV_BUF_REWARD_INFO
// [12, B, N]) and block_stride = B * w bytes between them.  The blob holds the segment's bytes in the same order at `offset`, a multiple of 16; segments follow each
// other in id order, each padded to 16 bytes (save writes zeros into the padding: two snapshots of equal state are equal blobs); `total` ends the last one.
//
// The copy grid is flat over PIECES of 16 bytes; a segment whose w is no multiple of 16 is moved in pieces of 4 bytes, or of 1 byte when w is no multiple of 4
// either, so that a piece never straddles two envs (the masked restore writes whole pieces or nothing).  Every segment takes a whole number of workgroups of
// SNAP_BLOCK lanes: wg_first[s] .. wg_first[s + 1]; a workgroup finds its segment with a scan of wg_first, a lane its piece q = (wg - wg_first[s]) * SNAP_BLOCK + lane
// (q >= pieces[s]: nothing to do), then
//   block = q / (B * ppe),  r = q - block * (B * ppe),  env = r / ppe,  c = r - env * ppe          ppe = w / piece bytes                                snap_locate
//   live byte offset = block * block_stride + env * w + c * piece;   blob byte offset = offset + q * piece
// The two divisions use the multipliers m = ceil(2^32 / d) of sigmaenv_device.h's fdiv where x * d < 2^32 holds for every x the segment can present (snap_magic
// decides that on the host and stores 0 otherwise: the lane then divides plainly).
#ifndef SIGMAENV_SNAPSHOT_H
#define SIGMAENV_SNAPSHOT_H
#include <stdint.h>

#ifndef SIGMA_HD
#define SIGMA_HD __host__ __device__ __forceinline__
#endif

#define SNAP_MAGIC 0x50414E53u /* "SNAP" */
#define SNAP_VERSION 1u        /* the layout below: a change of the segment list, of a width or of the padding raises it */
#define SNAP_MAX_SEGMENTS 32
#define SNAP_BLOCK 256         /* lanes of a workgroup of the copy kernel */
#define SNAP_N_BUF 21          /* SIGMAENV_BUF_COUNT */
#define SNAP_ID_RESET_MASK 21
#define SNAP_ID_RESET_FULL 22
#define SNAP_ID_FRESH 23
#define SNAP_ID_CBF_GROUPS 24
#define SNAP_OBS_BOUNDARY_POINTS 64 /* SIGMAENV_OBS_BOUNDARY_POINTS */
#define SNAP_CBF_NONE 0             /* the `cbf` quantity: no tables attached, */
#define SNAP_CBF_ATTACHED 1         /* attached, */
#define SNAP_CBF_GROUPED 2          /* attached with is_grouping (cbf_groups exists) */
#define SNAP_BUF_REWARD_INFO 14
#define SNAP_N_REWARD_INFO 12

// one segment as the documents and the tests read it
struct SnapSegment {
  int32_t id;
  int32_t elem;           // bytes of one element: 1, 4 or 8
  uint64_t w;             // bytes per env
  int32_t blocks;         // outer blocks
  uint64_t block_stride;  // bytes between them in the live buffer
  uint64_t offset;        // in the blob
};
struct SnapLayout {
  int32_t n;
  SnapSegment seg[SNAP_MAX_SEGMENTS];
  uint64_t total;
};

// the kernel's argument: the same table as a struct of arrays, with the piece arithmetic's constants
struct SnapTable {
  int32_t n, B;
  uint32_t wg_first[SNAP_MAX_SEGMENTS + 1];  // first workgroup of each segment; [n] = the grid
  uint32_t pieces[SNAP_MAX_SEGMENTS];        // blocks * B * ppe
  uint32_t ppe[SNAP_MAX_SEGMENTS], m_ppe[SNAP_MAX_SEGMENTS];  // pieces per env and its multiplier (0: divide)
  uint32_t ppb[SNAP_MAX_SEGMENTS], m_ppb[SNAP_MAX_SEGMENTS];  // pieces per block = B * ppe and its multiplier
  uint32_t piece[SNAP_MAX_SEGMENTS];         // bytes of a piece: 16, 4 or 1
  uint32_t w[SNAP_MAX_SEGMENTS];             // bytes per env
  uint64_t block_stride[SNAP_MAX_SEGMENTS];
  uint64_t offset[SNAP_MAX_SEGMENTS];
  void* live[SNAP_MAX_SEGMENTS];             // the handle's buffers (filled by the caller of snap_table)
};
static_assert(sizeof(SnapTable) <= 2048, "the segment table travels as a kernel argument");

static inline uint64_t snap_up16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }

// bytes per env of the 21 SIGMAENV_BUF_* (include/sigmaenv.h) and their element sizes
static inline void snap_buf_width(int id, int N, int K, int D, int n_short, uint64_t* w, int* elem) {
  const uint64_t n = (uint64_t)N;
  switch (id) {
    case 0: *w = n * 32; *elem = 4; break;            // STATE f32 [B,N,8]
    case 1: *w = n * 8; *elem = 4; break;             // PREV_POS f32 [B,N,2]
    case 2: *w = n * 40; *elem = 4; break;            // VERTICES f32 [B,N,5,2]
    case 3: *w = n * 16; *elem = 4; break;            // PATH i32 [B,N,4]
    case 4: *w = n * (uint64_t)n_short * 8; *elem = 4; break;  // SHORT_TERM f32 [B,N,n_short_term,2]
    case 5: *w = n * 4; *elem = 4; break;             // DIST_REF f32 [B,N]
    case 6: *w = n * 20; *elem = 4; break;            // DIST_LEFT f32 [B,N,5]
    case 7: *w = n * 20; *elem = 4; break;            // DIST_RIGHT
    case 8: *w = n * 4; *elem = 4; break;             // DIST_BOUND f32 [B,N]
    case 9: *w = n * 12; *elem = 4; break;            // CLOSEST i32 [B,N,3]
    case 10: *w = n * n * 4; *elem = 4; break;        // DIST_AGENTS f32 [B,N,N]
    case 11: *w = n * n; *elem = 1; break;            // COL_AGENTS u8 [B,N,N]
    case 12: *w = n * 4; *elem = 1; break;            // COL_FLAGS u8 [B,N,4]
    case 13: *w = n * 4; *elem = 4; break;            // REWARD f32 [B,N]
    case 14: *w = n * 4; *elem = 4; break;            // REWARD_INFO f32 [12,B,N]: per block
    case 15: *w = n * (uint64_t)D * 4; *elem = 4; break;  // OBS f32 [B,N,D]
    case 16: *w = n * (uint64_t)K * 4; *elem = 4; break;  // NEARING i32 [B,N,K]
    case 17: *w = 1; *elem = 1; break;                // DONE u8 [B]
    case 18: *w = 16; *elem = 4; break;               // TIMER i32 [B,4]
    case 19: *w = n * 8; *elem = 4; break;            // ACTION f32 [B,N,2]
    default: *w = n * 8; *elem = 4; break;            // CBF_NOMINAL f32 [B,N,2]
  }
}

// the segment table of (B, N, K, D, n_short_term, obs_flags, cbf)
static inline void snap_layout(int B, int N, int K, int D, int n_short, int obs_flags, int cbf, SnapLayout* L) {
  uint64_t at = 0;
  L->n = 0;
  auto add = [&](int id, int elem, uint64_t w, int blocks) {
    if (w == 0) return;  // (n_nearing = 0: SIGMAENV_BUF_NEARING is empty)
    SnapSegment& s = L->seg[L->n++];
    s.id = id; s.elem = elem; s.w = w; s.blocks = blocks; s.block_stride = (uint64_t)B * w; s.offset = at;
    at = snap_up16(at + (uint64_t)blocks * B * w);
  };
  for (int id = 0; id < SNAP_N_BUF; ++id) {
    uint64_t w; int elem;
    snap_buf_width(id, N, K, D, n_short, &w, &elem);
    add(id, elem, w, id == SNAP_BUF_REWARD_INFO ? SNAP_N_REWARD_INFO : 1);
  }
  add(SNAP_ID_RESET_MASK, 8, 8, 1);
  add(SNAP_ID_RESET_FULL, 1, 1, 1);
  if (obs_flags & SNAP_OBS_BOUNDARY_POINTS) add(SNAP_ID_FRESH, 1, (uint64_t)N, 1);
  if (cbf == SNAP_CBF_GROUPED) add(SNAP_ID_CBF_GROUPS, 4, (uint64_t)N * 4, 1);
  L->total = at;
}

static inline uint32_t snap_piece_bytes(uint64_t w) { return w % 16 == 0 ? 16u : (w % 4 == 0 ? 4u : 1u); }
// ceil(2^32 / d) when x * d < 2^32 for every x <= x_max (the quotient by multiplication is then exact), else 0: divide
static inline uint32_t snap_magic(uint64_t d, uint64_t x_max) {
  if (d <= 1u || x_max * d >= (1ull << 32)) return 0u;
  return (uint32_t)(((1ull << 32) + d - 1u) / d);
}
// the kernel's form of the layout (live[] stays for the caller); returns 0, or -1 when a segment has more than 2^32 - 1 pieces
static inline int snap_table(const SnapLayout& L, int B, SnapTable* T) {
  T->n = L.n; T->B = B;
  uint64_t wg = 0;
  for (int s = 0; s < L.n; ++s) {
    const SnapSegment& g = L.seg[s];
    const uint32_t piece = snap_piece_bytes(g.w);
    const uint64_t ppe = g.w / piece, ppb = ppe * (uint64_t)B, pieces = ppb * (uint64_t)g.blocks;
    if (pieces >= (1ull << 32) - SNAP_BLOCK) return -1;
    T->wg_first[s] = (uint32_t)wg;
    T->pieces[s] = (uint32_t)pieces;
    T->ppe[s] = (uint32_t)ppe; T->m_ppe[s] = snap_magic(ppe, ppb - 1);
    T->ppb[s] = (uint32_t)ppb; T->m_ppb[s] = snap_magic(ppb, pieces - 1);
    T->piece[s] = piece; T->w[s] = (uint32_t)g.w;
    T->block_stride[s] = g.block_stride; T->offset[s] = g.offset;
    T->live[s] = nullptr;
    wg += (pieces + SNAP_BLOCK - 1) / SNAP_BLOCK;
    if (wg >= (1ull << 31)) return -1;
  }
  for (int s = L.n; s <= SNAP_MAX_SEGMENTS; ++s) T->wg_first[s] = (uint32_t)wg;
  return 0;
}

// x / d with d's multiplier m (0: the plain division)
SIGMA_HD uint32_t snap_div(uint32_t x, uint32_t d, uint32_t m) { return m ? (uint32_t)(((uint64_t)x * m) >> 32) : x / d; }
// the segment of workgroup wg
SIGMA_HD int snap_segment_of(const SnapTable& T, uint32_t wg) {
  int s = 0;
  while (s + 1 < T.n && wg >= T.wg_first[s + 1]) ++s;
  return s;
}
// bytes between the end of segment s in the blob and the next multiple of 16 (0 .. 15): save writes zeros there, restore never reads them
SIGMA_HD uint32_t snap_padding(const SnapTable& T, int s) { return (uint32_t)((0u - (T.offset[s] + (uint64_t)T.pieces[s] * T.piece[s])) & 15u); }
struct SnapPiece {
  uint32_t block, env;
  uint64_t live_off, blob_off;
};
// piece q < pieces[s] of segment s
SIGMA_HD SnapPiece snap_locate(const SnapTable& T, int s, uint32_t q) {
  SnapPiece p;
  p.block = T.pieces[s] == T.ppb[s] ? 0u : snap_div(q, T.ppb[s], T.m_ppb[s]);  // (one block: every [B, ...] buffer)
  const uint32_t r = q - p.block * T.ppb[s];
  p.env = snap_div(r, T.ppe[s], T.m_ppe[s]);
  const uint32_t c = r - p.env * T.ppe[s];
  p.live_off = (uint64_t)p.block * T.block_stride[s] + (uint64_t)p.env * T.w[s] + (uint64_t)c * T.piece[s];
  p.blob_off = T.offset[s] + (uint64_t)q * T.piece[s];
  return p;
}
#endif  // SIGMAENV_SNAPSHOT_H
