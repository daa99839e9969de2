// sigmaenv_snapshot.inc -- snapshot and restore of an env handle's state (include/sigmaenv.h: sigmaenv_state_layout / _save / _restore).  The segment table, the piece
// arithmetic and the list of what is and is not state: sigmaenv_snapshot.h.  ONE kernel, a template over the direction; no atomics, no LDS; a masked-out lane of the
// restore issues no store.  Included at the end of sigmaenv.hip.

namespace snap {

template <int BYTES> struct PieceT;
template <> struct PieceT<16> { typedef uint4 type; };
template <> struct PieceT<4> { typedef uint32_t type; };
template <> struct PieceT<1> { typedef uint8_t type; };

template <int BYTES>
__device__ __forceinline__ void move_piece(char* dst, const char* src) {
  typedef typename PieceT<BYTES>::type V;
  *reinterpret_cast<V*>(dst) = *reinterpret_cast<const V*>(src);
}

// SAVE: live -> blob.  !SAVE: blob -> live, for the envs with a non-zero mask byte (mask == nullptr: all).  The grid is T.wg_first[T.n] workgroups of SNAP_BLOCK lanes.
template <bool SAVE>
__global__ void __launch_bounds__(SNAP_BLOCK) sigmaenv_snapshot_kernel(SnapTable T, char* __restrict__ blob, const uint8_t* __restrict__ mask) {
  const int s = snap_segment_of(T, blockIdx.x);  // the same for the whole workgroup
  const uint32_t q = (blockIdx.x - T.wg_first[s]) * SNAP_BLOCK + threadIdx.x;
  if (q >= T.pieces[s]) return;
  const SnapPiece p = snap_locate(T, s, q);
  if (!SAVE && mask != nullptr && mask[p.env] == 0) return;  // (indexed per lane: a vector load) -- no store at all for an env left out
  char* live = static_cast<char*>(T.live[s]) + p.live_off;
  char* in_blob = blob + p.blob_off;
  char* dst = SAVE ? in_blob : live;
  const char* src = SAVE ? live : in_blob;
  const uint32_t piece = T.piece[s];
  if (piece == 16u) move_piece<16>(dst, src);
  else if (piece == 4u) move_piece<4>(dst, src);
  else move_piece<1>(dst, src);
  if (SAVE && q + 1u == T.pieces[s]) {  // the lane of the segment's last piece zeroes the padding behind it: the blob is a function of the state alone
    char* end = in_blob + piece;
    for (uint32_t k = 0, n = snap_padding(T, s); k < n; ++k) end[k] = 0;
  }
}

}  // namespace snap

static int snap_cbf_quantity(const sigmaenv* h) { return !h->cbf_seg4 ? SNAP_CBF_NONE : (h->cbf_groups ? SNAP_CBF_GROUPED : SNAP_CBF_ATTACHED); }

// the handle's table with its live pointers
static int snap_handle_table(sigmaenv* h, SnapLayout* L, SnapTable* T) {
  snap_layout(h->B, h->N, h->K, h->D, NS, h->cfg.obs_flags, snap_cbf_quantity(h), L);
  if (snap_table(*L, h->B, T) != 0) { h->err = "state: a buffer has more pieces than the copy grid can index"; return SIGMAENV_EINVAL; }
  for (int s = 0; s < L->n; ++s) {
    const int id = L->seg[s].id;
    void* p = id < SIGMAENV_BUF_COUNT ? h->bufs[id]
              : id == SNAP_ID_RESET_MASK ? (void*)h->buf.reset_mask
              : id == SNAP_ID_RESET_FULL ? (void*)h->buf.reset_full
              : id == SNAP_ID_FRESH ? (void*)h->buf.fresh
                                    : (void*)h->cbf_groups;
    if (!p) { h->err = "state: a buffer of the layout is not allocated"; return SIGMAENV_EINVAL; }
    T->live[s] = p;
  }
  return SIGMAENV_OK;
}

static void snap_fill_header(const sigmaenv* h, const SnapLayout& L, sigmaenv_state_header_t* out) {
  memset(out, 0, sizeof(*out));
  out->magic = SNAP_MAGIC;
  out->version = SNAP_VERSION;
  out->n_envs = h->B; out->n_agents = h->N; out->n_nearing = h->K; out->obs_dim = h->D; out->n_short_term = NS;
  out->obs_flags = h->cfg.obs_flags;
  out->cbf = snap_cbf_quantity(h);
  out->observe_calls = h->observe_calls;
  out->cbf_groups_valid = h->cbf_groups_valid ? 1u : 0u;
  out->total_bytes = L.total;
}

extern "C" int sigmaenv_state_layout(sigmaenv_t* h, sigmaenv_state_header_t* out) {
  if (!h) return SIGMAENV_EINVAL;
  if (!out) { h->err = "state_layout: null header"; return SIGMAENV_EINVAL; }
  SnapLayout L;
  snap_layout(h->B, h->N, h->K, h->D, NS, h->cfg.obs_flags, snap_cbf_quantity(h), &L);
  snap_fill_header(h, L, out);
  return SIGMAENV_OK;
}

static int snap_check_blob(sigmaenv* h, const char* what, const void* blob, size_t bytes, const SnapLayout& L) {
  if (!blob) { h->err = std::string(what) + ": null blob"; return SIGMAENV_EINVAL; }
  if (reinterpret_cast<uintptr_t>(blob) % 16 != 0) { h->err = std::string(what) + ": the blob is not 16-byte aligned"; return SIGMAENV_EINVAL; }
  if ((uint64_t)bytes != L.total) {
    h->err = std::string(what) + ": bytes = " + std::to_string(bytes) + ", the layout's total is " + std::to_string(L.total);
    return SIGMAENV_EINVAL;
  }
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_state_save(sigmaenv_t* h, void* dev_blob, size_t bytes) {
  if (!h) return SIGMAENV_EINVAL;
  SnapLayout L;
  SnapTable T;
  int rc = snap_handle_table(h, &L, &T);
  if (rc) return rc;
  if ((rc = snap_check_blob(h, "state_save", dev_blob, bytes, L)) != SIGMAENV_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(snap::sigmaenv_snapshot_kernel<true>, dim3(T.wg_first[T.n]), dim3(SNAP_BLOCK), 0, h->stream, T, static_cast<char*>(dev_blob), (const uint8_t*)nullptr);
  HIPCHK(h, hipGetLastError());
  return SIGMAENV_OK;
}

extern "C" int sigmaenv_state_restore(sigmaenv_t* h, const sigmaenv_state_header_t* hdr, const void* dev_blob, size_t bytes, const uint8_t* env_mask) {
  if (!h) return SIGMAENV_EINVAL;
  if (!hdr) { h->err = "state_restore: null header"; return SIGMAENV_EINVAL; }
  SnapLayout L;
  SnapTable T;
  int rc = snap_handle_table(h, &L, &T);
  if (rc) return rc;
  sigmaenv_state_header_t own;
  snap_fill_header(h, L, &own);
  const struct { const char* name; long long got, want; } fields[] = {
      {"magic", (long long)hdr->magic, (long long)own.magic}, {"version", (long long)hdr->version, (long long)own.version},
      {"n_envs", hdr->n_envs, own.n_envs}, {"n_agents", hdr->n_agents, own.n_agents}, {"n_nearing", hdr->n_nearing, own.n_nearing},
      {"obs_dim", hdr->obs_dim, own.obs_dim}, {"n_short_term", hdr->n_short_term, own.n_short_term}, {"obs_flags", hdr->obs_flags, own.obs_flags},
      {"cbf", hdr->cbf, own.cbf}, {"total_bytes", (long long)hdr->total_bytes, (long long)own.total_bytes},
  };
  for (const auto& f : fields) {
    if (f.got != f.want) {
      h->err = std::string("state_restore: the header's ") + f.name + " is " + std::to_string(f.got) + ", the handle's " + std::to_string(f.want);
      return SIGMAENV_EINVAL;
    }
  }
  if ((rc = snap_check_blob(h, "state_restore", dev_blob, bytes, L)) != SIGMAENV_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(snap::sigmaenv_snapshot_kernel<false>, dim3(T.wg_first[T.n]), dim3(SNAP_BLOCK), 0, h->stream, T,
                     const_cast<char*>(static_cast<const char*>(dev_blob)), env_mask);
  HIPCHK(h, hipGetLastError());
  if (!env_mask) {  // the whole handle goes back to the snapshot's moment: its host words too
    h->observe_calls = hdr->observe_calls;
    h->cbf_groups_valid = h->cbf_groups != nullptr && hdr->cbf_groups_valid != 0;
  }
  return SIGMAENV_OK;
}
