"""The yardstick of the env snapshot (sigmarl_amd/csrc/sigmaenv_snapshot.h; the contract: include/sigmaenv.h, sigmaenv_state_*) -- no GPU and no pytest here: a plain
numpy statement of the segment table, of the piece arithmetic of the copy grid, and of save / restore / masked restore over plain byte arrays.
tests/test_snapshot_check.py holds the header compiled alone to it number for number; tests/test_gpu_snapshot.py holds the kernel to the same words.

Everything is Python integers (exact): the header's multiplier divisions must give what `//` gives.  ``defect=`` plants one of ``DEFECTS`` in this copy of the
arithmetic; every one of them must fail a named check of tests/test_snapshot_check.py."""
import numpy as np

MAGIC, VERSION = 0x50414E53, 1
BLOCK = 256  # SNAP_BLOCK
N_BUF = 21
ID_RESET_MASK, ID_RESET_FULL, ID_FRESH, ID_CBF_GROUPS = 21, 22, 23, 24
BUF_REWARD_INFO, N_REWARD_INFO = 14, 12
OBS_BOUNDARY_POINTS = 64
CBF_NONE, CBF_ATTACHED, CBF_GROUPED = 0, 1, 2

DEFECTS = ("segment_left_out", "reward_info_stride_n", "mask_by_piece", "odd_width_rounded_down", "host_words_under_mask", "total_off_by_one")


def up16(v):
    return (v + 15) & ~15


def buf_width(i, N, K, D, NS):
    """(bytes per env, element bytes) of SIGMAENV_BUF_* i (include/sigmaenv.h)"""
    return {0: (N * 32, 4), 1: (N * 8, 4), 2: (N * 40, 4), 3: (N * 16, 4), 4: (N * NS * 8, 4), 5: (N * 4, 4), 6: (N * 20, 4), 7: (N * 20, 4), 8: (N * 4, 4),
            9: (N * 12, 4), 10: (N * N * 4, 4), 11: (N * N, 1), 12: (N * 4, 1), 13: (N * 4, 4), 14: (N * 4, 4), 15: (N * D * 4, 4), 16: (N * K * 4, 4), 17: (1, 1),
            18: (16, 4), 19: (N * 8, 4), 20: (N * 8, 4)}[i]


def layout(B, N, K, D, NS, obs_flags, cbf, defect=None):
    """The segment table: a list of dicts (id, elem, w, blocks, block_stride, offset) and the total."""
    assert defect is None or defect in DEFECTS
    segs, at = [], 0

    def add(i, elem, w, blocks):
        nonlocal at
        if w == 0:
            return
        stride = B * w
        if defect == "reward_info_stride_n" and i == BUF_REWARD_INFO:
            stride = w  # [12, B, N] read as if the blocks were N elements apart
        segs.append(dict(id=i, elem=elem, w=w, blocks=blocks, block_stride=stride, offset=at))
        at = up16(at + blocks * B * w)

    for i in range(N_BUF):
        w, elem = buf_width(i, N, K, D, NS)
        add(i, elem, w, N_REWARD_INFO if i == BUF_REWARD_INFO else 1)
    add(ID_RESET_MASK, 8, 8, 1)
    if defect != "segment_left_out":
        add(ID_RESET_FULL, 1, 1, 1)
    if obs_flags & OBS_BOUNDARY_POINTS:
        add(ID_FRESH, 1, N, 1)
    if cbf == CBF_GROUPED:
        add(ID_CBF_GROUPS, 4, N * 4, 1)
    return segs, at + (1 if defect == "total_off_by_one" else 0)


def piece_bytes(w, defect=None):
    if defect == "odd_width_rounded_down":
        return 16 if w % 16 == 0 else 4  # never 1: a width that is no multiple of 4 loses its tail
    return 16 if w % 16 == 0 else (4 if w % 4 == 0 else 1)


def magic(d, x_max):
    """ceil(2^32 / d) where the multiplication is exact for every x <= x_max, else 0 (the lane divides)"""
    return 0 if d <= 1 or x_max * d >= 1 << 32 else ((1 << 32) + d - 1) // d


def table(segs, B, defect=None):
    """The kernel's constants per segment: piece, ppe, ppb, pieces, the two multipliers, wg_first; and the grid."""
    rows, wg = [], 0
    for g in segs:
        piece = piece_bytes(g["w"], defect)
        ppe = g["w"] // piece
        ppb = ppe * B
        pieces = ppb * g["blocks"]
        rows.append(dict(piece=piece, ppe=ppe, ppb=ppb, pieces=pieces, m_ppe=magic(ppe, ppb - 1), m_ppb=magic(ppb, pieces - 1), wg_first=wg))
        wg += (pieces + BLOCK - 1) // BLOCK
    return rows, wg


def padding(g, r):
    """bytes between the segment's end in the blob and the next multiple of 16: save writes zeros there (the blob is a function of the state alone)"""
    return -(g["offset"] + r["pieces"] * r["piece"]) % 16


def segment_of(rows, grid, wg):
    s = 0
    while s + 1 < len(rows) and wg >= rows[s + 1]["wg_first"]:
        s += 1
    return s


def locate(segs, rows, s, q):
    """(block, env, live byte offset, blob byte offset) of pieces q (an integer array) of segment s"""
    g, r = segs[s], rows[s]
    q = np.asarray(q, np.int64)
    block = q // r["ppb"]
    rem = q - block * r["ppb"]
    env = rem // r["ppe"]
    c = rem - env * r["ppe"]
    return block, env, block * g["block_stride"] + env * g["w"] + c * r["piece"], g["offset"] + q * r["piece"]


def enumerate_pieces(segs, rows, grid):
    """Every (workgroup, lane) of the flat grid -> per segment the arrays of locate, in grid order: what the kernel's lanes compute"""
    out = []
    for s, r in enumerate(rows):
        wg_end = rows[s + 1]["wg_first"] if s + 1 < len(rows) else grid
        lanes = (np.arange(r["wg_first"], wg_end, dtype=np.int64)[:, None] * BLOCK + np.arange(BLOCK, dtype=np.int64)[None, :]).reshape(-1)
        q = lanes - r["wg_first"] * BLOCK
        q = q[q < r["pieces"]]
        out.append((q,) + locate(segs, rows, s, q))
    return out


def coverage(segs, rows, grid, B, total):
    """How often each byte of every live buffer and of the blob is touched by the grid: (list of per-segment count arrays, blob count array)"""
    blob = np.zeros(max(total, max((g["offset"] + g["blocks"] * B * g["w"] for g in segs), default=0)) + 64, np.int32)
    live = []
    for (q, block, env, lo, bo), g, r in zip(enumerate_pieces(segs, rows, grid), segs, rows):
        cnt = np.zeros(g["blocks"] * B * g["w"] + 64, np.int32)
        j = np.arange(r["piece"], dtype=np.int64)[None, :]
        lo_b, bo_b = (lo[:, None] + j).reshape(-1), (bo[:, None] + j).reshape(-1)
        lo_b = lo_b[(lo_b >= 0) & (lo_b < cnt.size)]
        np.add.at(cnt, lo_b, 1)
        np.add.at(blob, bo_b[bo_b < blob.size], 1)
        live.append(cnt)
    return live, blob


def random_buffers(segs, B, rng):
    """id -> uint8 array of the live buffer's bytes"""
    return {g["id"]: rng.integers(0, 256, g["blocks"] * B * g["w"], dtype=np.uint8) for g in segs}


class Handle:
    """The state of a handle over plain arrays: ``bufs`` (id -> bytes) and the two host words."""

    def __init__(self, shape, rng, defect=None):
        self.shape, self.defect = tuple(shape), defect  # (B, N, K, D, NS, obs_flags, cbf)
        self.B = shape[0]
        self.true_segs, self.true_total = layout(*shape)
        self.segs, self.total = layout(*shape, defect=defect)
        self.rows, self.grid = table(self.segs, self.B, defect)
        self.bufs = random_buffers(self.true_segs, self.B, rng)
        self.observe_calls, self.cbf_groups_valid = int(rng.integers(0, 100)), int(rng.integers(0, 2))

    def header(self):
        return dict(magic=MAGIC, version=VERSION, n_envs=self.shape[0], n_agents=self.shape[1], n_nearing=self.shape[2], obs_dim=self.shape[3],
                    n_short_term=self.shape[4], obs_flags=self.shape[5], cbf=self.shape[6], observe_calls=self.observe_calls,
                    cbf_groups_valid=self.cbf_groups_valid, total_bytes=self.total)

    def save(self):
        blob = np.zeros(self.total, np.uint8)
        for (q, block, env, lo, bo), g, r in zip(enumerate_pieces(self.segs, self.rows, self.grid), self.segs, self.rows):
            j = np.arange(r["piece"], dtype=np.int64)[None, :]
            blob[(bo[:, None] + j).reshape(-1)] = self.bufs[g["id"]][(lo[:, None] + j).reshape(-1)]
        return self.header(), blob

    def restore(self, header, blob, mask=None):
        """mask: None or a uint8 [B] array; pieces of envs with a zero byte are skipped, whole"""
        own = self.header()
        for k in ("magic", "version", "n_envs", "n_agents", "n_nearing", "obs_dim", "n_short_term", "obs_flags", "cbf", "total_bytes"):
            if header[k] != own[k]:
                raise ValueError(f"state_restore: the header's {k} is {header[k]}, the handle's {own[k]}")
        if blob.size != self.total:
            raise ValueError("state_restore: bytes")
        for (q, block, env, lo, bo), g, r in zip(enumerate_pieces(self.segs, self.rows, self.grid), self.segs, self.rows):
            if mask is not None:
                key = np.minimum(q, self.B - 1) if self.defect == "mask_by_piece" else env
                keep = np.asarray(mask)[key] != 0
                lo, bo = lo[keep], bo[keep]
            j = np.arange(r["piece"], dtype=np.int64)[None, :]
            self.bufs[g["id"]][(lo[:, None] + j).reshape(-1)] = blob[(bo[:, None] + j).reshape(-1)]
        if mask is None or self.defect == "host_words_under_mask":
            self.observe_calls, self.cbf_groups_valid = header["observe_calls"], header["cbf_groups_valid"]

    def env_bytes(self, i, envs):
        """the bytes of buffer i that belong to the envs `envs` (a bool [B] array), by the true layout"""
        g = [x for x in self.true_segs if x["id"] == i][0]
        return self.bufs[i].reshape(g["blocks"], self.B, g["w"])[:, np.asarray(envs, bool), :]
