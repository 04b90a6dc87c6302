"""Deterministic frame records that sit on the edges of the device-side compaction, and the compact blob the
pack kernels must write for them (test helper: numpy, plus glc_amd for the host twin in the tests).

P1-P3 (k_pack_scan_rows / k_pack_scan_blocks / k_pack_rows, csrc/glc_kernels.hip) turn frame records into the
compact blob of DESIGN.md section 3.  They branch on data - a raw-flag word, an nnz field that need not agree
with its row, 64-bin ballot groups, 1024-row scan blocks whose two counts share one 32-bit word, chunks of
1024 scan blocks - and records that an encode of real audio leaves reach almost none of those edges.  A record
range is DESCRIBED here sparsely (`Desc`), `materialise` writes the dense records of that description in the
layout of glc_record_bytes, and `model` writes the blob that DESIGN.md section 3 and CompactLayout /
CompactHeader (csrc/glc_common.h) prescribe for it, from the description alone:

  header 64 B {u32 "GLCB", u32 channels, u64 n_frames, u64 n_pairs, u64 n_raw_rows, u64 bytes, 24 B zero}
  | is_raw u8[n_frames] | scale f32[M] | cnt u32[M] | pairs u32[n_pairs] | raw i16[n_raw_rows][2048]
  M = n_frames * channels, every section 64-byte aligned, all padding zero.

  a frame is raw when its whole u32 flag word is non-zero; cnt[m] = 0 for the rows of raw frames, else
  min(nnz field, 1024); the list of row m is its first cnt[m] non-zero bins below 1024 in ascending k as
  (k | u16(q) << 16), and where the row holds fewer the rest of its slot is 0x0000FFFF; bins 1024..2047 of a
  compressed row are not looked at; the planes of raw-frame rows follow the pairs in row order.

`model_batch` is the blob of a batch round (glc_encode_batch; glc_debug_compact_batch_device): a clip directory
u64[2 n_clips] between the header and the sections, which cover the REAL frames of a virtual record stream only -
clip i owns records slot_i .. slot_i + nf_i - 1, the record behind them is junk and nothing of it may show.

Families (cases()):
  counts    rows of 0 .. 1024 non-zeros in placements that load single ballot groups, their edges (bins 63 / 64)
            and every group; q at the ends of i16; scale bits that are no ordinary number
  disagree  nnz field above / below the row's true count, past 1024, non-zero on raw rows; junk in bins >= 1024
  raw       flag words that are not 1, every placement of raw frames, raw frames across a 1024-row block edge,
            planes of i16 extremes, the alignment gap in front of the raw section at 0 / 60 / 4 bytes
  blocks    row counts around one, two and four scan blocks for 1 / 3 / 8 channels, and blocks that fill the
            packed scan word: 1024 rows of 1024 pairs, 1024 raw rows, 1023 dense rows + one raw
  chunks    1024 * 1025 + 7 mono frames = 1026 scan blocks: the second chunk of k_pack_scan_blocks (never
            materialised on the host: 4.3 GB of records; the model needs the description only)
  batch     virtual streams for the batch hook: one-frame clips, clips that start at row 1023 / 1024 / 1025,
            raw first frames, all raw, a single clip, 700 clips; junk records full of pairs or flagged raw

`model(desc, mutation)` restates the packing with one rule changed (MUTATIONS): tests/test_compact_edges.py
uses it to show that the families would notice that edit of a kernel.
"""
from __future__ import annotations

import hashlib
import struct
from dataclasses import dataclass, field

import numpy as np

HOP, FRAME = 1024, 2048
BLOCK = 1024                     # rows per scan block (k_pack_scan_rows), blocks per chunk (k_pack_scan_blocks)
MAGIC = 0x42434C47               # "GLCB"
FILLER = 0x0000FFFF
SENTINEL = 0xAB
ONE = 0x3F800000                 # scale bits of rows that do not care

MUTATIONS = ("scan_inclusive", "block_carry_dropped", "chunk_carry_dropped", "raw_counted_as_pairs",
             "raw_flag_low_byte", "nnz_unclamped", "filler_missing", "keep_last_not_first", "descending_k",
             "idx_q_swapped", "upper_bins_counted", "raw_gap_unaligned", "raw_gap_not_zeroed",
             "raw_rows_by_block_not_global", "dir_off_by_one_clip", "junk_frame_counted")

NNZ_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 1023, 1024)
Q_VALUES = (1, -1, 32767, -32767, -32768)
SCALE_BITS = (0x80000000, 0x00000001, 0x7F800000, 0x7FC12345)        # -0.0, a subnormal, inf, a NaN payload
FLAG_WORDS = (1, 2, 0x100, 0x80000000)
CLAMPED_FIELDS = (1025, 0xFFFFFFFF)
RAW_CHANNELS = (3, 5, 7)
GAP_PAIRS = {16: 0, 17: 60, 31: 4}                                    # n_pairs -> bytes of gap in front of the raw section
BLOCK_CHANNELS = (1, 3, 8)
BLOCK_ROWS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
CHUNK_FRAMES = BLOCK * (BLOCK + 1) + 7                                # mono: 1026 scan blocks
CHUNK_RAW_BLOCKS = (0, 1023, 1024, 1025)
I16_EXTREMES = (-32768, -32767, -1, 0, 1, 32766, 32767)


def header_bytes(ch: int) -> int:
    return ((8 + 8 * ch) + 15) // 16 * 16


def record_bytes(ch: int) -> int:
    return header_bytes(ch) + 2 * FRAME * ch


def align64(v: int) -> int:
    return (v + 63) // 64 * 64


# ----------------------------------------------------------------------------------------------------
# the description of a record range
# ----------------------------------------------------------------------------------------------------

@dataclass
class Desc:
    """`nf` records of `ch` channels.  Entries (e_row, e_k, e_q) are the non-zero bins of compressed rows, sorted
    by (row, k), k in 0..2047; a raw frame (flags[f] != 0) has planes[f] (ch x 2048 i16) and no entries."""
    ch: int
    nf: int
    flags: np.ndarray                       # u32[nf]: the raw-flag word
    scale_bits: np.ndarray                  # u32[nf * ch]
    nnz: np.ndarray                         # u32[nf * ch]: the nnz FIELD
    e_row: np.ndarray                       # i64[E]
    e_k: np.ndarray                         # i64[E]
    e_q: np.ndarray                         # i16[E], never 0
    planes: dict = field(default_factory=dict)

    @property
    def rows(self) -> int:
        return self.nf * self.ch

    def true_counts(self) -> np.ndarray:
        """Non-zero bins below 1024 of every row of a compressed frame (0 for rows of raw frames)."""
        return np.bincount(self.e_row[self.e_k < HOP], minlength=self.rows).astype(np.int64)

    def consistent(self) -> bool:
        """Every nnz field says what its row holds (0 on the rows of raw frames): records an encode could leave."""
        return bool((self.nnz.astype(np.int64) == self.true_counts()).all())


class Builder:
    def __init__(self, ch: int, nf: int):
        self.ch, self.nf = ch, nf
        self.flags = np.zeros(nf, np.uint32)
        self.scale_bits = np.full(nf * ch, ONE, np.uint32)
        self.nnz = np.zeros(nf * ch, np.int64)
        self.field = {}
        self.r, self.k, self.q = [], [], []
        self.planes = {}

    def row(self, m, ks, qs, nnz=None, scale=None):
        ks, qs = np.asarray(ks, np.int64), np.asarray(qs, np.int16)
        assert ks.size == qs.size and (qs != 0).all() and (np.diff(ks) > 0).all() and (ks.size == 0 or 0 <= ks[0] and ks[-1] < FRAME)
        self.r.append(np.full(ks.size, m, np.int64)), self.k.append(ks), self.q.append(qs)
        self.nnz[m] += int((ks < HOP).sum())
        if nnz is not None:
            self.field[m] = nnz
        if scale is not None:
            self.scale_bits[m] = scale

    def raw(self, f, flag, planes, nnz=None):
        planes = np.asarray(planes, np.int16)
        assert flag != 0 and planes.shape == (self.ch, FRAME)
        self.flags[f] = flag
        self.planes[f] = planes
        if nnz is not None:
            for c in range(self.ch):
                self.field[f * self.ch + c] = nnz

    def desc(self) -> Desc:
        cat = lambda v, t: np.concatenate(v).astype(t) if v else np.zeros(0, t)
        r, k, q = cat(self.r, np.int64), cat(self.k, np.int64), cat(self.q, np.int16)
        o = np.lexsort((k, r))
        r, k, q = r[o], k[o], q[o]
        assert not ((np.diff(r) == 0) & (np.diff(k) == 0)).any(), "a bin given twice"
        nnz = self.nnz.copy()
        for m, v in self.field.items():
            nnz[m] = v
        assert not (self.flags[r // self.ch] != 0).any(), "entries on a raw frame"
        return Desc(self.ch, self.nf, self.flags, self.scale_bits, nnz.astype(np.uint32), r, k, q, self.planes)


def take_frames(d: Desc, frames) -> Desc:
    """The description of the records `frames` (ascending indices into d) as a range of their own."""
    frames = np.asarray(frames, np.int64)
    assert (np.diff(frames) > 0).all()
    ch = d.ch
    new = np.full(d.nf + 1, -1, np.int64)
    new[frames] = np.arange(frames.size)
    to = new[d.e_row // ch]
    keep = to >= 0
    rows = (frames[:, None] * ch + np.arange(ch)[None, :]).reshape(-1)
    return Desc(ch, int(frames.size), d.flags[frames], d.scale_bits[rows], d.nnz[rows],
                to[keep] * ch + d.e_row[keep] % ch, d.e_k[keep], d.e_q[keep],
                {int(new[f]): p for f, p in d.planes.items() if new[f] >= 0})


def materialise(d: Desc) -> np.ndarray:
    """Dense records, uint8 [nf, record_bytes(ch)]: u32 flag | u32 0 | ch x {scale, nnz} | pad | i16 [ch][2048]."""
    ch, hdr, rec = d.ch, header_bytes(d.ch), record_bytes(d.ch)
    out = np.zeros((d.nf, rec), np.uint8)
    w = out.view(np.uint32)
    w[:, 0] = d.flags
    w[:, 2:2 + 2 * ch:2] = d.scale_bits.reshape(d.nf, ch)
    w[:, 3:3 + 2 * ch:2] = d.nnz.reshape(d.nf, ch)
    h = out.view(np.int16)
    h[d.e_row // ch, hdr // 2 + (d.e_row % ch) * FRAME + d.e_k] = d.e_q
    for f, p in d.planes.items():
        h[f, hdr // 2:] = p.reshape(-1)
    return out


def materialise_torch(d: Desc, torch, device="cuda"):
    """The same records built on the device: zero fill plus indexed stores of the description's few entries
    (int16 tensor [nf, record_bytes / 2]); for ranges whose dense image does not belong on the host."""
    ch, hdr, rec = d.ch, header_bytes(d.ch), record_bytes(d.ch)
    t = torch.zeros((d.nf, rec // 2), dtype=torch.int16, device=device)
    w = t.view(torch.int32)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize
                                         else np.ascontiguousarray(a).astype(dt)).to(device)
    w[:, 0] = dev(d.flags, np.int32)
    w[:, 2:2 + 2 * ch:2] = dev(d.scale_bits, np.int32).view(d.nf, ch)
    w[:, 3:3 + 2 * ch:2] = dev(d.nnz, np.int32).view(d.nf, ch)
    slab = (1 << 30) // (rec // 2)                       # frames per indexed store: fewer than 2^31 elements under it
    for lo in range(0, d.nf, slab):
        a, b = np.searchsorted(d.e_row, [lo * ch, min(lo + slab, d.nf) * ch])
        r = d.e_row[a:b]
        t[lo:lo + slab][dev(r // ch - lo, np.int64), dev(hdr // 2 + (r % ch) * FRAME + d.e_k[a:b], np.int64)] = dev(d.e_q[a:b], np.int16)
    for f, p in d.planes.items():
        t[f, hdr // 2:] = dev(p.reshape(-1), np.int16)
    return t


# ----------------------------------------------------------------------------------------------------
# the blob a description must become, with optional mutations
# ----------------------------------------------------------------------------------------------------

def _content(d: Desc, raw_f: np.ndarray, with_raw_rows: bool):
    """(row, k, q) of every non-zero bin that the packing may look at, sorted by (row, k): the entries, and the
    planes of frames that a mutated rule does not treat as raw."""
    extra = [f for f in d.planes if with_raw_rows or not raw_f[f]]
    if not extra:
        return d.e_row, d.e_k, d.e_q
    r, k, q = [d.e_row], [d.e_k], [d.e_q]
    for f in extra:
        c, kk = np.nonzero(d.planes[f])
        r.append(f * d.ch + c), k.append(kk), q.append(d.planes[f][c, kk])
    r, k, q = np.concatenate(r), np.concatenate(k), np.concatenate(q)
    o = np.lexsort((k, r))
    return r[o], k[o], q[o]


def _restart(excl: np.ndarray, mut) -> np.ndarray:
    """Per-row exclusive offsets under the scan mutations that lose a carry."""
    m = np.arange(excl.size)
    if mut == "block_carry_dropped":
        return excl - excl[m // BLOCK * BLOCK]
    if mut == "chunk_carry_dropped" and excl.size > BLOCK * BLOCK:
        return excl - np.where(m >= BLOCK * BLOCK, excl[BLOCK * BLOCK], 0)
    return excl


def _pack(d: Desc, mut=None, clip_first_frames=None):
    ch, nf, M = d.ch, d.nf, d.rows
    raw_f = (d.flags & 0xFF) != 0 if mut == "raw_flag_low_byte" else d.flags != 0
    raw_row = np.repeat(raw_f, ch)
    fld = d.nnz.astype(np.int64)
    clamped = np.minimum(fld, HOP)
    cnt = clamped.copy() if mut == "raw_counted_as_pairs" else np.where(raw_row, 0, clamped)
    r, k, q = _content(d, raw_f, mut == "raw_counted_as_pairs")
    sel = k < (FRAME if mut == "upper_bins_counted" else HOP)
    r, k, q = r[sel], k[sel], q[sel]
    have = np.bincount(r, minlength=M)
    rank = np.arange(r.size) - np.searchsorted(r, r, "left")
    if mut == "keep_last_not_first":
        rank = rank - np.maximum(have - cnt, 0)[r]
    kept = np.minimum(have, cnt)
    keep = (rank >= 0) & (rank < cnt[r])
    r, k, q, rank = r[keep], k[keep], q[keep], rank[keep]
    excl = np.cumsum(cnt) - cnt
    n_pairs = int(cnt.sum())
    off = _restart(excl, mut) + (cnt if mut == "scan_inclusive" else 0)
    pairs = np.full(n_pairs, 0xABABABAB if mut == "filler_missing" else FILLER, np.uint32)
    pos = off[r] + (kept[r] - 1 - rank if mut == "descending_k" else rank)
    u = q.astype(np.int64) & 0xFFFF
    word = (u | k << 16) if mut == "idx_q_swapped" else (k | u << 16)
    ok = pos < n_pairs
    pairs[pos[ok]] = word[ok].astype(np.uint32)

    rr_excl = np.cumsum(raw_row) - raw_row
    rr = _restart(rr_excl, "block_carry_dropped" if mut == "raw_rows_by_block_not_global" else mut)
    n_raw = int(raw_row.sum())
    rawsec = np.full((n_raw, FRAME), np.int16(-21589), np.int16)         # 0xABAB: a plane nobody wrote
    for f in np.flatnonzero(raw_f):
        p = d.planes.get(int(f))
        if p is None:                       # only a mutated rule calls a frame without planes raw: its dense rows
            p = np.zeros((ch, FRAME), np.int16)
            s = (d.e_row // ch) == f
            p[d.e_row[s] % ch, d.e_k[s]] = d.e_q[s]
        rawsec[rr[f * ch:(f + 1) * ch]] = p

    n_clips = 0 if clip_first_frames is None else len(clip_first_frames)
    o_dir = 64
    o_israw = o_dir + align64(16 * n_clips)
    o_scale = o_israw + align64(nf)
    o_cnt = o_scale + align64(4 * M)
    o_pairs = o_cnt + align64(4 * M)
    pairs_end = o_pairs + 4 * n_pairs
    raw_off = pairs_end if mut == "raw_gap_unaligned" else align64(pairs_end)
    total = raw_off + 2 * FRAME * n_raw
    blob = np.zeros(total, np.uint8)
    blob[:64] = np.frombuffer(struct.pack("<IIQQQQ24x", MAGIC, ch, nf, n_pairs, n_raw, total), np.uint8)
    if n_clips:
        first = np.asarray(clip_first_frames, np.int64) * ch
        if mut == "dir_off_by_one_clip":
            first = np.concatenate([first[1:], [M]])
        ex = np.concatenate([off, [n_pairs]])
        rx = np.concatenate([rr, [n_raw]])
        blob[o_dir:o_dir + 16 * n_clips] = np.stack([ex[first], rx[first]], 1).astype(np.uint64).reshape(-1).view(np.uint8)
    blob[o_israw:o_israw + nf] = raw_f
    blob[o_scale:o_scale + 4 * M] = d.scale_bits.view(np.uint8)
    cnt_out = np.where(raw_row, 0, fld) if mut == "nnz_unclamped" else cnt
    blob[o_cnt:o_cnt + 4 * M] = cnt_out.astype(np.uint32).view(np.uint8)
    blob[o_pairs:pairs_end] = pairs.view(np.uint8)
    if mut == "raw_gap_not_zeroed":
        blob[pairs_end:raw_off] = SENTINEL
    blob[raw_off:] = rawsec.reshape(-1).view(np.uint8)
    return blob, (nf, n_pairs, n_raw, total)


def model(d: Desc, mutation=None):
    """(blob bytes as uint8, (n_frames, n_pairs, n_raw_rows, bytes)) of glc_compact_device_records on `d`."""
    assert mutation is None or mutation in MUTATIONS
    return _pack(d, mutation)


def real_frames(clip_frames, mutation=None) -> np.ndarray:
    """Records of the virtual stream that are the clips' frames: clip i at slot_i, a junk record behind each."""
    out, slot = [], 0
    for n in clip_frames:
        out.append(np.arange(slot, slot + n))
        slot += n + (0 if mutation == "junk_frame_counted" else 1)
    return np.concatenate(out)


def model_batch(d_virtual: Desc, clip_frames, mutation=None):
    """The blob of a batch round over the virtual records `d_virtual` (sum(clip_frames[i] + 1) of them): header,
    clip directory (dir[2i], dir[2i + 1] = pairs, raw rows in front of clip i), the sections over the real frames."""
    assert mutation is None or mutation in MUTATIONS
    assert d_virtual.nf == sum(clip_frames) + len(clip_frames) and min(clip_frames) >= 1
    first = np.cumsum([0] + list(clip_frames[:-1]))
    return _pack(take_frames(d_virtual, real_frames(clip_frames, mutation)), mutation, first)


def layout(ch: int, nf: int, n_clips: int = 0):
    """(o_israw, o_scale, o_cnt, o_pairs, bound) of a blob of nf frames (n_clips > 0: of a batch round)."""
    M = nf * ch
    o_israw = 64 + align64(16 * n_clips)
    o_scale = o_israw + align64(nf)
    o_cnt = o_scale + align64(4 * M)
    o_pairs = o_cnt + align64(4 * M)
    return o_israw, o_scale, o_cnt, o_pairs, o_pairs + 4096 * M + 64


# ----------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    family: str
    desc: Desc
    clip_frames: tuple = ()          # batch: desc is the virtual stream
    info: dict = field(default_factory=dict)
    dense: bool = True               # False: too long for a dense host image (chunks)


def _q(rng, n):
    """n non-zero i16 values; the ends of the range among them."""
    q = rng.integers(1, 32768, n).astype(np.int64) * rng.choice([-1, 1], n)
    q[rng.random(n) < 0.1] = -32768
    return q.astype(np.int16)


def _qcycle(n, start=0):
    return np.array([Q_VALUES[(start + i) % len(Q_VALUES)] for i in range(n)], np.int16)


def _plane(rng, ch):
    p = rng.integers(-32768, 32768, (ch, FRAME)).astype(np.int16)
    ext = np.array(I16_EXTREMES, np.int16)
    for c in range(ch):
        p[c, :ext.size] = np.roll(ext, c)
        p[c, HOP - 1], p[c, HOP], p[c, FRAME - 1] = -32768, 32767, -32768
    return p


def _sparse_rows(b: Builder, rng, rows, hi=6):
    for m in rows:
        n = int(rng.integers(0, hi))
        ks = np.sort(rng.choice(HOP, n, replace=False))
        b.row(m, ks, _q(rng, n), scale=int(rng.integers(0, 1 << 32)))


def _fill(b: Builder, rng, raw_frames, flag_of=lambda f: FLAG_WORDS[f % len(FLAG_WORDS)], hi=6):
    raw_frames = set(int(f) for f in raw_frames)
    for f in range(b.nf):
        if f in raw_frames:
            b.raw(f, flag_of(f), _plane(rng, b.ch))
            for c in range(b.ch):
                b.scale_bits[f * b.ch + c] = int(rng.integers(0, 1 << 32))
        else:
            _sparse_rows(b, rng, range(f * b.ch, (f + 1) * b.ch), hi)


def _dense_row(b: Builder, rng, m, **kw):
    b.row(m, np.arange(HOP), _q(rng, HOP), **kw)


def _counts_cases():
    out = []
    for ch in (1, 3):
        rng = np.random.default_rng(7100 + ch)
        rows = []                                     # (placement, bins)
        for n in NNZ_COUNTS:
            rows.append(("spread", np.sort(rng.choice(HOP, n, replace=False))))
            if n <= 64:
                rows.append(("low", np.sort(rng.choice(64, n, replace=False))))
                rows.append(("high", 960 + np.sort(rng.choice(64, n, replace=False))))
        for lane in (0, 63, None):
            rows.append(("one_per_group", np.array([64 * g + ((37 * g + 5) % 64 if lane is None else lane) for g in range(16)])))
        rows.append(("63_64", np.array([63, 64])))
        rows.append(("every_other", np.arange(0, HOP, 2)))
        rows.append(("every_other", np.arange(1, HOP, 2)))
        nf = -(-len(rows) // ch)
        b = Builder(ch, nf)
        marks = []
        for m, (kind, ks) in enumerate(rows):
            b.row(m, ks, _qcycle(ks.size, m), scale=SCALE_BITS[m % len(SCALE_BITS)])
            marks.append((m, kind, int(ks.size)))
        out.append(Case(f"counts-ch{ch}", "counts", b.desc(), info={"marks": marks}))
    return out


def _disagree_cases():
    out = []
    rng = np.random.default_rng(7200)

    def rows_case(name, pairs_of_true_field, ch=2):
        nf = -(-len(pairs_of_true_field) // ch)
        b = Builder(ch, nf)
        for m, (true, fld) in enumerate(pairs_of_true_field):
            ks = np.arange(HOP) if true == HOP else np.sort(rng.choice(HOP, true, replace=False))
            b.row(m, ks, _q(rng, true), nnz=fld, scale=int(rng.integers(0, 1 << 32)))
        return Case(name, "disagree", b.desc(), info={"true_field": list(pairs_of_true_field)})

    out.append(rows_case("disagree-over", [(0, 1), (0, 1024), (5, 6), (5, 64), (5, 70), (63, 64), (64, 65), (64, 129),
                                           (1023, 1024), (3, 200)]))
    out.append(rows_case("disagree-under", [(1, 0), (2, 1), (64, 63), (65, 64), (65, 1), (128, 64), (129, 65), (1024, 1023),
                                            (1024, 0), (1024, 1)]))
    out.append(rows_case("disagree-clamp", [(1024, CLAMPED_FIELDS[0]), (1024, CLAMPED_FIELDS[1]), (10, CLAMPED_FIELDS[0]),
                                            (10, CLAMPED_FIELDS[1]), (0, CLAMPED_FIELDS[1]), (3, 3)]))
    b = Builder(2, 6)                                   # a non-zero nnz field on the rows of raw frames
    fields = {1: 7, 3: 1024, 4: 0xFFFFFFFF}
    for f in range(6):
        if f in fields:
            b.raw(f, FLAG_WORDS[f % 4], _plane(rng, 2), nnz=fields[f])
        else:
            _sparse_rows(b, rng, (2 * f, 2 * f + 1))
    out.append(Case("disagree-rawnnz", "disagree", b.desc(), info={"fields": fields}))
    b = Builder(2, 3)                                   # junk in bins 1024..2047 of compressed rows
    for m, true in enumerate((0, 3, 1024, 1, 64, 0)):
        ks = np.arange(HOP) if true == HOP else np.sort(rng.choice(HOP, true, replace=False))
        b.row(m, np.concatenate([ks, np.arange(HOP, FRAME)]), _q(rng, true + HOP))
    out.append(Case("disagree-upper", "disagree", b.desc()))
    b = Builder(2, 2)                                   # ... under a field that leaves room for them: filler, not junk
    for m, (true, fld) in enumerate(((0, 1), (3, 10), (1000, 1024), (64, 65))):
        ks = np.sort(rng.choice(HOP, true, replace=False))
        b.row(m, np.concatenate([ks, np.arange(HOP, FRAME)]), _q(rng, true + HOP), nnz=fld)
    out.append(Case("disagree-upper-over", "disagree", b.desc()))
    return out


def _raw_cases():
    out = []
    straddle = {3: 341, 5: 204, 7: 146}                 # the frame whose rows lie on both sides of row 1024
    for ch in RAW_CHANNELS:
        rng = np.random.default_rng(7300 + ch)
        f0 = straddle[ch]
        assert f0 * ch < BLOCK < (f0 + 1) * ch
        nf = f0 + 2
        raw = {3: range(1, nf, 2), 5: range(nf), 7: (f0,)}[ch]
        kind = {3: "alternating", 5: "all", 7: "straddle"}[ch]
        b = Builder(ch, nf)
        _fill(b, rng, raw, hi=4)
        out.append(Case(f"raw-ch{ch}-{kind}", "raw", b.desc(), info={"placement": kind, "straddle": f0}))
    for kind, raw in (("none", ()), ("first", (0,)), ("last", (4,))):
        rng = np.random.default_rng(7310 + len(kind))
        b = Builder(2, 5)
        _fill(b, rng, raw, flag_of=lambda f: 0x100)
        out.append(Case(f"raw-{kind}", "raw", b.desc(), info={"placement": kind}))
    for i, flag in enumerate(FLAG_WORDS):                # one flag word each, so that no other case hides a miss
        rng = np.random.default_rng(7320 + i)
        b = Builder(1, 3)
        _fill(b, rng, (1,), flag_of=lambda f: flag)
        out.append(Case(f"raw-flag-{flag:#x}", "raw", b.desc(), info={"placement": "middle", "flag": flag}))
    for n, gap in GAP_PAIRS.items():
        rng = np.random.default_rng(7330 + n)
        b = Builder(1, 3)
        b.row(0, np.sort(rng.choice(HOP, n, replace=False)), _q(rng, n))
        b.raw(1, 1, _plane(rng, 1))
        out.append(Case(f"raw-gap{gap}", "raw", b.desc(), info={"placement": "middle", "gap": gap}))
    return out


def block_frames(ch: int, rows: int) -> int:
    return max(1, int(rows / ch + 0.5))


def _blocks_cases():
    out, seen = [], set()
    for ch in BLOCK_CHANNELS:
        for M in BLOCK_ROWS:
            nf = block_frames(ch, M)
            if (ch, nf) in seen:
                continue
            seen.add((ch, nf))
            rng = np.random.default_rng(7400 + 10000 * ch + nf)
            b = Builder(ch, nf)
            raw = np.flatnonzero(rng.random(nf) < 0.08) if nf > 1 else ()
            _fill(b, rng, raw)
            out.append(Case(f"blocks-ch{ch}-nf{nf}", "blocks", b.desc(), info={"rows": nf * ch}))
    rng = np.random.default_rng(7490)
    b = Builder(1, BLOCK + 1)                            # 1024 rows x 1024 pairs: the pair count of a block at its limit
    for m in range(BLOCK):
        _dense_row(b, rng, m)
    b.row(BLOCK, [77], [-32768])
    out.append(Case("blocks-dense-then-one", "blocks", b.desc(), info={"rows": BLOCK + 1}))
    b = Builder(1, BLOCK + 2)                            # 1024 raw rows: the raw-row count of a block at its limit
    for f in range(BLOCK):
        p = np.zeros((1, FRAME), np.int16)
        p[0, :4] = (f + 1, -(f + 1), -32768, 32767)
        p[0, FRAME - 1] = f - 512
        b.raw(f, FLAG_WORDS[f % 4], p)
    b.row(BLOCK, [0, 63, 64, 1023], [1, -1, 32767, -32768])
    b.raw(BLOCK + 1, 0x100, _plane(rng, 1))
    out.append(Case("blocks-raw-block", "blocks", b.desc(), info={"rows": BLOCK + 2}))
    b = Builder(1, BLOCK + 2)                            # 1023 dense rows and a raw one: both fields of the word loaded
    for m in range(BLOCK - 1):
        _dense_row(b, rng, m)
    b.raw(BLOCK - 1, 2, _plane(rng, 1))
    b.row(BLOCK, [5, 900], [3, -3])
    b.raw(BLOCK + 1, 1, _plane(rng, 1))
    out.append(Case("blocks-1023-dense-1-raw", "blocks", b.desc(), info={"rows": BLOCK + 2}))
    return out


def _chunks_case():
    rng = np.random.default_rng(7500)
    nf = CHUNK_FRAMES
    raw = np.array([5, 1023 * BLOCK + 17, 1024 * BLOCK + 3, 1025 * BLOCK + 2])
    assert tuple(raw // BLOCK) == CHUNK_RAW_BLOCKS and raw[-1] < nf
    # 0..3 pairs per row, the mix different in every block: a block's total is its own
    bias = rng.random(-(-nf // BLOCK))
    n = np.minimum((rng.random(nf) * 4 * (0.25 + 0.75 * bias[np.arange(nf) // BLOCK])).astype(np.int64), 3)
    n[nf - 7:] = (1, 2, 0, 3, 1, 2, 3)                  # the last block is 7 rows, and they count
    n[raw] = 0
    r = np.repeat(np.arange(nf), n)
    j = np.arange(r.size) - np.searchsorted(r, r, "left")
    # ascending, distinct bins: the j-th entry of a row lies in the j-th third of the bins
    k = j * 341 + rng.integers(0, 341, r.size)
    k[(j == 2) & (rng.random(r.size) < 0.05)] = HOP - 1
    q = _q(rng, r.size)
    flags = np.zeros(nf, np.uint32)
    flags[raw] = FLAG_WORDS
    planes = {int(f): _plane(rng, 1) for f in raw}
    scale = rng.integers(0, 1 << 32, nf).astype(np.uint32)
    d = Desc(1, nf, flags, scale, n.astype(np.uint32), r, k, q, planes)
    return Case("chunks", "chunks", d, info={"raw": raw.tolist()}, dense=False)


def _junk(b: Builder, rng, f, kind):
    if kind == "rawflag":
        b.raw(f, 0x100 if f % 2 else 1, _plane(rng, b.ch), nnz=1024)
    else:
        for c in range(b.ch):
            _dense_row(b, rng, f * b.ch + c)


def _batch_case(name, ch, clips, raw_of, junk_of, seed, hi=6):
    """clips: frames per clip; raw_of(i, f): is frame f of clip i raw; junk_of(i): kind of the junk record behind clip i."""
    rng = np.random.default_rng(seed)
    V = sum(clips) + len(clips)
    b = Builder(ch, V)
    slot, kinds = 0, []
    for i, n in enumerate(clips):
        for f in range(n):
            v = slot + f
            if raw_of(i, f):
                b.raw(v, FLAG_WORDS[v % 4], _plane(rng, ch))
            else:
                _sparse_rows(b, rng, range(v * ch, (v + 1) * ch), hi)
        kinds.append(junk_of(i))
        _junk(b, rng, slot + n, kinds[-1])
        slot += n + 1
    return Case(name, "batch", b.desc(), clip_frames=tuple(clips), info={"junk": kinds})


def _batch_cases():
    alt = lambda i: "rawflag" if i % 2 == 0 else "dense"
    out = [
        _batch_case("batch-one-frame-clips", 2, [1] * 5, lambda i, f: i == 3, lambda i: "dense", 7601),
        _batch_case("batch-first-raw", 3, [2, 3, 1, 2], lambda i, f: f == 0 and i in (1, 3), lambda i: "rawflag", 7602),
        _batch_case("batch-all-raw", 2, [1, 2, 3], lambda i, f: True, lambda i: "dense", 7603),
        _batch_case("batch-single", 2, [5], lambda i, f: f == 2, alt, 7604),
        _batch_case("batch-single-dense-junk", 1, [2], lambda i, f: False, lambda i: "dense", 7605),
        _batch_case("batch-700", 1, [1] * 700, lambda i, f: i % 97 == 5, alt, 7606),
    ]
    for first in (1023, 1024, 1025):                     # a clip that starts at this row of the round's real rows
        out.append(_batch_case(f"batch-edge-{first}", 1, [first, 3, 1], lambda i, f: (i == 0 and f % 199 == 7) or (i == 2),
                               alt, 7610 + first, hi=4))
    return out


def build_cases():
    return (_counts_cases() + _disagree_cases() + _raw_cases() + _blocks_cases() + [_chunks_case()] + _batch_cases())


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
    return _cases


def digest(cs) -> str:
    h = hashlib.sha256()
    for c in cs:
        d = c.desc
        h.update(f"{c.name}|{c.family}|{d.ch}|{d.nf}|{c.clip_frames}".encode())
        for a in (d.flags, d.scale_bits, d.nnz, d.e_row, d.e_k, d.e_q):
            h.update(np.ascontiguousarray(a).tobytes())
        for f in sorted(d.planes):
            h.update(struct.pack("<q", f) + d.planes[f].tobytes())
    return h.hexdigest()
