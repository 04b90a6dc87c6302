"""Compact blobs written by hand for tests/test_compact_decode.py, from the model of DESIGN.md section 3:

  header 64 B {u32 "GLCB", u32 channels, u64 n_frames, u64 n_pairs, u64 n_raw_rows, u64 bytes, 24 B zero}
  | is_raw u8[n_frames] | scale f32[M] | cnt u32[M] | pairs u32[n_pairs] | raw i16[n_raw_rows][2048]
  M = n_frames * channels, every section 64-byte aligned, all padding zero.

A stream is DESCRIBED as a list of frames - ("raw", planes int16 [ch][2048]) or ("c", [Row per channel]) - and
`pack` writes its blob into a buffer of glc_compact_bound bytes.  `pack` takes overrides for the fields a
malformed blob lies in (header words, single cnt entries); whatever it is given, it keeps every cnt <= 1024
and every raw count <= M, so that a reader with no checks at all would still stay inside the buffer: the
tests pin a defined result, they provoke nothing.  `emptied` is the description of what the device check must
decode such a blob AS: the rejected rows' lists emptied (a rejected raw frame becomes a compressed frame of
empty lists), which then goes through the host path (glc_frames_from_compact + glc_decode) for the expected
samples.  `tables` is the numpy model of the row tables R2 builds (row_begin, row_cnt, row_raw).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

HOP, FRAME = 1024, 2048
MAGIC = 0x42434C47
SCAN_BLOCK = 1024        # rows per k_r2_scan_rows workgroup, block sums per chunk of k_r2_scan_blocks
F32 = np.float32

BAD_HEADER, ROW_BOUNDS, NOT_CANONICAL, RAW_RANGE, PAIR_SUM, RAW_SUM = 1, 2, 4, 8, 16, 32


def align64(v: int) -> int:
    return (v + 63) & ~63


def layout(ch: int, nf: int):
    m = nf * ch
    o_israw = 64
    o_scale = o_israw + align64(nf)
    o_cnt = o_scale + align64(4 * m)
    o_pairs = o_cnt + align64(4 * m)
    return o_israw, o_scale, o_cnt, o_pairs, o_pairs + 4096 * m + 64


@dataclass
class Row:
    idx: np.ndarray          # bins as stored (uint16)
    q: np.ndarray            # int16
    scale_bits: int = 0x3C23D70A     # 0.01f

    @property
    def pairs(self) -> np.ndarray:
        return (np.asarray(self.idx, np.uint32) & 0xFFFF) | ((np.asarray(self.q, np.int16).view(np.uint16).astype(np.uint32)) << 16)


def row(rng, n, scale_bits=0x3C23D70A, lo=-3000, hi=3000) -> Row:
    idx = np.sort(rng.choice(HOP, n, replace=False)).astype(np.uint16)
    q = rng.randint(lo, hi, n).astype(np.int16)
    q[q == 0] = 7
    return Row(idx, q, scale_bits)


EMPTY_IDX, EMPTY_Q = np.zeros(0, np.uint16), np.zeros(0, np.int16)


def raw_planes(rng, ch):
    p = rng.randint(-32768, 32768, (ch, FRAME)).astype(np.int16)
    p[0, 0], p[-1, -1] = -32768, 32767
    return p


def n_samples_of(ch: int, nf: int) -> int:
    """An interleaved length whose stream has exactly nf frames (src/codec.rs:433-455)."""
    return nf * HOP * ch


def pack(ch: int, frames, *, magic=MAGIC, n_frames=None, n_pairs=None, n_raw_rows=None, bytes_field=None, cnt_set=None,
         size=None) -> tuple:
    """-> (buffer uint8 of glc_compact_bound bytes (or `size`), the blob's true byte count)."""
    nf = len(frames)
    m = nf * ch
    o_israw, o_scale, o_cnt, o_pairs, bound = layout(ch, nf)
    buf = np.zeros(bound if size is None else size, np.uint8)
    israw = buf[o_israw:o_israw + nf]
    scale = buf[o_scale:o_scale + 4 * m].view(np.uint32)
    cnt = buf[o_cnt:o_cnt + 4 * m].view(np.uint32)
    lists, planes = [], []
    for f, (kind, body) in enumerate(frames):
        if kind == "raw":
            israw[f] = 1
            planes.append(np.ascontiguousarray(body, np.int16).reshape(ch, FRAME))
            continue
        assert len(body) == ch
        for c, r in enumerate(body):
            scale[f * ch + c] = r.scale_bits
            cnt[f * ch + c] = len(r.idx)
            lists.append(r.pairs)
    pairs = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32)
    raw = np.concatenate(planes).reshape(-1) if planes else np.zeros(0, np.int16)
    raw_off = align64(o_pairs + 4 * pairs.size)
    true_bytes = raw_off + 2 * raw.size
    buf[o_pairs:o_pairs + 4 * pairs.size] = pairs.view(np.uint8)
    buf[raw_off:raw_off + 2 * raw.size] = raw.view(np.uint8)
    for mrow, v in (cnt_set or {}).items():
        assert v <= HOP
        cnt[mrow] = v
    hp = pairs.size if n_pairs is None else n_pairs
    hr = raw.size // FRAME if n_raw_rows is None else n_raw_rows
    assert hr <= m and hp <= HOP * m
    buf[:64] = np.frombuffer(struct.pack("<IIQQQQ24x", magic, ch, nf if n_frames is None else n_frames, hp, hr,
                                         true_bytes if bytes_field is None else bytes_field), np.uint8)
    return buf, true_bytes


def emptied(ch: int, frames, rows=(), all_rows=False):
    """The description with the lists of `rows` (row = frame * ch + channel) emptied; a raw frame named by any
    of its rows becomes a compressed frame of empty lists of scale +0.0 (a blob keeps no scale a test could
    name for them: the builder writes 0).  all_rows (a bad header): every list empty, every scale +0.0."""
    rows = set(rows)
    out = []
    for f, (kind, body) in enumerate(frames):
        hit = [all_rows or (f * ch + c) in rows for c in range(ch)]
        if kind == "raw":
            out.append(("c", [Row(EMPTY_IDX, EMPTY_Q, 0) for _ in range(ch)]) if any(hit) else (kind, body))
        else:
            out.append(("c", [Row(EMPTY_IDX, EMPTY_Q, 0 if all_rows else r.scale_bits) if hit[c] else r
                              for c, r in enumerate(body)]))
    return out


def tables(ch: int, frames):
    """row_begin (u32 elements from the blob's start), row_cnt, row_raw (i16 elements from the blob's start, -1)
    of a VALID description, as R2 must build them."""
    nf = len(frames)
    m = nf * ch
    o_pairs = layout(ch, nf)[3]
    cnt = np.zeros(m, np.uint32)
    is_raw = np.zeros(m, bool)
    for f, (kind, body) in enumerate(frames):
        if kind == "raw":
            is_raw[f * ch:(f + 1) * ch] = True
        else:
            cnt[f * ch:(f + 1) * ch] = [len(r.idx) for r in body]
    excl = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))[:-1]]).astype(np.uint64)
    n_pairs = int(cnt.sum(dtype=np.uint64))
    raw_off = align64(o_pairs + 4 * n_pairs)
    begin = np.where(is_raw, 0, o_pairs // 4 + excl).astype(np.uint64)
    planes_before = np.concatenate([[0], np.cumsum(is_raw)[:-1]]).astype(np.int64)
    first_plane = planes_before - (np.arange(m) % ch)
    row_raw = np.where(is_raw, raw_off // 2 + first_plane * FRAME, -1).astype(np.int64)
    return begin, cnt, row_raw


def big_mono(nf: int, raw_frames, seed=5):
    """A mono blob of `nf` frames built without a Python loop over them: lists of 0..3 entries (ascending bins
    that depend on the row), the frames in `raw_frames` raw.  -> (buffer of exactly the blob's bytes + 64, bytes,
    (row_begin, row_cnt, row_raw) as R2 must build them)."""
    rng = np.random.RandomState(seed)
    o_israw, o_scale, o_cnt, o_pairs, _ = layout(1, nf)
    cnt = rng.randint(0, 4, nf).astype(np.uint32)
    is_raw = np.zeros(nf, bool)
    is_raw[list(raw_frames)] = True
    cnt[is_raw] = 0
    excl = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))[:-1]]).astype(np.uint64)
    n_pairs = int(cnt.sum(dtype=np.uint64))
    owner = np.repeat(np.arange(nf, dtype=np.uint64), cnt)
    j = np.arange(n_pairs, dtype=np.uint64) - excl[owner]
    idx = (j * 300 + owner % 200).astype(np.uint32)              # ascending inside a row, below 1024
    pairs = idx | (((owner % 1000) + 1).astype(np.uint32) << 16)
    n_raw = int(is_raw.sum())
    raw_off = align64(o_pairs + 4 * n_pairs)
    nbytes = raw_off + 4096 * n_raw
    buf = np.zeros(nbytes + 64, np.uint8)
    buf[o_israw:o_israw + nf] = is_raw
    buf[o_scale:o_scale + 4 * nf].view(np.uint32)[:] = 0x3C23D70A
    buf[o_cnt:o_cnt + 4 * nf].view(np.uint32)[:] = cnt
    buf[o_pairs:o_pairs + 4 * n_pairs] = pairs.view(np.uint8)
    buf[raw_off:nbytes].view(np.int16)[:] = (np.arange(n_raw * FRAME) % 30000 - 15000).astype(np.int16)
    buf[:64] = np.frombuffer(struct.pack("<IIQQQQ24x", MAGIC, 1, nf, n_pairs, n_raw, nbytes), np.uint8)
    begin = np.where(is_raw, 0, o_pairs // 4 + excl).astype(np.uint64)
    planes_before = np.concatenate([[0], np.cumsum(is_raw)[:-1]]).astype(np.int64)
    row_raw = np.where(is_raw, raw_off // 2 + planes_before * FRAME, -1).astype(np.int64)
    return buf, nbytes, (begin, cnt, row_raw)
