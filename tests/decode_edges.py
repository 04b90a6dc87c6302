"""Deterministic streams that sit on the structural edges of the decode kernels, what to run on them, and the
bits every run must give (test helper: numpy + the CPU oracle only).

The decode side branches on SHAPE, not on data: how many indices the union of 8 frames holds (the apply
loop walks it four entries per trip and has a 1..3-entry tail), how long a list is against the plan
kernel's first load of 256 pairs, which rows of a group are raw or lie past the last frame, how many units
a launch has (placement by rank, plan batches of 2048 units), whether a launch repeats the one before, and
where an overlap-add destination starts.  Encoded audio lands on those edges by accident at best.  The
families built here land on them on purpose:

  union      n_u of UNION_SIZES, once with all 8 rows on the same indices (dense unit, priority ladder) and
             once split disjointly over the rows (every per-row skip taken and not taken); indices on both
             sides of the scan's nibble / mask-word / wave boundaries; a union of stored q == 0 only
  lists      one row of LIST_LENGTHS pairs beside seven empty and beside seven full rows, at every position
  groups     n_frames of GROUP_FRAMES, ranges that start inside a group, one-frame ranges, a raw frame at
             each position of a group, all / all but one raw, raw only in the partial last group; 1..8 channels
  raw        raw_pcm of 0, 1, ch, 2048 ch - 1, 2048 ch, 2048 ch + 1 samples, the int16 extremes, a ramp over all of int16; 1, 2, 3, 7 channels
  values     q at the ends of int16, scales 0, -1, subnormal, 1e-12 and its neighbours, FLT_MAX, inf, NaN
  placement  launches of PLACEMENT_UNITS units and one of two plan batches, every unit's work equal / different
  reuse      launch sequences on one Decoder that repeat, change range, variant and stream
  overlap    hop ranges at both ends of a stream and across the 4096-frame decode round, 1..9 channels,
             destinations 0 / 4 / 8 / 12 bytes past a 16-byte boundary

A stream is serialised to .glc here (`Stream.to_glc`, the bincode layout of src/codec.rs:31-69) and handed
to the library through the constructors it already has (`Stream.to_encoded`).  Expected blocks come from the
C oracle's imdct_block on the dequantised row (src/codec.rs:651-675), computed once per DISTINCT row (the
families share rows so that launches of thousands of units cost a few hundred oracle rows); expected PCM is
the overlap-add of those blocks (src/codec.rs:693-729), which tests/test_decode_edges.py checks against both
oracles' whole-stream decode.  `model_blocks` / `model_hops` restate the SHIPPED algorithm (union, skip,
four-at-a-time walk, raw rows, rank-and-deal placement, plan batches, rounds, overlap-add) in numpy with
optional single-edit mutations (MUTATIONS): each must change some expected output, which is what shows that
the families would notice such an edit of a kernel.

Subnormal products: the clamp max(scale, 1e-12) and |q| >= 1 keep every non-zero coefficient at or above
1e-12 / 32768 = 3.05e-17, and the smallest non-zero |T[k][i]| is 1.6e-4 (no table entry is zero), so no single
product coef * T[k][i] of any stream can be subnormal (smallest: 4.9e-21); `smallest_product` computes that
bound from the tables and the test asserts it, so there is no subnormal-product case to keep.
"""
from __future__ import annotations

import hashlib
import os
import struct
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O

F32 = np.float32
HOP, FRAME, G = 1024, 2048, 8
SENTINEL_BITS = 0x7FC5A5A5          # a NaN no arithmetic produces: "never written"
PLAN_GROUPS = 2048                  # glc_api.hip kPlanGroups: (group, channel) units per plan batch
ROUND_FRAMES = 4096                 # glc_api.hip kDecodeChunkFrames
ORDER_MAX_UNITS = 4096              # glc_kernels.hip kOrderMaxUnits

UNION_SIZES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 1020, 1021, 1022, 1023, 1024)
SCAN_EDGES = (0, 3, 4, 31, 32, 255, 256, 511, 512, 767, 768, 1023)
LIST_LENGTHS = (0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024)
GROUP_FRAMES = (1, 7, 8, 9, 15, 16, 17)
GROUP_CHANNELS = (1, 2, 3, 5, 8)
RANGE_STARTS = (1, 7, 8, 9)
RAW_CHANNELS = (1, 2, 3, 7)
RAW_VALUES = (-32768, -32767, -1, 0, 1, 32767)
Q_VALUES = (-32768, -32767, -1, 1, 32767)
TINY = F32(1e-12)
SCALES = tuple(F32(x) for x in (0.0, -1.0, 1e-40, np.nextafter(TINY, F32(0)), TINY, np.nextafter(TINY, F32(1)),
                                np.finfo(np.float32).max, np.inf, np.nan))
PLACEMENT_UNITS = (255, 256, 257, 1023, 1024, 1025, 2047, 2048)
PLACEMENT_SHAPES = {255: 3, 256: 2, 257: 1, 1023: 3, 1024: 4, 1025: 5, 2047: 1, 2048: 8}  # units -> channels
TWO_BATCH = (7, 292 * G + 3)        # channels, frames: 293 groups x 7 = 2051 units, a batch holds 292 groups
OVERLAP_CHANNELS = (1, 2, 3, 4, 5, 8, 9)
OFFSETS = (0, 4, 8, 12)
LONG_FRAMES = ROUND_FRAMES + 4      # the overlap family's stream of more than one decode round

MUTATIONS = ("drop_tail", "first_256_pairs", "union_7_rows", "pair_skip_either", "no_clamp", "nan_through_clamp",
             "past_end_live", "raw_le", "raw_planar", "raw_mul_recip", "norm_times_window", "rank_tie_le",
             "tail_added", "hop0_reads_prev")
_UNIT_MUTATIONS = {"drop_tail", "first_256_pairs", "union_7_rows", "pair_skip_either", "no_clamp", "nan_through_clamp",
                   "norm_times_window"}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def sentinel(shape) -> np.ndarray:
    return np.full(shape, SENTINEL_BITS, np.uint32).view(F32)


# ----------------------------------------------------------------------------------------------------
# rows and streams
# ----------------------------------------------------------------------------------------------------

class Row:
    """One sparse list (idx ascending, q as stored - zero allowed) and its scale.  Rows are shared between
    frames and streams; `key` identifies the content."""
    __slots__ = ("idx", "q", "scale", "pairs", "key")

    def __init__(self, idx, q, scale):
        self.idx = np.ascontiguousarray(idx, np.uint16)
        self.q = np.ascontiguousarray(q, np.int16)
        assert self.idx.size == self.q.size and (np.diff(self.idx.astype(np.int64)) > 0).all() and \
            (self.idx.size == 0 or self.idx[-1] < HOP)
        self.scale = F32(scale)
        self.pairs = self.idx.astype(np.uint32) | (self.q.view(np.uint16).astype(np.uint32) << 16)
        self.key = self.pairs.tobytes() + self.scale.tobytes()

    def __len__(self):
        return self.idx.size

    def coefficients(self, mut=None) -> np.ndarray:
        """src/codec.rs:651-663: q / 32768 * max(scale, 1e-12) at the stored indices, +0.0 elsewhere."""
        n = 256 if mut == "first_256_pairs" else HOP
        if mut == "no_clamp":
            s = self.scale
        elif mut == "nan_through_clamp":
            s = TINY if TINY > self.scale else self.scale     # what Python's max(scale, 1e-12) returns
        else:
            s = np.fmax(self.scale, TINY)                     # f32::max ignores a NaN scale
        co = np.zeros(HOP, F32)
        with np.errstate(all="ignore"):
            co[self.idx[:n]] = (self.q[:n].astype(F32) / F32(32768.0)) * s
        return co


EMPTY = Row([], [], 0.5)


class Stream:
    """sample rate, channels, rows[f * ch + c] (ignored for raw frames), raw[f] (int16 vector or None)."""

    def __init__(self, sr, ch, rows, raw=None, delay=512, lose=300):
        self.sr, self.ch = sr, ch
        self.rows = list(rows)
        assert len(self.rows) % ch == 0
        self.nf = len(self.rows) // ch
        self.raw = list(raw) if raw is not None else [None] * self.nf
        assert len(self.raw) == self.nf
        self.raw = [None if r is None else np.ascontiguousarray(r, np.int16) for r in self.raw]
        self.delay = delay
        self.orig = max(0, (self.nf + 1) * HOP * ch - delay - lose)   # the trim takes from both ends
        self.total = self.orig
        self._glc = None

    def to_glc(self) -> bytes:
        if self._glc is None:
            out = [struct.pack("<IHQQ", self.sr, self.ch, self.total, self.nf)]
            for f in range(self.nf):
                if self.raw[f] is not None:     # src/codec.rs:510-521: a raw frame carries no lists and no scales
                    out += [struct.pack("<QQB", 0, 0, 1), struct.pack("<Q", self.raw[f].size), self.raw[f].tobytes()]
                    continue
                rows = self.rows[f * self.ch:(f + 1) * self.ch]
                out.append(struct.pack("<Q", self.ch))
                for r in rows:
                    out += [struct.pack("<Q", len(r)), r.pairs.tobytes()]
                out += [struct.pack("<Q", self.ch), np.array([r.scale for r in rows], F32).tobytes(), b"\x00"]
            out.append(struct.pack("<IIQ", self.delay, 0, self.orig))
            self._glc = b"".join(out)
        return self._glc

    def to_encoded(self, glc_amd, how="bytes", stream_id=0):
        """The stream as an EncodedAudio, through one of the library's constructors."""
        if how == "bytes":
            return glc_amd.EncodedAudio.from_bytes(self.to_glc())
        if how == "nested":
            frames = []
            for f in range(self.nf):
                if self.raw[f] is not None:
                    frames.append(([], np.zeros(0, F32), self.raw[f]))
                else:
                    rows = self.rows[f * self.ch:(f + 1) * self.ch]
                    frames.append(([r.pairs for r in rows], np.array([r.scale for r in rows], F32), None))
            return glc_amd.EncodedAudio.from_nested(glc_amd.AudioHeader(self.sr, self.ch, self.total), frames,
                                                    glc_amd.GaplessInfo(self.delay, 0, self.orig), stream_id)
        if how == "parts":
            live = [f for f in range(self.nf) if self.raw[f] is None]
            lists = [r for f in live for r in self.rows[f * self.ch:(f + 1) * self.ch]]
            per_frame = np.array([0 if self.raw[f] is not None else self.ch for f in range(self.nf)], np.uint64)
            begin = np.concatenate([[0], np.cumsum(per_frame)]).astype(np.uint64)
            raws = [r if r is not None else np.zeros(0, np.int16) for r in self.raw]
            parts = dict(sample_rate=self.sr, channels=self.ch, total_samples=self.total, encoder_delay=self.delay,
                         padding=0, original_length=self.orig, n_frames=self.nf, n_lists=len(lists),
                         list_begin=begin, scale_begin=begin,
                         list_off=np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.uint64),
                         pairs=np.concatenate([r.pairs for r in lists] + [np.zeros(0, np.uint32)]),
                         scales=np.array([r.scale for r in lists], F32),
                         raw_tag=np.array([r is not None for r in self.raw], np.uint8),
                         raw_begin=np.concatenate([[0], np.cumsum([r.size for r in raws])]).astype(np.uint64),
                         raw=np.concatenate(raws + [np.zeros(0, np.int16)]))
            return glc_amd.EncodedAudio.from_parts(parts, stream_id)
        assert how == "records" and all(r is None for r in self.raw)
        rec = glc_amd.lib.glc_record_bytes(self.ch)
        hdr = rec - 4096 * self.ch
        buf = np.zeros((self.nf, rec), np.uint8)
        pay = buf[:, hdr:].view(np.int16).reshape(self.nf, self.ch, FRAME)          # views of buf
        meta = buf[:, 8:8 + 8 * self.ch].view(np.uint32).reshape(self.nf, self.ch, 2)
        for m, r in enumerate(self.rows):
            assert (r.q != 0).all()             # a record holds dense q: a stored zero cannot be expressed
            pay[m // self.ch, m % self.ch, r.idx] = r.q
            meta[m // self.ch, m % self.ch] = (r.scale.view(np.uint32), len(r))
        # a stream length that gives nf frames (src/codec.rs:431-436); the gapless window is then the library's own,
        # so cases built this way run imdct launches only
        return glc_amd.EncodedAudio.from_records(self.sr, (self.nf * HOP + 512) * self.ch, self.ch, buf.reshape(-1))


@dataclass
class Run:
    """kind 'decode' (Decoder.decode), 'imdct' (imdct_device frames [a, b)), 'range' (decode_range_device hops
    [a, b) to a destination `offset` bytes past a 16-byte boundary); `variant` as in include/glc_debug.h."""
    kind: str
    a: int = 0
    b: int = 0
    offset: int = 0
    variant: int = 0


@dataclass
class Case:
    name: str
    family: str
    stream: Stream
    runs: list
    how: str = "bytes"
    info: dict = field(default_factory=dict)


# ----------------------------------------------------------------------------------------------------
# expected bits: the C oracle per distinct row, a three-line overlap-add
# ----------------------------------------------------------------------------------------------------

_block_cache: dict = {}


def _oracle_block(row: Row) -> np.ndarray:
    _, w, _ = O.tables()
    with np.errstate(all="ignore"):
        return O.imdct_block(row.coefficients()) * w      # :669, :674


def row_blocks(rows) -> None:
    """Fill the cache with the oracle block of every distinct row of `rows`."""
    todo = {}
    for r in rows:
        if r.key not in _block_cache and r.key not in todo:
            todo[r.key] = r
    if todo:
        O.tables()
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:      # ctypes releases the GIL
            for k, b in zip(todo, ex.map(_oracle_block, todo.values())):
                _block_cache[k] = b


def raw_block(raw: np.ndarray, ch: int, c: int, mut=None, pool_after=None) -> np.ndarray:
    """src/codec.rs:629-640: the vector read as if interleaved, / 32767, zero past its end, no window."""
    i = np.arange(FRAME)
    si = c * FRAME + i if mut == "raw_planar" else i * ch + c
    ok = si <= raw.size if mut == "raw_le" else si < raw.size
    pool = raw if pool_after is None else np.concatenate([raw, pool_after])   # what follows it in the raw pool
    v = np.zeros(FRAME, F32)
    x = pool[si[ok]].astype(F32)
    v[ok] = x * F32(1.0 / 32767.0) if mut == "raw_mul_recip" else x / F32(32767.0)
    return v


def expected_blocks(st: Stream, f0: int, f1: int) -> np.ndarray:
    """[(f1 - f0) * ch, 2048]: what imdct_device must write for frames [f0, f1)."""
    ch = st.ch
    row_blocks(st.rows[m] for f in range(f0, f1) if st.raw[f] is None for m in range(f * ch, (f + 1) * ch))
    out = np.empty(((f1 - f0) * ch, FRAME), F32)
    for f in range(f0, f1):
        for c in range(ch):
            out[(f - f0) * ch + c] = raw_block(st.raw[f], ch, c) if st.raw[f] is not None else _block_cache[st.rows[f * ch + c].key]
    return out


def overlap_add(blocks: np.ndarray, f_first: int, nf: int, ch: int, h0: int, h1: int) -> np.ndarray:
    """Hops [h0, h1) from blocks[(f - f_first) * ch + c]: second half of frame h - 1 (+0.0 before frame 0) plus
    first half of frame h; hop nf is the bare tail (src/codec.rs:601, :693-705, :722-729)."""
    b = blocks.reshape(-1, ch, FRAME)
    out = np.empty((h1 - h0, HOP, ch), F32)
    with np.errstate(all="ignore"):
        for h in range(h0, h1):
            prev = b[h - 1 - f_first, :, HOP:] if h >= 1 else np.zeros((ch, HOP), F32)
            out[h - h0] = (prev + b[h - f_first, :, :HOP]).T if h < nf else prev.T
    return out.reshape(-1)


def expected_hops(st: Stream, h0: int, h1: int) -> np.ndarray:
    if h1 <= h0:
        return np.zeros(0, F32)
    f_first = max(h0 - 1, 0)
    return overlap_add(expected_blocks(st, f_first, min(h1, st.nf)), f_first, st.nf, st.ch, h0, h1)


def trim(st: Stream, allv: np.ndarray) -> np.ndarray:
    """src/codec.rs:756-765"""
    if allv.size > st.delay:
        allv = allv[st.delay:]
    return allv[:st.orig]


def expected_run(st: Stream, run: Run) -> np.ndarray:
    if run.kind == "imdct":
        return expected_blocks(st, run.a, run.b).reshape(-1)
    if run.kind == "range":
        return expected_hops(st, run.a, run.b)
    return trim(st, expected_hops(st, 0, st.nf + 1))


def smallest_product() -> float:
    T, _, _ = O.tables()
    assert (T != 0).all()
    return float(TINY / F32(32768.0)) * float(np.abs(T).min())


# ----------------------------------------------------------------------------------------------------
# the plan of one unit (what k_imdct_plan derives), used by the coverage test and the model
# ----------------------------------------------------------------------------------------------------

_plan_cache: dict = {}


def unit_rows(st: Stream, f0: int, f1: int, fg: int, c: int):
    """The 8 entries of unit (fg, c) of a launch over frames [f0, f1): a Row, 'raw', or None past the end."""
    out = []
    for g in range(G):
        f = f0 + fg * G + g
        out.append(None if f >= f1 else "raw" if st.raw[f] is not None else st.rows[f * st.ch + c])
    return out


def unit_plan(rows) -> dict:
    key = tuple(r.key if isinstance(r, Row) else r for r in rows)
    p = _plan_cache.get(key)
    if p is None:
        live = [isinstance(r, Row) for r in rows]
        lens = [len(r) if l else 0 for r, l in zip(rows, live)]
        idx = [r.idx for r, l in zip(rows, live) if l]
        union = np.unique(np.concatenate(idx)) if idx else np.zeros(0, np.uint16)
        total, n_u = sum(lens), int(union.size)
        rawm = sum(1 << g for g, r in enumerate(rows) if r == "raw")
        C = np.stack([r.coefficients() if l else np.zeros(HOP, F32) for r, l in zip(rows, live)])
        present = C.view(np.uint32)[:, union] != 0           # the skip test of k_imdct_apply: coefficient bits
        states = [set(map(tuple, present[2 * p:2 * p + 2].T.astype(int).tolist())) for p in range(G // 2)]
        p = dict(live=sum(1 << g for g, l in enumerate(live) if l), rawm=rawm, lens=lens, union=union, n_u=n_u,
                 total=total, dense=n_u * G <= 2 * total, work=total + n_u + (64 if rawm else 0), states=states,
                 owners=present.sum(axis=0) if n_u else np.zeros(0, int))
        _plan_cache[key] = p
    return p


def launch_batches(n_frames: int, ch: int, plan_groups: int):
    """(first group, groups) of each plan batch of a launch (launch_imdct_rows)."""
    groups, per = (n_frames + G - 1) // G, plan_groups // ch
    return [(g0, min(per, groups - g0)) for g0 in range(0, groups, per)]


def plan_groups_of(st: Stream) -> int:
    units = (st.nf + G - 1) // G * st.ch
    return max(st.ch, min(max(PLAN_GROUPS, st.ch), units))       # decode_prepare_impl


def launches_of(st: Stream, run: Run):
    """Frame ranges of the D1 launches a run makes (decode_hops_prepared / the decode rounds)."""
    if run.kind == "imdct":
        return [(run.a, run.b)] if run.b > run.a else []
    h0, h1 = (0, st.nf + 1) if run.kind == "decode" else (run.a, run.b)
    if h1 <= h0:
        return []
    out = [(h0 - 1, h0)] if h0 else []
    f_end = min(h1, st.nf)
    chunk = max(1, min(ROUND_FRAMES, f_end - h0 if f_end > h0 else 1))
    return out + [(f, min(f + chunk, f_end)) for f in range(h0, f_end, chunk)]


# ----------------------------------------------------------------------------------------------------
# numpy model of the shipped algorithm, with single-edit mutations
# ----------------------------------------------------------------------------------------------------

_model_cache: dict = {}


_row_cache: dict = {}


def _model_unit(rows, mut):
    """Blocks of the live rows of one unit: k_imdct_plan + k_imdct_apply.  The union of the 8 lists is walked in
    ascending order, four entries per trip and then the tail; a row takes an entry unless its coefficient there
    is absent (bits 0).  The sum a row ends with depends on the entries it took, so it is kept per (row,
    entries taken): units that share rows share the work."""
    T, w, norm = O.tables()
    live = [isinstance(r, Row) for r in rows]
    C = np.stack([r.coefficients(mut) if l else np.zeros(HOP, F32) for r, l in zip(rows, live)])
    cut = 256 if mut == "first_256_pairs" else HOP
    idx = [r.idx[:cut] for g, (r, l) in enumerate(zip(rows, live)) if l and not (mut == "union_7_rows" and g == G - 1)]
    union = np.unique(np.concatenate(idx)) if idx else np.zeros(0, np.uint16)
    n_u = int(union.size)
    walk, j = [], 0
    while j + 4 <= n_u:                                      # four entries per trip
        walk += [int(union[j + e]) for e in range(4)]
        j += 4
    if mut != "drop_tail":
        walk += [int(union[e]) for e in range(j, n_u)]       # the 1..3-entry tail
    walk = np.array(walk, np.int64)
    present = C.view(np.uint32)[:, walk] != 0                # [8, entries]
    if mut == "pair_skip_either":
        present = np.repeat(present[0::2] & present[1::2], 2, axis=0)
    out = np.zeros((G, FRAME), F32)
    with np.errstate(all="ignore"):
        for g in range(G):
            if not live[g]:
                continue
            taken = walk[present[g]]
            key = (rows[g].key, mut, taken.tobytes())
            blk = _row_cache.get(key)
            if blk is None:
                acc = np.zeros(FRAME, F32)
                for k in taken.tolist():
                    acc = acc + C[g, k] * T[k]
                blk = _row_cache[key] = acc * (norm * w) if mut == "norm_times_window" else (acc * norm) * w
            out[g] = blk
    return out


def _deal(work: np.ndarray, mut) -> np.ndarray:
    """k_imdct_order: slot -> unit (-1: no unit was dealt to the slot)."""
    n = work.size
    u = np.arange(n)
    more = (work[None, :] > work[:, None]) | ((work[None, :] == work[:, None]) &
                                              ((u[None, :] <= u[:, None]) if mut == "rank_tie_le" else (u[None, :] < u[:, None])))
    rank = more.sum(axis=1)
    order = np.full(n + 1, -1)
    for unit, r in enumerate(rank.tolist()):
        pos = r
        if r < 1024:
            rnd, p = r >> 8, r & 255
            in_round = min(256, min(n, 1024) - (rnd << 8))
            pos = (rnd << 8) + (in_round - 1 - p if rnd & 1 else p)
        if pos < n:
            order[pos] = unit
    return order[:n]


def model_blocks(st: Stream, f0: int, f1: int, mut=None, variant=0, plan_groups=None) -> np.ndarray:
    """[(f1 - f0 + 8) * ch, 2048] as a launch over frames [f0, f1) leaves a sentinel-filled buffer (8 spare
    frames behind the range)."""
    ch, n = st.ch, f1 - f0
    out = sentinel(((n + G) * ch, FRAME)).copy()
    if n <= 0:
        return out
    pool_after = {}
    if mut == "raw_le":                                         # the sample behind each raw vector in the raw pool
        nxt = np.array([12345], np.int16)
        for f in range(st.nf - 1, -1, -1):
            if st.raw[f] is not None:
                pool_after[f] = nxt
                nxt = st.raw[f][:1] if st.raw[f].size else nxt
    for f in range(f0, f1):                                     # k_imdct_raw_rows
        if st.raw[f] is not None:
            for c in range(ch):
                out[(f - f0) * ch + c] = raw_block(st.raw[f], ch, c, mut, pool_after.get(f))
    umut = mut if mut in _UNIT_MUTATIONS else None
    for g0, n_fg in launch_batches(n, ch, plan_groups or plan_groups_of(st)):
        n_units = n_fg * ch
        units = [unit_rows(st, f0, f1, g0 + u // ch, u % ch) for u in range(n_units)]
        if 256 < n_units <= ORDER_MAX_UNITS and variant != 6:
            if variant == 5 and n_units % 256 == 0:
                rounds, order = n_units >> 8, np.full(n_units, -1)
                for u in range(n_units):
                    v = (u % ch) * n_fg + u // ch
                    order[(v % rounds) * 256 + v // rounds] = u
            else:
                order = _deal(np.array([unit_plan(r)["work"] for r in units]), mut)
        else:                                                   # natural order, channel rotated by the round
            order = np.array([(b // ch) * ch + (b - (b // ch) * ch + (((b // ch) * ch) >> 8)) % ch for b in range(n_units)])
        for u in order.tolist():
            if u < 0:
                continue
            rows = units[u]
            if mut == "past_end_live":
                rows = [EMPTY if r is None else r for r in rows]
            if not any(isinstance(r, Row) for r in rows):
                continue
            key = (umut, tuple(r.key if isinstance(r, Row) else r for r in rows))
            blk = _model_cache.get(key)
            if blk is None:
                blk = _model_cache[key] = _model_unit(rows, umut)
            fg, c = g0 + u // ch, u % ch
            for g, r in enumerate(rows):
                if isinstance(r, Row):
                    out[(fg * G + g) * ch + c] = blk[g]
    return out


def model_hops(st: Stream, h0: int, h1: int, mut=None) -> np.ndarray:
    """decode_hops_prepared: halo launch, rounds of <= 4096 frames through a ring whose slot 0 carries the frame
    in front of the round, the overlap-add of each round."""
    ch, nf = st.ch, st.nf
    if h1 <= h0:
        return np.zeros(0, F32)
    f_end = min(h1, nf)
    blocks = sentinel(((f_end - h0 + 2) * ch, FRAME)).copy()     # frames h0 - 1 .. f_end (one spare slot behind)
    for a, b in launches_of(st, Run("range", h0, h1)):
        blocks[(a - h0 + 1) * ch:(b - h0 + 1) * ch] = model_blocks(st, a, b, mut)[:(b - a) * ch]
    b3 = blocks.reshape(-1, ch, FRAME)
    out = np.empty((h1 - h0, HOP, ch), F32)
    with np.errstate(all="ignore"):
        for h in range(h0, h1):
            s = h - h0 + 1                                        # slot of frame h
            prev = b3[s - 1, :, HOP:] if h >= 1 or mut == "hop0_reads_prev" else np.zeros((ch, HOP), F32)
            out[h - h0] = (prev + b3[s, :, :HOP]).T if h < nf or mut == "tail_added" else prev.T
    return out.reshape(-1)


def model_run(st: Stream, run: Run, mut=None) -> np.ndarray:
    """The run's destination as the model leaves it: imdct runs include the 8 spare frames behind the range."""
    if run.kind == "imdct":
        return model_blocks(st, run.a, run.b, mut, run.variant).reshape(-1)
    if run.kind == "range":
        return model_hops(st, run.a, run.b, mut)
    return trim(st, model_hops(st, 0, st.nf + 1, mut))


def expected_model_run(st: Stream, run: Run) -> np.ndarray:
    """expected_run in the model's layout (sentinel frames behind an imdct range)."""
    e = expected_run(st, run)
    return np.concatenate([e, sentinel(G * st.ch * FRAME)]) if run.kind == "imdct" else e


# ----------------------------------------------------------------------------------------------------
# the families
# ----------------------------------------------------------------------------------------------------

def _q(rng, n):
    return (rng.integers(1, 20000, n) * rng.choice([-1, 1], n)).astype(np.int16)


def _scale(rng):
    return F32(rng.uniform(1e-3, 1.0))


def _indices(rng, n, edges=SCAN_EDGES):
    """n ascending bins: 1023 and 0 first, then the scan's boundaries, the rest at random."""
    first = [1023, 0] + [e for e in edges if e not in (0, 1023)]
    take = first[:min(n, len(first))]
    rest = np.setdiff1d(np.arange(HOP), take)
    return np.sort(np.concatenate([take, rng.permutation(rest)[:n - len(take)]]).astype(np.uint16))


def _palette(seed, n=40, max_len=40):
    rng = np.random.default_rng(seed)
    return [Row(np.sort(rng.permutation(HOP)[:int(L)]), _q(rng, int(L)), _scale(rng))
            for L in rng.integers(0, max_len + 1, n)]


def _pick(pal, *k):
    h = 0
    for x in k:
        h = (h * 1000003 + x * 7919 + 12345) & 0xFFFFFFFF
    return pal[h % len(pal)]


def _union_family():
    cases = []
    for shape in ("dense", "split"):
        rng = np.random.default_rng(101 + (shape == "split"))
        rows = []
        for n_u in UNION_SIZES:
            idx = _indices(rng, n_u)
            if shape == "dense":
                rows += [Row(idx, _q(rng, n_u), _scale(rng)) for _ in range(G)]
            else:
                owner = rng.permutation(G)[np.arange(n_u) % G]
                rows += [Row(idx[owner == g], _q(rng, int((owner == g).sum())), _scale(rng)) for g in range(G)]
        # a union of stored zeros only: n_u > 0 and every coefficient +0.0
        idx = _indices(rng, 6)
        rows += [Row(idx if shape == "dense" else idx[g % 6:g % 6 + 1], np.zeros(6 if shape == "dense" else 1, np.int16),
                     _scale(rng)) for g in range(G)]
        st = Stream(44100, 1, rows)
        cases.append(Case(f"union-{shape}", "union", st, [Run("imdct", 0, st.nf), Run("decode")],
                          how="nested" if shape == "dense" else "bytes", info=dict(shape=shape, zero_group=len(UNION_SIZES))))
    return cases


def _lists_family():
    rng = np.random.default_rng(202)
    full = [Row(np.arange(HOP), _q(rng, HOP), _scale(rng)) for _ in range(G - 1)]
    rows, marks = [], []       # marks: (group, position, length, neighbours)

    def group(long_row, pos, others):
        g = [None] * G
        g[pos] = long_row
        it = iter(others)
        marks.append((len(rows) // G, pos, len(long_row), "full" if others is full else "empty"))
        rows.extend(r if r is not None else next(it) for r in g)

    for i, L in enumerate(LIST_LENGTHS):
        group(Row(_indices(rng, L), _q(rng, L), _scale(rng)), i % G, [EMPTY] * (G - 1))
        group(Row(_indices(rng, L), _q(rng, L), _scale(rng)), (i + 3) % G, full)
    for pos in range(G):
        group(Row(_indices(rng, 257), _q(rng, 257), _scale(rng)), pos, full)
        group(Row(_indices(rng, 513), _q(rng, 513), _scale(rng)), pos, [EMPTY] * (G - 1))
    st = Stream(48000, 1, rows)
    return [Case("lists", "lists", st, [Run("imdct", 0, st.nf), Run("decode")], how="parts", info=dict(marks=marks))]


def _group_runs(nf):
    runs = [Run("imdct", 0, nf), Run("decode")]
    for s in RANGE_STARTS:
        if s < nf:
            runs += [Run("imdct", s, nf), Run("imdct", s, s + 1)]
    return runs


def _raw_vec(rng, ch, n=None):
    n = FRAME * ch if n is None else n
    v = rng.integers(-32768, 32768, n).astype(np.int16)
    if n:
        v[0] = v[0] or 1
    return v


def _groups_family():
    pal = _palette(303)
    cases = []
    shapes = [(1, nf) for nf in GROUP_FRAMES] + [(2, 9), (2, 13), (2, 17), (3, 7), (3, 16), (5, 1), (5, 15), (8, 8), (8, 17)]
    for ch, nf in shapes:
        st = Stream(44100, ch, [_pick(pal, ch, nf, m) for m in range(nf * ch)])
        cases.append(Case(f"groups-ch{ch}-nf{nf}", "groups", st, _group_runs(nf), how=("bytes", "nested", "parts")[(ch + nf) % 3]))
    for ch in (1, 3, 8):      # group g < 8: one raw frame at position g; group 8: all raw; group 9: all but one; 3 more frames
        nf = 10 * G + 3
        rng = np.random.default_rng(310 + ch)
        raw_at = {g * G + g for g in range(G)} | set(range(8 * G, 9 * G)) | (set(range(9 * G, 10 * G)) - {9 * G + 5})
        st = Stream(48000, ch, [_pick(pal, ch, 99, m) for m in range(nf * ch)],
                    [_raw_vec(rng, ch) if f in raw_at else None for f in range(nf)])
        cases.append(Case(f"groups-rawpos-ch{ch}", "groups", st, _group_runs(nf), how=("bytes", "parts")[ch % 2]))
    for ch in (2, 5):         # raw frames only in the partial last group
        nf = G + 3
        rng = np.random.default_rng(320 + ch)
        st = Stream(48000, ch, [_pick(pal, ch, 77, m) for m in range(nf * ch)],
                    [_raw_vec(rng, ch) if f >= G + 1 else None for f in range(nf)])
        cases.append(Case(f"groups-rawlast-ch{ch}", "groups", st, _group_runs(nf), how="nested"))
    return cases


def _raw_family():
    pal = _palette(404, n=6)
    cases = []
    for ch in RAW_CHANNELS:
        rng = np.random.default_rng(400 + ch)
        lengths = [0, 1, ch, FRAME * ch - 1, FRAME * ch, FRAME * ch + 1]
        specials = np.tile(np.array(RAW_VALUES, np.int16), FRAME * ch // len(RAW_VALUES) + 1)[:FRAME * ch]
        raws = [None] + [_raw_vec(rng, ch, n) for n in lengths] + [None, specials]
        if ch == RAW_CHANNELS[-1]:      # every int16 once, in order, over as many frames as that takes
            ramp = np.arange(-32768, 32768).astype(np.int16)
            ramp = np.concatenate([ramp, ramp[:(-ramp.size) % (FRAME * ch)]])
            raws += list(ramp.reshape(-1, FRAME * ch))
        raws += [_raw_vec(rng, ch)]
        nf = len(raws)
        st = Stream(44100, ch, [_pick(pal, ch, m) for m in range(nf * ch)], raws)
        cases.append(Case(f"raw-ch{ch}", "raw", st, [Run("imdct", 0, nf), Run("decode"), Run("range", 0, nf + 1)],
                          how=("bytes", "parts", "nested")[ch % 3], info=dict(lengths=lengths)))
    return cases


def _values_family():
    rng = np.random.default_rng(505)
    idx = np.array([0, 5, 300, 777, 1023], np.uint16)
    rows, names = [], []
    for s in SCALES:
        rows.append(Row(idx, np.array(Q_VALUES, np.int16), s))
        names.append(f"scale {s!r}")
    rows.append(Row([3, 9], [0, 100], 0.25)), names.append("stored zero, finite scale")
    rows.append(Row([3, 9], [0, 100], np.inf)), names.append("stored zero, infinite scale")
    rows.append(Row([3], [0], np.inf)), names.append("only a stored zero, infinite scale")
    for qv in Q_VALUES:
        n = 40
        rows.append(Row(_indices(rng, n), np.full(n, qv, np.int16), 1.0)), names.append(f"q {qv}")
    rows += [EMPTY] * ((-len(rows)) % G)
    st = Stream(44100, 1, rows)
    return [Case("values", "values", st, [Run("imdct", 0, st.nf), Run("decode")], info=dict(names=names))]


def _placement_rows(kind):
    """row(unit, g): `ties` - every unit one index, 8 pairs, work 9, neighbouring units different in index and
    q; `alldiff` - lists are prefixes of one index sequence, unit k holds (k % 8) rows of k // 8 + 1 pairs and the
    rest of k // 8, so that work = total + n_u is different for every k < 2048."""
    rng = np.random.default_rng(606)
    if kind == "ties":
        idx = rng.permutation(HOP)[:7]
        pal = [[Row([i], [q], F32(0.5)) for q in (-7, 11, 300, -20000, 5)] for i in idx]
        return lambda u, g: pal[u % 7][(u // 7 + g) % 5]
    seq, q = np.sort(rng.permutation(HOP)[:257]), _q(rng, 257)
    pal = [Row(seq[:L], q[:L], F32(0.75)) for L in range(258)]
    step = 1237                                                  # odd: u -> k is a bijection of 0..2047
    return lambda u, g: pal[((u * step + 11) % PLAN_GROUPS) // G + (1 if g < ((u * step + 11) % PLAN_GROUPS) % G else 0)]


def _placement_family():
    cases = []
    for kind in ("ties", "alldiff"):
        shapes = [(u, PLACEMENT_SHAPES[u], u // PLACEMENT_SHAPES[u] * G) for u in PLACEMENT_UNITS] + \
                 [((TWO_BATCH[1] + G - 1) // G * TWO_BATCH[0],) + TWO_BATCH]
        for units, ch, nf in shapes:
            row = _placement_rows(kind)
            st = Stream(48000, ch, [row((f // G) * ch + c, f % G) for f in range(nf) for c in range(ch)])
            runs = [Run("imdct", 0, nf)]
            if kind == "alldiff" and units in (1023, 1025):
                runs.append(Run("imdct", 0, nf, variant=6))     # natural order, rotated channel; 256 % ch != 0
            if kind == "alldiff" and units in (1024, 2048):
                runs.append(Run("imdct", 0, nf, variant=5))     # consecutive groups of one channel share a CU
            cases.append(Case(f"placement-{kind}-{units}", "placement", st, runs, how="records" if units % 2 else "bytes",
                              info=dict(kind=kind, units=units)))
    return cases


def _reuse_family():
    pal_a, pal_b = _palette(707, max_len=30), None
    rng = np.random.default_rng(708)
    pal_b = [Row(r.idx, -r.q, _scale(rng)) for r in pal_a]      # same shape and pool sizes, other content
    ch, nf = 2, 20
    rng = np.random.default_rng(709)
    raw = [_raw_vec(rng, ch) if f == 13 else None for f in range(nf)]
    a = Stream(44100, ch, [_pick(pal_a, m) for m in range(nf * ch)], raw)
    b = Stream(44100, ch, [_pick(pal_b, m) for m in range(nf * ch)], [None if r is None else (r ^ 0x55) for r in raw])
    steps = [("a", Run("imdct", 0, nf)), ("a", Run("imdct", 0, nf)),             # the second one keeps the plan
             ("a", Run("imdct", 3, 17)), ("a", Run("imdct", 0, nf)),             # another range, the first again
             ("a", Run("imdct", 0, nf, variant=2)), ("a", Run("imdct", 0, nf)),  # another variant and back
             ("b", Run("imdct", 0, nf)), ("b", Run("imdct", 0, nf)),             # another stream of the same shape
             ("a", Run("imdct", 0, nf)),
             ("a", Run("range", 5, 6)), ("a", Run("imdct", 4, 5)),               # halo launch (M = ch), then one frame
             ("a", Run("range", 5, 6)), ("b", Run("range", 5, 6)), ("b", Run("imdct", 4, 5)),
             ("a", Run("decode")), ("a", Run("decode")), ("b", Run("decode"))]
    return [Case("reuse", "reuse", a, [r for s, r in steps if s == "a"], info=dict(other=b, steps=steps))]


def _overlap_family():
    pal = _palette(808)
    cases = []
    for i, ch in enumerate(OVERLAP_CHANNELS):
        nf = 5
        rng = np.random.default_rng(800 + ch)
        st = Stream(48000, ch, [_pick(pal, ch, m) for m in range(nf * ch)], [_raw_vec(rng, ch) if f == 2 else None for f in range(nf)])
        runs = [Run("range", 0, nf + 1, off) for off in OFFSETS]
        for j, (a, b) in enumerate([(0, 1), (nf, nf + 1), (nf - 1, nf + 1), (2, 2), (1, 3)]):
            runs.append(Run("range", a, b, OFFSETS[(i + j) % 4]))
        cases.append(Case(f"overlap-ch{ch}", "overlap", st, runs + [Run("decode")], how=("bytes", "nested")[ch % 2]))
    nf = LONG_FRAMES                  # longer than one decode round: ranges that end at / cross frames 4095..4097
    st = Stream(48000, 1, [_pick(pal, 1, m) for m in range(nf)])
    R = ROUND_FRAMES
    runs = [Run("range", 0, R - 1), Run("range", 0, R, 4), Run("range", 0, R + 1, 8), Run("range", 1, R + 2, 12),
            Run("range", R - 2, R + 1), Run("range", 3, nf + 1), Run("decode")]
    cases.append(Case("overlap-long", "overlap", st, runs, how="parts"))
    return cases


def build_cases():
    return (_union_family() + _lists_family() + _groups_family() + _raw_family() + _values_family() +
            _placement_family() + _reuse_family() + _overlap_family())


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
    return _cases


def digest(cs) -> str:
    h = hashlib.sha256()
    for c in cs:
        h.update(c.name.encode() + c.how.encode() + repr(c.runs).encode())
        h.update(hashlib.sha256(c.stream.to_glc()).digest())
        if "other" in c.info:
            h.update(hashlib.sha256(c.info["other"].to_glc()).digest())
    return h.hexdigest()
