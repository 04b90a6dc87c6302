"""Virtual record streams for the per-clip pack A1-A3 (k_store_scan_rows / k_store_place / k_store_rows,
csrc/glc_kernels.hip) and the model of what glc_encode_batch_device_compact must leave in its arena (test helper:
numpy only, built on tests/compact_edges.py).

The store: the blob of clip i is the single-stream compact blob of the clip's own frames -
`compact_edges.model(take_frames(virtual, frames of clip i))`, no directory, padding zeroed - and the device places
the blobs itself:

  start  = cursor rounded up to 64
  offset = start + the sizes of the clips in front (every size is a multiple of 64)
  stored = offset + bytes <= arena_bytes; the running sum counts a clip whether or not it was stored
  cursor = start + the sizes of ALL clips

`store_model(..., mutation)` restates that with one rule changed (MUTATIONS): tests/test_compact_store.py shows
that every such edit changes the expected arena, entries or cursor of at least one case below.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import compact_edges as E

HOP, FRAME = E.HOP, E.FRAME
SENTINEL = E.SENTINEL

MUTATIONS = ("pairs_not_restarted", "junk_frame_counted", "gap_not_zeroed", "cursor_not_rounded", "overflow_stored_anyway",
             "cursor_stops_at_overflow")


def align64(v: int) -> int:
    return (v + 63) // 64 * 64


@dataclass
class Case:
    name: str
    desc: E.Desc                 # the virtual stream: clip i's frames, one junk record behind each clip
    clip_frames: tuple
    cursor0: int = 0
    cut: object = None           # arena_bytes = the bytes needed + cut (None: a roomy arena)


# ----------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------

def clip_descs(d_virtual: E.Desc, clip_frames, mutation=None):
    """The description of every clip's records as a range of its own."""
    out, slot = [], 0
    for n in clip_frames:
        out.append(E.take_frames(d_virtual, np.arange(slot, slot + n)))
        slot += n + (0 if mutation == "junk_frame_counted" else 1)
    return out


def _gaps(ch, nf, n_pairs):
    o_israw, o_scale, o_cnt, o_pairs, _ = E.layout(ch, nf)
    m = nf * ch
    return ((o_israw + nf, o_scale), (o_scale + 4 * m, o_cnt), (o_cnt + 4 * m, o_pairs), (o_pairs + 4 * n_pairs, align64(o_pairs + 4 * n_pairs)))


def clip_blobs(d_virtual: E.Desc, clip_frames, mutation=None):
    """[(blob uint8, n_pairs, n_raw_rows)] per clip."""
    out, pairs_before = [], 0
    for d in clip_descs(d_virtual, clip_frames, mutation):
        blob, (nf, n_pairs, n_raw, total) = E.model(d)
        blob = blob.copy()
        if mutation == "gap_not_zeroed":
            for a, b in _gaps(d.ch, nf, n_pairs):
                blob[a:b] = SENTINEL
        if mutation == "pairs_not_restarted" and pairs_before:
            o_pairs = E.layout(d.ch, nf)[3]
            sec = blob[o_pairs:o_pairs + 4 * n_pairs].view(np.uint32)
            moved = np.full(n_pairs, 0xABABABAB, np.uint32)
            keep = max(n_pairs - pairs_before, 0)
            moved[n_pairs - keep:] = sec[:keep]       # the lists land pairs_before places further on; what leaves the section is lost
            sec[:] = moved
        pairs_before += n_pairs
        out.append((blob, n_pairs, n_raw))
    return out


def store_model(d_virtual: E.Desc, clip_frames, cursor0: int, arena_bytes: int, mutation=None, blobs=None):
    """-> (entries [(offset, bytes, n_pairs, n_raw_rows, stored)], blobs [uint8], final cursor)."""
    assert mutation is None or mutation in MUTATIONS
    blobs = clip_blobs(d_virtual, clip_frames, mutation) if blobs is None else blobs
    at = cursor0 if mutation == "cursor_not_rounded" else align64(cursor0)
    entries, stopped = [], False
    for blob, n_pairs, n_raw in blobs:
        fits = at + blob.size <= arena_bytes
        stored = fits or mutation == "overflow_stored_anyway"
        entries.append((at, blob.size, n_pairs, n_raw, int(stored)))
        if mutation == "cursor_stops_at_overflow" and not fits:
            stopped = True
        if not stopped:
            at += blob.size
    return entries, [b for b, _, _ in blobs], at


def arena_image(size: int, entries, blobs, image=None) -> np.ndarray:
    """The arena after the call: the stored blobs over the prefill (`image`, or SENTINEL bytes)."""
    img = np.full(size, SENTINEL, np.uint8) if image is None else image.copy()
    for (off, n, _, _, stored), blob in zip(entries, blobs):
        if stored:
            hi = min(off + n, size)           # a mutated rule may store what does not fit
            img[off:hi] = blob[:hi - off]
    return img


def entry_rows(entries) -> np.ndarray:
    """The entries as the (n, 4) int64 view of the structs: offset, bytes, n_pairs, n_raw_rows | stored << 32."""
    return np.array([[o, b, p, r | (s << 32)] for o, b, p, r, s in entries], np.int64).reshape(-1, 4)


# ----------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------

def _build(ch, clips, kind_of, junk_of, seed, hi=6):
    """kind_of(i, f): "sparse" | "raw" | "silent" | "over" | "under"; junk_of(i): "dense" | "rawflag"."""
    rng = np.random.default_rng(seed)
    b = E.Builder(ch, sum(clips) + len(clips))
    slot = 0
    for i, n in enumerate(clips):
        for f in range(n):
            v = slot + f
            kind = kind_of(i, f)
            if kind == "raw":
                b.raw(v, E.FLAG_WORDS[v % 4], E._plane(rng, ch), nnz=(7 if v % 2 else None))
                for c in range(ch):
                    b.scale_bits[v * ch + c] = int(rng.integers(0, 1 << 32))   # the quantiser's scale stays
            elif kind == "silent":
                for c in range(ch):
                    b.row(v * ch + c, [], [], scale=0)
            elif kind in ("over", "under"):
                for c in range(ch):
                    true = int(rng.integers(2, 70))
                    ks = np.sort(rng.choice(HOP, true, replace=False))
                    b.row(v * ch + c, ks, E._q(rng, true), nnz=true + 9 if kind == "over" else true - 2, scale=int(rng.integers(0, 1 << 32)))
            else:
                E._sparse_rows(b, rng, range(v * ch, (v + 1) * ch), hi)
        E._junk(b, rng, slot + n, junk_of(i))
        slot += n + 1
    return b.desc()


_alt = lambda i: "rawflag" if i % 2 == 0 else "dense"


def build_cases():
    out = []
    sparse = lambda i, f: "sparse"
    out.append(Case("one-clip-one-frame", _build(2, [1], sparse, _alt, 8101), (1,)))
    out.append(Case("three-one-frame-clips", _build(1, [1, 1, 1], lambda i, f: "raw" if i == 1 else "sparse", _alt, 8102), (1, 1, 1), cursor0=64))
    edge = [3, 1, 64, 65]                             # 64 frames: no gap behind the raw flags; 65: a gap of 63 bytes
    for ch, cur in ((1, 0), (2, 100), (3, 1), (6, 4160)):   # 4 M mod 64 varies; cursors that are no multiple of 64
        kind = lambda i, f: "raw" if (i == 0 and f in (0, 2)) or (i == 3 and f == 64) or (i == 2 and f == 0) else "sparse"
        out.append(Case(f"edges-ch{ch}", _build(ch, edge, kind, _alt, 8110 + ch, hi=4), tuple(edge), cursor0=cur))
    out.append(Case("all-raw-and-silent", _build(2, [2, 3, 2, 1], lambda i, f: ("raw", "silent", "sparse", "silent")[i], lambda i: "dense", 8120),
                    (2, 3, 2, 1), cursor0=63))
    out.append(Case("nnz-disagrees", _build(2, [2, 2, 1], lambda i, f: ("over", "under", "over")[(i + f) % 3], _alt, 8130), (2, 2, 1), cursor0=65))
    out.append(Case("clip-across-a-scan-block", _build(1, [5, 1030, 3], lambda i, f: "raw" if f % 211 == 3 else "sparse", _alt, 8140, hi=4),
                    (5, 1030, 3), cursor0=7))
    out.append(Case("clip-of-1200-rows-ch3", _build(3, [400, 2], lambda i, f: "raw" if f in (0, 399) else "sparse", lambda i: "dense", 8141, hi=3),
                    (400, 2)))
    out.append(Case("1100-mono-clips", _build(1, [1] * 1100, lambda i, f: "raw" if i % 97 == 5 else ("silent" if i % 89 == 1 else "sparse"), _alt, 8150),
                    (1,) * 1100, cursor0=200))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
    return _cases


def case(name) -> Case:
    return next(c for c in cases() if c.name == name)
