"""Models and inputs for the streaming decode (glc_plan_stream_dec_push, glc_stream_dec_*; test helper: numpy only).

The geometry, restated from the reference's decoder (src/codec.rs:595-765) and from nothing else: a stream of L samples
per channel has nf frames, 1024 nf - 511 <= L <= 1024 nf + 512; its un-trimmed output is nf + 1 hops of 1024 * ch
interleaved samples, hop h = second half of frame h - 1 + first half of frame h; the trim keeps the interleaved
positions [512, 512 + L * ch), so decoded sample t of channel c lies at position 512 + t * ch + c.  A receiver that has
D frames knows hops 0 .. D - 1 for good and does not know L: it may emit per-channel samples below 1024 D - 512 and no
more, because a stream that ends with frame D can be as short as 1024 D - 511.
"""
from __future__ import annotations

import numpy as np

HOP, FRAME = 1024, 2048
SR = 48000
S16, PF32 = 1, 3
NO_BLOB, BAD_HEADER, NOT_CANONICAL = 64, 1, 4


def num_frames(L: int) -> int:
    """Frames of a mono stream of L samples (0: the reference panics), counted one by one: the padded stream is 512
    zeros, the samples, zeros up to a multiple of 1024, and 512 more; frames start every 1024."""
    if L <= 512:
        return 0
    padded = -(-(512 + L) // HOP) * HOP + 512
    f = 0
    while HOP * f + FRAME <= padded:
        f += 1
    return f


def emitted(done: int) -> int:
    return max(0, HOP * done - HOP // 2)


def model_plan(done: int, n: int, finish: bool, total_len: int):
    """(first_sample, n_samples) of a push, or None where it must be refused."""
    if finish:
        if num_frames(total_len) != done + n or done + n == 0:
            return None
        return emitted(done), total_len - emitted(done)
    return emitted(done), emitted(done + n) - emitted(done)


def chunkings(nf: int, rng):
    """Frame counts of the pushes of a stream of nf frames: 1 per push, 2 per push, all at once, random."""
    out = [[1] * nf, [2] * (nf // 2) + [1] * (nf % 2), [nf]]
    left, r = nf, []
    while left:
        k = int(rng.integers(1, left + 1))
        r.append(k)
        left -= k
    out.append(r)
    return out


def compact_blob(ch: int, n_frames: int, cnt=None, pairs=None, scale=None) -> bytes:
    """A valid compact blob of n_frames compressed frames (include: header 64 B | is_raw u8[nf] | scale f32[M] |
    cnt u32[M] | pairs u32[n_pairs], every section 64-byte aligned); all rows empty lists of scale 0 by default."""
    a64 = lambda v: (v + 63) // 64 * 64
    M = n_frames * ch
    cnt = np.zeros(M, np.uint32) if cnt is None else np.asarray(cnt, np.uint32)
    pairs = np.zeros(0, np.uint32) if pairs is None else np.asarray(pairs, np.uint32)
    scale = np.zeros(M, np.float32) if scale is None else np.asarray(scale, np.float32)
    o_israw = 64
    o_scale = o_israw + a64(n_frames)
    o_cnt = o_scale + a64(4 * M)
    o_pairs = o_cnt + a64(4 * M)
    total = a64(o_pairs + 4 * pairs.size)
    b = np.zeros(total, np.uint8)
    hdr = np.zeros(8, np.uint64)
    hdr[0] = 0x42434C47 | (ch << 32)
    hdr[1], hdr[2], hdr[3], hdr[4] = n_frames, pairs.size, 0, total
    b[:64] = hdr.view(np.uint8)
    b[o_scale:o_scale + 4 * M] = scale.view(np.uint8)
    b[o_cnt:o_cnt + 4 * M] = cnt.view(np.uint8)
    b[o_pairs:o_pairs + 4 * pairs.size] = pairs.view(np.uint8)
    return b.tobytes()


def header_frames(blob: bytes) -> int:
    return int(np.frombuffer(blob[:64], np.uint64)[1])


def with_header_frames(blob: bytes, n: int) -> bytes:
    h = np.frombuffer(blob[:64], np.uint64).copy()
    h[1] = n
    return h.tobytes() + blob[64:]


def with_magic_flipped(blob: bytes) -> bytes:
    return bytes([blob[0] ^ 0xFF]) + blob[1:]
