"""Models and inputs for the streaming encode (glc_plan_stream_push, glc_stream_enc_*; test helper: numpy only).

The geometry, restated from the reference's frame loop (src/codec.rs:433-474) and from nothing else: frame f of a stream
reads the per-channel samples [1024 f - 512, 1024 f + 1536), so it is final once 1024 f + 1536 samples are there.  The
model below counts frames one by one; the library has closed forms.
"""
from __future__ import annotations

import numpy as np

HOP, FRAME = 1024, 2048
SR = 48000
S16, S32, PF32 = 1, 2, 3


def frames_done(received: int) -> int:
    """Frames of a stream that are final after `received` samples per channel, counted one by one."""
    f = 0
    while HOP * f + FRAME - HOP // 2 <= received:
        f += 1
    return f


def model_plan(received: int, n_new: int, finish: bool, num_frames):
    """(first_frame, n_frames, carry) of a push, or None where a finish must be refused.  num_frames(L, 1): the
    oracle's frame count of a mono stream of L samples (0: the reference panics)."""
    done0, total = frames_done(received), received + n_new
    if finish:
        nf = num_frames(total, 1)
        return None if nf == 0 else (done0, nf - done0, 0)
    done1 = frames_done(total)
    held_from = HOP * done1 - HOP // 2 if done1 else 0
    return done0, done1 - done0, total - held_from


def random_chunking(rng, total: int, biggest: int, zeros: float = 0.15):
    """Chunk sizes (some 0) that add up to `total`."""
    out, left = [], total
    while left:
        n = 0 if rng.random() < zeros else int(min(left, rng.integers(1, biggest + 1)))
        out.append(n)
        left -= n
    return out


def fixed_chunking(total: int, size: int):
    return [min(size, total - at) for at in range(0, total, size)]


def boundary_chunking(total: int, delta: int):
    """Pushes that end `delta` samples off every frame's completion point 1024 f + 1536."""
    cuts = [c for c in (HOP * f + FRAME - HOP // 2 + delta for f in range(total // HOP + 1)) if 0 < c < total]
    edges = [0] + cuts + [total]
    return [b - a for a, b in zip(edges, edges[1:])]


def widen(x: np.ndarray, bits: int) -> np.ndarray:
    """The reference's loaders: `s as f32 / (1 << (bits - 1)) as f32`, the 32-bit shift going into the sign (Q11)."""
    mx = np.float32(-2147483648.0) if bits == 32 else np.float32(1 << (bits - 1))
    return (x.astype(np.float32) / mx).astype(np.float32)


def to_int(x: np.ndarray, fmt: int, bits: int) -> np.ndarray:
    """Float samples in [-1, 1) as `bits`-bit integers in their container."""
    dt = np.int16 if fmt == S16 else np.int32
    full = float(1 << (bits - 1))
    return np.clip(np.round(x.astype(np.float64) * full), -full, full - 1).astype(dt)


def np_dtype(fmt: int):
    return {S16: np.int16, S32: np.int32, PF32: np.float32}[fmt]


def padding_value(fmt: int):
    """What the layout's padding holds: NaN for floats, a full-scale integer otherwise."""
    return {S16: np.int16(-32768), S32: np.int32(-2 ** 31), PF32: np.float32(np.nan)}[fmt]


class Layout:
    """A flat host array in which lane i's chunk of `lens[i]` samples per channel lies as a glc_clip_layout says:
    `off` elements in front, odd strides, everything outside the chunks holding padding_value."""

    def __init__(self, ch: int, lens, planar: bool, fmt: int, off: int = 0, slack: int = 3):
        self.ch, self.lens, self.planar, self.fmt, self.off = ch, [int(v) for v in lens], planar, fmt, off
        longest = max(self.lens + [1])
        if planar and ch > 1:
            self.channel_stride = longest + slack
            self.clip_stride = self.channel_stride * ch + slack + 2
        else:
            self.channel_stride = 0
            self.clip_stride = longest * ch + slack
        if self.clip_stride % 2 == 0:
            self.clip_stride += 1                     # odd: the lanes start at every residue of a vector of four
        self.size = off + self.clip_stride * len(self.lens) + 5
        self.flat = np.full(self.size, padding_value(fmt), np_dtype(fmt))

    def put(self, i: int, chunk: np.ndarray):
        """chunk: interleaved samples of lane i, lens[i] * ch of them."""
        n, ch = self.lens[i], self.ch
        assert chunk.size == n * ch
        base = self.off + i * self.clip_stride
        if self.planar and ch > 1:
            planes = chunk.reshape(n, ch).T
            for c in range(ch):
                self.flat[base + c * self.channel_stride: base + c * self.channel_stride + n] = planes[c]
        else:
            self.flat[base: base + n * ch] = chunk
