"""Integer PCM on the device batch and store paths (tests/test_store_int_model.py, tests/test_store_int.py): the two
rules restated in numpy, the integer case set, and builders of strided batches.  numpy only - nothing here loads
the library under test.

  widen   load_wav / load_flac, src/audio.rs:52-60, :72-81:  s as f32 / (1 << (bits - 1)) as f32
          (the literal is an i32: at 32 bits the divisor is i32::MIN, quirk Q11)
  narrow  convert_f32_to_i16, src/audio.rs:11-16:  (s * 32767.0).clamp(-32768.0, 32767.0) as i16
          - NaN gives 0, truncation toward zero (the rule of tests/test_int_pcm.py, restated here)

A batch is ONE flat array of the sample type with the clips at `off + i * clip_stride` (elements); everything that is
not a true sample of a clip is filled with full-scale integers of alternating sign - integers have no NaN, so a read
outside a clip has to change bytes - or, on the output side, with the sentinel 0x5A5A."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

HOP, FRAME = 1024, 2048
F32 = np.float32
S16, S32, PF32 = 1, 2, 3                       # glc_pcm_format
SR = 48000
SENTINEL = 0x5A5A

# (format, bits): the encode families
FORMATS = ((S16, 16), (S16, 12), (S32, 24), (S32, 32))
CHANNELS = (1, 2, 3, 4, 6, 8)
# samples per channel: a last hop that is empty, nearly empty and full
LENGTHS = (513, 1023, 1024, 1025, 1535, 2049)


def np_dtype(fmt):
    return {S16: np.int16, S32: np.int32, PF32: np.float32}[fmt]


def widen(s, bits):
    mx = F32(-2147483648.0) if bits == 32 else F32(1 << (bits - 1))
    return np.asarray(s).astype(F32) / mx


def narrow(x):
    with np.errstate(all="ignore"):
        v = np.asarray(x, F32) * F32(32767.0)
    v = np.where(np.isnan(v), F32(0.0), v)
    return np.trunc(np.clip(v, F32(-32768.0), F32(32767.0))).astype(np.int16)


def int_range(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


# ------------------------------------------------------------------------------------------ signals

def _lcg(n, seed):
    """Uniform noise in [-1, 1) from a 32-bit LCG (Numerical Recipes constants): no structure a tonal model could keep."""
    s = np.empty(n, np.uint64)
    x = np.uint64(seed & 0xFFFFFFFF)
    a, c, m = np.uint64(1664525), np.uint64(1013904223), np.uint64(0xFFFFFFFF)
    for i in range(n):
        x = (a * x + c) & m
        s[i] = x
    return s.astype(np.float64) / 2147483648.0 - 1.0


_noise = {}


def noise(n, seed):
    key = seed
    if key not in _noise or _noise[key].size < n:
        _noise[key] = _lcg(max(n, 1 << 15), seed)
    return _noise[key][:n]


def chord(ch, per_channel, seed, amp=0.04, n_tones=12):
    rng = np.random.RandomState(seed)
    t = np.arange(per_channel, dtype=np.float64) / SR
    out = np.zeros((per_channel, ch), np.float64)
    for c in range(ch):
        for f, p in zip(rng.uniform(80.0, 8000.0, n_tones), rng.uniform(0, 2 * np.pi, n_tones)):
            out[:, c] += amp * np.sin(2 * np.pi * f * t + p)
    return out


def signal(ch, per_channel, index):
    """Clip `index` of a family as float64 (per_channel, ch) in about [-0.6, 0.6]: even clips a chord (compressed
    frames), odd clips noise for their first hop and a chord behind it (a raw frame, then compressed ones)."""
    x = chord(ch, per_channel, seed=11 + index)
    if index % 2:
        n = min(per_channel, HOP + 300)
        x[:n] = 0.6 * noise(n * ch, seed=5 + index).reshape(n, ch)
    return x


_SPECIAL = ("min", "max", 0, 1, -1)


def int_clip(fmt, bits, ch, per_channel, index):
    """Clip `index` as integers of `bits` bits in the container of `fmt`, shape (per_channel, ch): the signal
    rounded to the range, with INT_MIN / INT_MAX / 0 / +1 / -1 of that range in the first and the last sample of
    every channel (which of the five rotates with the clip and the channel)."""
    lo, hi = int_range(bits)
    x = np.clip(np.rint(signal(ch, per_channel, index) * (hi + 1.0)), lo, hi).astype(np.int64)
    pick = lambda k: {"min": lo, "max": hi}.get(_SPECIAL[k % 5], _SPECIAL[k % 5])
    for c in range(ch):
        x[0, c] = pick(index + c)
        x[-1, c] = pick(index + c + 2)
    return x.astype(np_dtype(fmt))


def family_clips(fmt, bits, ch, lengths=LENGTHS):
    return [int_clip(fmt, bits, ch, n, i) for i, n in enumerate(lengths)]


def loud_clip(ch, per_channel, index):
    """A float clip for the narrowing cases: a chord whose peaks pass +-1.0 by a wide margin (the decode clamps at both
    rails) and whose body lies inside them."""
    x = chord(ch, per_channel, seed=31 + index, amp=0.16, n_tones=12)
    return x.astype(F32)


# ------------------------------------------------------------------------------------------ strided batches

def odd(v):
    return v | 1


@dataclass
class Batch:
    flat: np.ndarray          # everything, `off` elements of filler in front
    mask: np.ndarray          # bool, the clips' true samples
    off: int                  # the batch's first element
    ch: int
    planar: bool
    clip_stride: int
    channel_stride: int
    lengths: tuple
    index: list               # per clip the flat indices of its samples in INTERLEAVED order (t * ch + c)

    @property
    def n_clips(self):
        return len(self.lengths)

    def gather(self, flat, i):
        return flat[self.index[i]]


def geometry(lengths, ch, planar, off, pad=5):
    """Odd strides, a few elements of slack between planes and between clips, `off` elements in front and 8 behind."""
    t = max(lengths)
    planes = planar and ch > 1
    chs = odd(t + 3) if planes else 0
    occ = (ch - 1) * chs + t if planes else t * ch
    cs = odd(occ + pad)
    size = off + (len(lengths) - 1) * cs + occ + 8
    index = []
    for i, n in enumerate(lengths):
        base = off + i * cs
        tt, cc = np.meshgrid(np.arange(n), np.arange(ch), indexing="ij")
        index.append((base + cc * chs + tt if planes else base + tt * ch + cc).reshape(-1))
    return cs, chs, size, index


def filler(n, dtype):
    """Full scale, alternating sign."""
    info = np.iinfo(dtype)
    a = np.empty(n, dtype)
    a[0::2], a[1::2] = info.max, info.min
    return a


def input_batch(clips, ch, planar, off, dtype):
    """Integer clips of shape (len_i, ch) in a flat array of full-scale filler."""
    lengths = tuple(c.shape[0] for c in clips)
    cs, chs, size, index = geometry(lengths, ch, planar, off)
    flat = filler(size, dtype)
    mask = np.zeros(size, bool)
    for c, ix in zip(clips, index):
        flat[ix] = np.asarray(c, dtype).reshape(-1)
        mask[ix] = True
    assert mask.sum() == sum(c.size for c in clips)
    return Batch(flat, mask, off, ch, planar, cs, chs, lengths, index)


def output_batch(lengths, ch, planar, off, dtype=np.int16, pad=5):
    """An output of the given clip lengths: the sentinel everywhere (as bits, for a float output too)."""
    cs, chs, size, index = geometry(tuple(lengths), ch, planar, off, pad)
    flat = np.full(size, SENTINEL, np.uint16).astype(np.int16) if dtype == np.int16 else \
        np.full(size, 0x7FC05A5A, np.uint32).view(F32)
    mask = np.zeros(size, bool)
    for ix in index:
        mask[ix] = True
    return Batch(flat, mask, off, ch, planar, cs, chs, tuple(lengths), index)


def crop_set(length):
    """(start, L) for L in 1, 2, 3, 4, 5, 1023, 1024, 1025 at starts 0, 511, 512, 513 and length - L."""
    out = []
    for L in (1, 2, 3, 4, 5, 1023, 1024, 1025):
        for s in (0, 511, 512, 513, length - L):
            assert 0 <= s and s + L <= length
            out.append((s, L))
    return out
