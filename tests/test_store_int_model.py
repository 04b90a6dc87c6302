"""The soundness of tests/store_int_cases.py, on the CPU: the library exposes the five integer twins of the device
batch calls, the helper's `widen` is the reference's expression, and the case set can show what tests/test_store_int.py
asks of it - the oracle alone decides that."""
import math

import numpy as np
import pytest

import store_int_cases as SI
from conftest import O

F32 = np.float32

SYMBOLS = ("glc_encode_batch_device_compact_int", "glc_roundtrip_batch_device_pcm", "glc_decode_batch_device_compact_i16",
           "glc_decode_crops_device_compact_i16", "glc_decode_crops_device_store_i16")


def test_the_library_exposes_the_five_calls():
    import glc_amd
    for name in SYMBOLS:
        assert hasattr(glc_amd.lib, name), name
        assert name in glc_amd._lib.SIGNATURES, name


def _as_f32_exact(s: int) -> float:
    """`s as f32` by integer arithmetic: round to nearest, ties to even, on a 24-bit significand."""
    a = abs(s)
    if a < (1 << 24):
        return float(s)
    shift = a.bit_length() - 24
    q, r = a >> shift, a & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return math.copysign(math.ldexp(q, shift), s)


def _rule(s: int, bits: int) -> float:
    """`s as f32 / (1 << (bits - 1)) as f32` with the divisor an i32 literal: 1 << 31 is i32::MIN (Q11).  The divisor
    is a power of two and no quotient is subnormal, so the f32 division is exact: ldexp."""
    e = bits - 1
    v = math.ldexp(_as_f32_exact(s), -e)
    return -v if bits == 32 else v


@pytest.mark.parametrize("fmt,bits", [(SI.S16, 8), (SI.S16, 12), (SI.S16, 16), (SI.S32, 17), (SI.S32, 24), (SI.S32, 32)])
def test_widen_is_the_reference_rule(fmt, bits):
    dt = SI.np_dtype(fmt)
    info = np.iinfo(dt)
    lo, hi = SI.int_range(bits)
    rng = np.random.default_rng(bits)
    vals = [info.min, info.max, lo, hi, 0, 1, -1, lo + 1, hi - 1] + rng.integers(info.min, info.max, 500, endpoint=True).tolist()
    if fmt == SI.S32:
        vals += [(1 << 24) + 1, (1 << 25) + 3, -(1 << 24) - 1, (1 << 24) + 3, (1 << 30) + 65, info.max - 64]
    s = np.array(vals, dt)
    got = SI.widen(s, bits)
    assert got.dtype == F32
    want = np.array([_rule(int(v), bits) for v in s.tolist()], np.float64)
    assert np.array_equal(want.astype(F32).astype(np.float64), want)          # every expected value is an f32
    assert np.array_equal(got.view(np.uint32), want.astype(F32).view(np.uint32))


def test_widen_named_values():
    i32 = lambda v: np.array([v], np.int32)
    assert SI.widen(i32(-2147483648), 32)[0] == F32(1.0)                       # Q11: INT32_MIN -> +1.0
    assert SI.widen(i32(2147483647), 32)[0] == F32(-1.0)                       # rounds to 2^31, over -2^31
    assert SI.widen(i32((1 << 24) + 1), 32)[0] == F32(-(1 << 24) / 2.0 ** 31)  # tie to even: down
    assert SI.widen(i32((1 << 25) + 3), 32)[0] == F32(-((1 << 25) + 4) / 2.0 ** 31)
    assert SI.widen(i32((1 << 24) + 1), 24)[0] == F32((1 << 24) / 2.0 ** 23)
    assert SI.widen(np.array([-32768], np.int16), 16)[0] == F32(-1.0)
    z = SI.widen(i32(0), 32)
    assert z.view(np.uint32)[0] == 0x80000000                                  # a zero SAMPLE is -0.0 at 32 bits


def test_narrow_named_values():
    x = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, -1.00004, 0.99999, 3.0518e-05, -3.0518e-05, 0.5], F32)
    assert SI.narrow(x).tolist() == [0, 32767, -32768, 32767, -32767, -32768, 32766, 0, 0, 16383]


@pytest.mark.parametrize("fmt,bits", SI.FORMATS)
@pytest.mark.parametrize("ch", (1, 2, 6))
def test_every_encode_family_has_raw_and_compressed_frames(fmt, bits, ch):
    """The oracle's streams of widen(clip) over a family's clips hold a raw and a compressed frame: a gather that
    scrambled samples would change both kinds of payload."""
    raw = comp = 0
    for clip in SI.family_clips(fmt, bits, ch):
        enc = O.encode(SI.widen(clip.reshape(-1), bits), SI.SR, ch, taps=True)
        raw += int(enc.is_raw.sum())
        comp += int((enc.is_raw == 0).sum())
    assert raw >= 1 and comp >= 1, (raw, comp)


def test_the_special_values_are_where_the_helper_says():
    for fmt, bits in SI.FORMATS:
        lo, hi = SI.int_range(bits)
        seen = set()
        for clip in SI.family_clips(fmt, bits, 3):
            seen |= set(clip[0].tolist()) | set(clip[-1].tolist())
        assert {lo, hi, 0, 1, -1} <= seen
    assert SI.int_range(32) == (np.iinfo(np.int32).min, np.iinfo(np.int32).max)
    assert SI.int_range(16) == (np.iinfo(np.int16).min, np.iinfo(np.int16).max)


@pytest.mark.parametrize("ch", (1, 2, 3, 6))
def test_the_narrowing_cases_clamp_at_both_rails_and_lie_inside(ch):
    x = SI.loud_clip(ch, 2049, 0).reshape(-1)
    y, _, _ = O.decode(O.encode(x, SI.SR, ch).glc)
    q = SI.narrow(y)
    with np.errstate(all="ignore"):
        v = y * F32(32767.0)
    assert (v > F32(32767.0)).any() and (v < F32(-32768.0)).any()              # clamped, not merely equal to a rail
    assert (q == 32767).any() and (q == -32768).any()
    assert ((q > -32768) & (q < 32767) & (q != 0)).any()


def test_builders_fill_everything_outside_the_clips():
    clips = SI.family_clips(SI.S16, 16, 3, (513, 1025))
    for planar in (True, False):
        for off in range(4):
            b = SI.input_batch(clips, 3, planar, off, np.int16)
            assert b.clip_stride % 2 == 1 and (not planar or b.channel_stride % 2 == 1)
            out = b.flat[~b.mask]
            assert set(out.tolist()) == {32767, -32768}
            for i, c in enumerate(clips):
                assert np.array_equal(b.gather(b.flat, i), c.reshape(-1))
            starts = {int(ix[0]) % 4 for ix in b.index}
            assert len(starts) == 2                                            # an odd stride: the clips differ in alignment
    o = SI.output_batch((5, 1025), 2, True, 3)
    assert (o.flat.view(np.uint16) == SI.SENTINEL).all() and o.mask.sum() == 2 * 1030
