"""glc_encode_batch_int / glc_decode_batch_i16: the batch calls taking and returning integer PCM, and the CLI on them.

Expected values come from the CPU oracle (`O.encode(..).glc`, `O.decode(..)`) and from the restated conversions
`widen` / `narrow` of test_int_pcm.py; the library's own single calls (`glc_encode_int`, `glc_decode_i16`) are a
third side of a comparison, never the only one.  Every comparison is bit for bit.  The conditions a batch must
meet to test anything (both frame kinds; every decision of the narrowing; every chunk shape of the narrowing
overlap-add) are asserted on the oracle's output or on the lengths alone, on the CPU, before a device is touched -
and once more as CPU tests of their own."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import conftest as cf
import decode_edges as DE
import glc_amd
import test_batch as TB
from conftest import O
from test_int_pcm import _write_wav, narrow, quantise16, widen

SR = 44100
HOP, FRAME = 1024, 2048
CHANNELS = (1, 2, 3, 8)
EINVAL, EFORMAT = -1, -4
S16, S32, PF32 = 1, 2, 3
F32 = np.float32
I16_SENTINEL = -21846   # 0xAAAA
FORMATS = ((np.int16, 16), (np.int32, 20), (np.int32, 24), (np.int32, 32))
PACK_CLIP_BYTES = 256 << 10      # glc_api.hip kPackClipBytes: clips of at most this many bytes AS UPLOADED are packed
CLI = os.path.join(cf.ROOT, "build", "glc")
lib = glc_amd.lib


def quantise(x, dt, bits):
    """A float signal as the `bits`-bit file a user would have."""
    if dt == np.int16:
        assert bits == 16
        return quantise16(x)
    full = 1 << (bits - 1)
    return np.clip(np.rint(x.astype(np.float64) * full), -full, full - 1).astype(np.int32)


_ref = {}


def oracle_glc(s, bits, ch) -> bytes:
    """The oracle's .glc for the integers `s`: what the reference encodes after its loader widened them."""
    key = (s.tobytes(), str(s.dtype), bits, ch)
    if key not in _ref:
        _ref[key] = O.encode(widen(s, bits), SR, ch).glc
    return _ref[key]


def frame_kinds(glc: bytes):
    frames = cf.parse_glc(glc)["frames"]
    return {"raw" if f["raw"] is not None else "compressed" for f in frames}


# ------------------------------------------------------------------------------------------ encode: the batches

def mixed_int_clips(ch, dt, bits):
    """[(name, int samples)]: 1 frame, a few frames, ragged ends, one longer than a round (which also closes the
    round in front of it), and a last clip that is left alone in its round behind it."""
    sigs = [(f"len{L}", cf.gen_chord(SR, ch, L, seed=L)) for L in (513, 1024, 1535, 1537, 2049)]
    sigs.append(("sine", cf.gen_tone("sine", 440.0, SR, ch, 0.5)))
    sigs.append(("noise", cf.gen_noise(SR, ch, 0.25, 11)))                  # full scale: raw frames
    sigs.append(("silence", np.zeros(5000 * ch, F32)))
    sigs.append(("ragged", cf.gen_chord(SR, ch, 3000, seed=5)[:3000 * ch - 1].copy()))
    nf = TB.encode_chunk_frames(ch) + 37
    sigs.append(("longer-than-a-round", TB.sine(ch, nf * HOP + 100, 523.25)))
    assert TB.frames_of(nf * HOP + 100) == nf
    sigs.append(("alone-in-its-round", cf.gen_chord(SR, ch, 4000, seed=9)))
    return [(name, quantise(x, dt, bits)) for name, x in sigs]


def both_frame_kinds(clips, bits, ch):
    """On the oracle's output, cheapest clips first: the batch holds raw frames and compressed frames."""
    seen = set()
    for _, s in sorted(clips, key=lambda c: c[1].size):
        seen |= frame_kinds(oracle_glc(s, bits, ch))
        if seen == {"raw", "compressed"}:
            return True
    return False


@pytest.mark.parametrize("ch", CHANNELS)
def test_mixed_batches_hold_both_frame_kinds_on_the_oracle(ch):
    for dt, bits in FORMATS:
        assert both_frame_kinds(mixed_int_clips(ch, dt, bits), bits, ch), (dt, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("dt,bits", FORMATS)
def test_encode_mixed_batch(ch, dt, bits):
    clips = mixed_int_clips(ch, dt, bits)
    assert both_frame_kinds(clips, bits, ch)
    enc = glc_amd.Encoder(SR)
    out = enc.encode_batch([s for _, s in clips], ch, bits=bits)
    assert len(out) == len(clips)
    for (name, s), ea in zip(clips, out):
        got = ea.to_bytes()
        assert got == oracle_glc(s, bits, ch), (name, "differs from the oracle's bytes for widen(clip)")
        assert got == enc.encode(s, ch, bits=bits).to_bytes(), (name, "differs from glc_encode_int of the clip alone")


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("dt,bits", ((np.int16, 16), (np.int32, 32)))
def test_encode_isolation(ch, dt, bits):
    """A probe between two neighbours at the extremes of its container keeps the bytes it has alone; the staging
    memory is stale from a long, loud encode just before."""
    enc = glc_amd.Encoder(SR)
    info = np.iinfo(dt)
    enc.encode(np.full(300000 * ch, info.min, dt), ch, bits=bits)
    probes = [quantise(x, dt, bits) for x in (cf.gen_chord(SR, ch, 513, seed=1), cf.gen_chord(SR, ch, 1537, seed=2),
                                               TB.noise(ch, 3000, 3), TB.sine(ch, 4410), np.zeros(2049 * ch, F32))]
    for lo_first in (True, False):
        a, b = (info.min, info.max) if lo_first else (info.max, info.min)
        batch = [np.full(2000 * ch, a, dt)]
        for k, p in enumerate(probes):
            batch += [p, np.full(2000 * ch, b if k % 2 == 0 else a, dt)]
        out = enc.encode_batch(batch, ch, bits=bits)
        for i, ea in enumerate(out):
            assert ea.to_bytes() == oracle_glc(batch[i], bits, ch), (i, lo_first)


def int_pool(ch, dt, bits):
    return [quantise(x, dt, bits) for x in TB.small_pool(ch)]


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("n", (1, 2, 64, 700))
def test_encode_sizes(ch, n):
    enc = glc_amd.Encoder(SR)
    for dt, bits in ((np.int16, 16), (np.int32, 24)):
        pool = int_pool(ch, dt, bits)
        pick = np.random.default_rng(2000 * ch + n).integers(0, len(pool), n)
        out = enc.encode_batch([pool[i] for i in pick], ch, bits=bits)
        assert len(out) == n
        for i, ea in zip(pick, out):
            assert ea.to_bytes() == oracle_glc(pool[i], bits, ch), (dt, int(i))


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_encode_staging(ch):
    """Both sides of the packing limit, which counts the bytes as uploaded: 131072 int16 samples or 65536 int32
    samples are 256 KiB and are packed into the pinned image, one interleaved frame more goes up on its own -
    per channel 131072 / ch and 65536 / ch samples (+ 1 frame), rounded to whole interleaved frames below and
    above the limit for 3 channels.  Sources sit at odd element offsets inside a larger array (2-byte aligned
    only for int16, 4-byte aligned only for int32)."""
    enc = glc_amd.Encoder(SR)
    for dt, bits in ((np.int16, 16), (np.int32, 24)):
        limit = PACK_CLIP_BYTES // np.dtype(dt).itemsize // ch          # per-channel samples of the largest packed clip
        clips = []
        for k, per in enumerate((limit - 1, limit, limit + 1, 700, limit + 1, limit, 2048)):
            x = cf.gen_chord(SR, ch, per, seed=40 + k, n_tones=3) + (TB.noise(ch, per, 50 + k) * F32(0.3) if k % 3 == 0 else 0)
            s = quantise(x.astype(F32), dt, bits)
            assert (s.nbytes <= PACK_CLIP_BYTES) == (per <= limit)
            store = np.zeros(s.size + 3, dt)
            store[1 + (k % 2) * 2:][:s.size] = s
            view = store[1 + (k % 2) * 2:][:s.size]
            assert view.ctypes.data % np.dtype(dt).itemsize == 0 and view.ctypes.data % (2 * np.dtype(dt).itemsize) != 0
            clips.append(view)
        out = enc.encode_batch(clips, ch, bits=bits)
        for k, (s, ea) in enumerate(zip(clips, out)):
            assert ea.to_bytes() == oracle_glc(np.ascontiguousarray(s), bits, ch), (dt, k)


def _raw_encode_batch_int(enc, arrays, lens, ch, fmt=S16, bits=16, null_at=None):
    n = len(arrays)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrays])
    if null_at is not None:
        ptrs[null_at] = None
    ln = (C.c_uint64 * max(n, 1))(*lens)
    outs = (C.c_void_p * max(n, 1))(*([0xDEAD0] * n))
    rc = lib.glc_encode_batch_int(enc._h, ptrs, fmt, bits, ln, n, ch, outs)
    msg = (lib.glc_last_error(enc._h) or b"").decode()
    return rc, msg, [outs[i] for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_encode_errors(ch):
    enc = glc_amd.Encoder(SR)
    good = int_pool(ch, np.int16, 16)[:5]
    sizes = [a.size for a in good]
    for bad_len in (1, 511, 512):                   # per-channel samples the reference slices out of bounds on
        for at in (0, 2, 5):
            arrays = good[:at] + [np.zeros(bad_len * ch, np.int16)] + good[at:]
            rc, msg, outs = _raw_encode_batch_int(enc, arrays, [a.size for a in arrays], ch)
            assert rc == EINVAL and f"clip {at}" in msg and all(o is None for o in outs), (bad_len, at, rc, msg, outs)
    rc, msg, outs = _raw_encode_batch_int(enc, good, sizes, ch, null_at=3)
    assert rc == EINVAL and "clip 3" in msg and all(o is None for o in outs), (rc, msg)
    rc, msg, outs = _raw_encode_batch_int(enc, good, sizes, 0)
    assert rc == EINVAL and "channels == 0" in msg and all(o is None for o in outs), (rc, msg)
    # bits out of range for the format, unknown formats: the codes of glc_encode_int
    one = C.c_void_p()
    for fmt, b in ((S16, 0), (S16, 17), (S32, 0), (S32, 33), (0, 16), (4, 16), (-1, 16)):
        rc, msg, outs = _raw_encode_batch_int(enc, good, sizes, ch, fmt=fmt, bits=b)
        single = lib.glc_encode_int(enc._h, good[0].ctypes.data_as(C.c_void_p), fmt, b, good[0].size, ch, C.byref(one))
        assert rc == single == EINVAL and all(o is None for o in outs), (fmt, b, rc, single, msg)
    rc, msg, outs = _raw_encode_batch_int(enc, [], [], ch)
    assert rc == 0
    assert lib.glc_encode_batch_int(enc._h, None, S16, 16, None, 0, ch, None) == 0
    # GLC_PCM_F32 forwards to the float batch path
    fl = [widen(a, 16) for a in good]
    rc, msg, outs = _raw_encode_batch_int(enc, fl, sizes, ch, fmt=PF32, bits=0)
    assert rc == 0, msg
    for a, o in zip(good, outs):
        assert glc_amd.EncodedAudio(o).to_bytes() == oracle_glc(a, 16, ch)
    # ... and the context still encodes correctly
    for a, ea in zip(good, enc.encode_batch(good, ch)):
        assert ea.to_bytes() == oracle_glc(a, 16, ch)


# ------------------------------------------------------------------------------------------ decode: values

def value_streams(ch):
    """[(name, .glc bytes)]: hand-made streams with the decode edges and crafted trims of test_batch, its
    non-canonical stream, and the encoder's own output for a tone, full-scale noise (raw frames) and silence."""
    out = [(name, st.to_glc()) for name, st in TB.crafted_streams(ch)]
    out.append(("non-canonical", TB.noncanonical_glc(ch)))
    for name, x in (("sine", TB.sine(ch, 4410)), ("noise", TB.noise(ch, 3000, 3)), ("silence", np.zeros(2049 * ch, F32)),
                    ("chord", cf.gen_chord(SR, ch, 1537, seed=2))):
        out.append((name, O.encode(x, SR, ch).glc))
    order = np.random.default_rng(91 + ch).permutation(len(out))
    return [out[i] for i in order]


_dec = {}


def oracle_pcm(glc: bytes) -> np.ndarray:
    if glc not in _dec:
        _dec[glc] = O.decode(glc)[0]
    return _dec[glc]


def narrowing_classes(floats):
    """Which decisions of `(s * 32767.0).clamp(-32768.0, 32767.0) as i16` the samples exercise."""
    x = np.concatenate([np.asarray(f, F32) for f in floats])
    with np.errstate(all="ignore"):
        v = x * F32(32767.0)
    fin = np.isfinite(v) & (np.abs(v) < 32767)
    return dict(below=bool((v < -32768).any()), above=bool((v > 32767).any()), nan=bool(np.isnan(v).any()),
                negative_fraction=bool(((v[fin] < 0) & (np.trunc(v[fin]) != v[fin])).any()),
                exact=bool((np.trunc(v[fin]) == v[fin]).any()))


@pytest.mark.parametrize("ch", CHANNELS)
def test_value_streams_cover_the_narrowing_on_the_oracle(ch):
    cov = narrowing_classes([oracle_pcm(g) for _, g in value_streams(ch)])
    assert all(cov.values()), cov


def _decode_batch_i16_raw(dec, encs, byte_offset=0, front=40, slack=333, cap=None):
    """glc_decode_batch_i16 into a sentinel-filled buffer `byte_offset` bytes past a 16-byte boundary, with
    `front` sentinels before it and `slack` behind.  -> rc, offsets, the span, the whole store, lens."""
    n = len(encs)
    lens = [int(lib.glc_decoded_len(e._h)) for e in encs]
    total = sum(lens)
    store = np.full(front + total + slack + 16, I16_SENTINEL, np.int16)
    skew = ((-(store.ctypes.data + 2 * front)) % 16 + byte_offset) // 2 + front
    buf = store[skew:skew + total + slack]
    assert buf.ctypes.data % 16 == byte_offset and skew >= front
    handles = (C.c_void_p * max(n, 1))(*[e._h for e in encs])
    offsets = (C.c_uint64 * (n + 1))(*([0xABCDEF] * (n + 1)))
    rc = lib.glc_decode_batch_i16(dec._h, handles, n, buf.ctypes.data_as(C.c_void_p), total + slack if cap is None else cap,
                                  offsets)
    untouched = (store[:skew] == I16_SENTINEL).all() and (store[skew + (total if rc == 0 else 0):] == I16_SENTINEL).all()
    return rc, [int(o) for o in offsets], buf, untouched, lens


def _check_spans(dec, names, encs, wants, byte_offset=0, **kw):
    rc, offsets, buf, untouched, lens = _decode_batch_i16_raw(dec, encs, byte_offset, **kw)
    assert rc == 0, lib.glc_last_error(dec._h)
    assert offsets == [0] + list(np.cumsum(lens)), "offsets are the running sums of glc_decoded_len, in samples"
    for i, (name, want) in enumerate(zip(names, wants)):
        got = buf[offsets[i]:offsets[i + 1]]
        assert got.size == want.size, (name, got.size, want.size)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    assert untouched, "samples in front of the output or behind offsets[n] were written"
    assert dec.resident_stream() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_decode_values(ch):
    streams = value_streams(ch)
    floats = [oracle_pcm(g) for _, g in streams]                      # CPU first
    cov = narrowing_classes(floats)
    assert all(cov.values()), cov
    wants = [narrow(f) for f in floats]
    encs = [glc_amd.EncodedAudio.from_bytes(g) for _, g in streams]
    dec = glc_amd.Decoder(ch, SR)
    _check_spans(dec, [n for n, _ in streams], encs, wants)
    one = glc_amd.Decoder(ch, SR)
    for (name, _), ea, want in zip(streams, encs, wants):
        assert np.array_equal(one.decode(ea, dtype=np.int16), want), (name, "glc_decode_i16 of the stream alone")
    # batches of one and of two
    for i in range(len(encs)):
        _check_spans(dec, [streams[i][0]], encs[i:i + 1], wants[i:i + 1], 2, slack=17)
        _check_spans(dec, [s[0] for s in streams[i:i + 2]], encs[i:i + 2], wants[i:i + 2], 6, slack=17)


# ------------------------------------------------------------------------------------------ decode: kernel edges

def kept_spans(shapes, ch):
    """(dst, cnt) of every kept span of a batch, from the lengths alone: Decoder::decode keeps
    all[delay ..][.. original_length] of the (n_frames + 1) * 1024 * ch samples (the delay only when the stream is
    longer than it, src/codec.rs:756-765), a span is what one output hop keeps of it, dst the running sum."""
    P = HOP * ch
    spans, dst0 = [], 0
    for nf, delay, orig in shapes:
        total = (nf + 1) * P
        start = delay if total > delay else 0
        n = min(orig, total - start)
        if n:
            for h in range(start // P, (start + n - 1) // P + 1):
                lo, hi = max(start, h * P), min(start + n, (h + 1) * P)
                spans.append((dst0 + lo - start, hi - lo))
        dst0 += n
    return spans


def edge_shapes(ch):
    """(n_frames, encoder_delay, original_length) of a batch whose kept spans start at every residue of dst mod 4
    and have every residue of cnt mod 4: one-frame streams and longer ones, trims at both ends, inside one hop."""
    rng = np.random.default_rng(500 + ch)
    P = HOP * ch
    shapes = [(1, 0, 2 * P), (1, 512, 2 * P - 512 - 300), (1, P + 5, 3)]
    for k in range(36):
        nf = int(rng.integers(1, 4))
        total = (nf + 1) * P
        delay = int(rng.integers(0, total - 8))
        orig = int(rng.integers(1, total - delay + 1))
        shapes.append((nf, delay, orig))
    return shapes


def all_sixteen(ch):
    seen = {(d % 4, c % 4) for d, c in kept_spans(edge_shapes(ch), ch)}
    return seen == {(a, b) for a in range(4) for b in range(4)}


@pytest.mark.parametrize("ch", CHANNELS)
def test_edge_batches_reach_every_chunk_shape(ch):
    assert all_sixteen(ch)
    assert kept_spans([(5, 101, 6 * HOP * ch - 400)], ch)[0] == (0, HOP * ch - 101)      # the rule itself, once by hand


def edge_streams(ch):
    pal = DE._palette(1300 + ch)
    out = []
    for k, (nf, delay, orig) in enumerate(edge_shapes(ch)):
        st = DE.Stream(SR, ch, [DE._pick(pal, ch, k, m) for m in range(nf * ch)])
        st.delay, st.orig, st.total = delay, orig, orig
        out.append((f"edge{k}-{nf}f-{delay}-{orig}", st.to_glc()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_decode_edges_of_the_kernel(ch):
    assert all_sixteen(ch)
    streams = edge_streams(ch)
    wants = [narrow(oracle_pcm(g)) for _, g in streams]
    encs = [glc_amd.EncodedAudio.from_bytes(g) for _, g in streams]
    shapes = edge_shapes(ch)
    assert [w.size for w in wants] == [sum(c for _, c in kept_spans([s], ch)) for s in shapes]
    dec = glc_amd.Decoder(ch, SR)
    names = [n for n, _ in streams]
    for byte_offset in range(0, 16, 2):             # every 2-byte offset of a 16-byte line
        _check_spans(dec, names, encs, wants, byte_offset)
    total = sum(w.size for w in wants)
    _check_spans(dec, names, encs, wants, 10, slack=0, cap=total)                           # cap exactly the total
    rc, offsets, buf, untouched, lens = _decode_batch_i16_raw(dec, encs, 2, cap=0)          # cap == 0 sizes the buffer
    assert rc == EINVAL and b"output buffer too small" in lib.glc_last_error(dec._h)
    assert offsets == [0] + list(np.cumsum(lens)) and offsets[-1] == total and untouched
    rc, offsets, buf, untouched, lens = _decode_batch_i16_raw(dec, encs, 2, cap=total - 1)
    assert rc == EINVAL and untouched
    single = glc_amd.Decoder(ch, SR)
    for name, ea, want in zip(names, encs, wants):
        assert np.array_equal(single.decode(ea, dtype=np.int16), want), name


# ------------------------------------------------------------------------------------------ decode: state, errors

@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_decode_state(ch):
    by = dict(value_streams(ch))
    a, b, c = (glc_amd.EncodedAudio.from_bytes(by[k]) for k in ("sine", "noise", "raw"))
    fa, fb, fc = (oracle_pcm(by[k]) for k in ("sine", "noise", "raw"))
    dec = glc_amd.Decoder(ch, SR)
    assert np.array_equal(DE.bits(dec.decode(a)), DE.bits(fa)) and dec.resident_stream() == a.stream_id
    got = dec.decode_batch([b, c], dtype=np.int16)
    assert got[0].dtype == np.int16 and np.array_equal(got[0], narrow(fb)) and np.array_equal(got[1], narrow(fc))
    assert dec.resident_stream() == 0
    # a float batch decode and a single glc_decode_i16 on the same context afterwards are still bit-exact
    fl = dec.decode_batch([b, c])
    assert np.array_equal(DE.bits(fl[0]), DE.bits(fb)) and np.array_equal(DE.bits(fl[1]), DE.bits(fc))
    assert np.array_equal(dec.decode(a, dtype=np.int16), narrow(fa))
    # an open streaming session is closed, as glc_decode_batch does
    assert lib.glc_decode_stream_begin(dec._h, a._h) == 0
    assert dec.decode_batch([b], dtype=np.int16)[0].size == fb.size
    chunk = np.empty((glc_amd.FRAMES_PER_CHUNK + 1) * HOP * ch, np.int16)
    n, last = C.c_uint64(), C.c_int()
    assert lib.glc_decode_stream_next_i16(dec._h, chunk.ctypes.data_as(C.c_void_p), chunk.size, C.byref(n), C.byref(last)) == EINVAL
    assert b"no stream open" in lib.glc_last_error(dec._h)
    assert np.array_equal(DE.bits(dec.decode(a)), DE.bits(fa))


@pytest.mark.gpu
def test_decode_errors():
    dec = glc_amd.Decoder(2, SR)
    by2, by1 = dict(value_streams(2)), dict(value_streams(1))
    names = ("sine", "noise", "chord")
    two = [glc_amd.EncodedAudio.from_bytes(by2[k]) for k in names]
    one = glc_amd.EncodedAudio.from_bytes(by1["sine"])
    rc, offsets, buf, untouched, lens = _decode_batch_i16_raw(dec, two[:2] + [one] + two[2:])
    assert rc == EINVAL and b"stream 2" in lib.glc_last_error(dec._h) and untouched      # mixed channel counts
    off0 = (C.c_uint64 * 1)(99)
    assert lib.glc_decode_batch_i16(dec._h, None, 0, None, 0, off0) == 0 and off0[0] == 0
    # a frame with fewer channel vectors than header.channels (the reference panics, src/codec.rs:652-653)
    bad = b"".join([struct.pack("<IHQQ", SR, 2, 0, 1), struct.pack("<Q", 1), struct.pack("<Q", 0), struct.pack("<Q", 1),
                    np.ones(1, F32).tobytes(), b"\x00", struct.pack("<IIQ", 512, 0, 100)])
    rc, offsets, buf, untouched, lens = _decode_batch_i16_raw(dec, [two[0], glc_amd.EncodedAudio.from_bytes(bad), two[1]])
    assert rc == EFORMAT, lib.glc_last_error(dec._h)
    # ... and the context still decodes: the integer batch, a float batch, a single glc_decode_i16
    wants = [narrow(oracle_pcm(by2[k])) for k in names]
    _check_spans(dec, names, two, wants)
    for k, f in zip(names, dec.decode_batch(two)):
        assert np.array_equal(DE.bits(f), DE.bits(oracle_pcm(by2[k])))
    assert np.array_equal(dec.decode(two[1], dtype=np.int16), wants[1])


# ------------------------------------------------------------------------------------------ Python

@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_round_trip_python(ch):
    clips = [quantise16(x) for x in TB.small_pool(ch)[::5]] + [quantise16(TB.noise(ch, 3000, 3)), np.zeros(2049 * ch, np.int16)]
    enc, dec = glc_amd.Encoder(SR), glc_amd.Decoder(ch, SR)
    encoded = enc.encode_batch(clips, ch)
    decoded = dec.decode_batch(encoded, dtype=np.int16)
    assert len(decoded) == len(clips)
    for s, ea, d in zip(clips, encoded, decoded):
        assert ea.to_bytes() == oracle_glc(s, 16, ch)
        assert d.dtype == np.int16 and np.array_equal(d, narrow(oracle_pcm(oracle_glc(s, 16, ch))))
    total = sum(d.size for d in decoded)
    out = np.full(total + 50, I16_SENTINEL, np.int16)
    again = dec.decode_batch(encoded, out=out, dtype=np.int16)
    assert all(np.shares_memory(a, out) and np.array_equal(a, d) for a, d in zip(again, decoded))
    assert (out[total:] == I16_SENTINEL).all()
    with pytest.raises(glc_amd.GlcError) as e:      # out of the wrong dtype, either way
        dec.decode_batch(encoded, out=np.zeros(total, F32), dtype=np.int16)
    assert e.value.code == EINVAL
    with pytest.raises(glc_amd.GlcError) as e:
        dec.decode_batch(encoded, out=np.zeros(total, np.int16))
    assert e.value.code == EINVAL
    with pytest.raises(glc_amd.GlcError) as e:      # one call, one sample format
        enc.encode_batch([clips[0], clips[1].astype(np.int32)], ch)
    assert e.value.code == EINVAL
    with pytest.raises(glc_amd.GlcError) as e:
        enc.encode_batch([clips[0], widen(clips[1], 16)], ch)
    assert e.value.code == EINVAL
    assert dec.decode_batch([], dtype=np.int16) == [] and enc.encode_batch([], ch, bits=None) == []
    # int32 clips of 24 bits through the same call
    c24 = [quantise(x, np.int32, 24) for x in TB.small_pool(ch)[1::9]]
    for s, ea in zip(c24, enc.encode_batch(c24, ch, bits=24)):
        assert ea.to_bytes() == oracle_glc(s, 24, ch)


# ------------------------------------------------------------------------------------------ CPU: bindings, dtypes

def test_bindings_and_argument_checks_without_a_device():
    assert len(lib.glc_encode_batch_int.argtypes) == 8 and len(lib.glc_decode_batch_i16.argtypes) == 6
    buf = np.zeros(4096, np.int16)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data)
    lens = (C.c_uint64 * 1)(buf.size)
    outs = (C.c_void_p * 1)()
    offs = (C.c_uint64 * 2)()
    for fmt in (S16, S32, PF32, 0):                  # a null context is refused before anything else is looked at
        assert lib.glc_encode_batch_int(None, ptrs, fmt, 16, lens, 1, 1, outs) == EINVAL
    assert lib.glc_encode_batch_int(None, None, S16, 16, None, 0, 1, None) == EINVAL
    assert lib.glc_decode_batch_i16(None, None, 1, buf.ctypes.data_as(C.c_void_p), buf.size, offs) == EINVAL
    assert lib.glc_decode_batch_i16(None, None, 0, None, 0, offs) == EINVAL
    enc = glc_amd.Encoder.__new__(glc_amd.Encoder)   # no context: a check that reached the library would fail differently
    enc._h = None
    i16, i32, f32 = np.zeros(4096, np.int16), np.zeros(4096, np.int32), np.zeros(4096, F32)
    for mixed in ([i16, i32], [i32, i16], [i16, f32], [f32, i16, f32], [i32, f32]):
        with pytest.raises(glc_amd.GlcError) as e:
            enc.encode_batch(mixed, 1)
        assert e.value.code == EINVAL
    for clips, b in (([i16, i16], 0), ([i16], 17), ([i32, i32], 33)):
        with pytest.raises(glc_amd.GlcError) as e:
            enc.encode_batch(clips, 1, bits=b)
        assert e.value.code == EINVAL
    with pytest.raises(TypeError):
        enc.encode_batch([f32, f32], 1, bits=16)
    with pytest.raises(TypeError):
        enc.encode_batch([i16, np.zeros(4096, np.int64)], 1)
    dec = glc_amd.Decoder.__new__(glc_amd.Decoder)
    dec._h = None
    for dt in (np.int32, np.float64, np.uint16):
        with pytest.raises(TypeError):
            dec.decode_batch([], dtype=dt)
    for out, dt in ((np.zeros(8, F32), np.int16), (np.zeros(8, np.int16), np.float32), (np.zeros(8, np.int32), np.int16)):
        with pytest.raises(glc_amd.GlcError) as e:
            dec.decode_batch([], out=out, dtype=dt)
        assert e.value.code == EINVAL


# ------------------------------------------------------------------------------------------ CLI

def _cli_inputs(d):
    """WAV / FLAC files of two sample rates, three channel counts, 16 and 24 bits - several per batch group - with
    an unreadable file and a too-short file in the middle.  -> the file names, in argument order."""
    names = []
    k = 0
    for sr, ch, bits, kind in ((44100, 2, 16, "wav"), (48000, 2, 16, "wav"), (44100, 1, 24, "wav"), (44100, 2, 16, "flac"),
                               (48000, 2, 16, "wav"), (44100, 2, 16, "wav"), ("unreadable", 0, 0, "wav"), (44100, 3, 16, "wav"),
                               ("short", 2, 16, "wav"), (44100, 1, 24, "wav"), (48000, 2, 16, "flac"), (44100, 2, 16, "flac"),
                               (44100, 3, 16, "wav"), (48000, 1, 24, "wav")):
        k += 1
        name = f"f{k:02d}_{sr}_{ch}ch_{bits}.{kind}"
        if sr == "unreadable":
            (d / name).write_bytes(b"RIFF" + bytes(range(200)))
        elif sr == "short":
            _write_wav(d / name, 1, 16, ch, 44100, quantise16(cf.gen_chord(44100, ch, 300, seed=k)).tobytes())
        else:
            per = 3000 + 777 * k
            x = cf.gen_chord(sr, ch, per, seed=k, amp=0.1) if k % 3 else TB.noise(ch, per, k)
            if kind == "flac":
                (d / name).write_bytes(glc_amd.encode_flac(x, sr, ch))
            elif bits == 16:
                _write_wav(d / name, 1, 16, ch, sr, quantise16(x).tobytes())
            else:
                s = quantise(x, np.int32, 24)
                _write_wav(d / name, 1, 24, ch, sr, b"".join(int(v).to_bytes(3, "little", signed=True) for v in s))
        names.append(name)
    return names


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _one_by_one(flags, names, cwd):
    rcs, out, err = [], "", ""
    for n in names:
        rc, o, e = _run(flags + [n], cwd)
        rcs.append(rc)
        out += o
        err += e
    return rcs, out, err


@pytest.mark.gpu
def test_cli_many_files_equal_one_invocation_per_file(tmp_path):
    assert os.path.exists(CLI), "build/glc missing: run __graft_entry__.build()"
    single, many = tmp_path / "single", tmp_path / "many"
    single.mkdir()
    names = _cli_inputs(single)
    shutil.copytree(single, many)
    names.insert(4, "missing.wav")                  # argument errors keep their place among the others
    names.insert(9, "notes.txt")
    (single / "notes.txt").write_text("x")
    (many / "notes.txt").write_text("x")
    rcs, out1, err1 = _one_by_one([], names, single)
    rc, out, err = _run(names, many)
    assert rc == 1 and sorted(set(rcs)) == [0, 1]
    assert out == out1
    assert err.splitlines() == err1.splitlines()
    glcs = sorted(p.name for p in single.iterdir() if p.suffix == ".glc")
    assert len(glcs) == len(names) - 4 and glcs == sorted(p.name for p in many.iterdir() if p.suffix == ".glc")
    for g in glcs:
        assert (many / g).read_bytes() == (single / g).read_bytes(), g
        src = next(n for n in names if n.startswith(g[:-4] + "."))
        x, sr, ch = glc_amd.load_audio_file_lossless(single / src)
        assert (single / g).read_bytes() == O.encode(x, sr, ch).glc, g                     # ... and they are the oracle's
    # decode: the results, with a file that is no stream in the middle (a missing file is not among them: -d
    # reports those while it reads its arguments, before the first file, in one invocation or in many)
    args = glcs[:5] + ["broken.glc"] + glcs[5:]
    for d in (single, many):
        (d / "broken.glc").write_bytes(bytes(range(64)))
    for flags, ext in ((["-d", "--wav"], ".wav"), (["-d"], ".flac"), (["-d", "--flac-level", "2"], ".flac")):
        for d in (single, many):
            for p in d.iterdir():
                if p.suffix in (".wav", ".flac"):
                    p.unlink()
        rcs, out1, err1 = _one_by_one(flags, args, single)
        rc, out, err = _run(flags + args, many)
        assert rc == 1 and sorted(set(rcs)) == [0, 1], flags
        assert out == out1, flags
        assert err.splitlines() == err1.splitlines(), flags
        made = sorted(p.name for p in single.iterdir() if p.suffix == ext)
        assert len(made) == len(glcs) and made == sorted(p.name for p in many.iterdir() if p.suffix == ext)
        for m in made:
            assert (many / m).read_bytes() == (single / m).read_bytes(), (flags, m)
        if ext == ".wav":                           # the samples are the narrowed oracle decode
            for m in made:
                want = narrow(oracle_pcm((single / (m[:-4] + ".glc")).read_bytes()))
                assert (single / m).read_bytes()[44:] == want.tobytes(), m
