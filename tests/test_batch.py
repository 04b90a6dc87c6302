"""glc_encode_batch / glc_decode_batch: many clips in one call, the same bytes per clip.

Expected values come from the CPU oracle (`O.encode(..).glc`, `O.decode(..)`) and, for hand-made streams, from
`decode_edges.expected_run`; the library's own single-stream calls are the expectation only where a test says
"equal to the single call".  Every comparison is bit for bit: `.glc` bytes, float32 viewed as uint32."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import conftest as cf
import decode_edges as DE
from conftest import O

pytestmark = pytest.mark.gpu

SR = 44100
HOP, FRAME = 1024, 2048
CHANNELS = (1, 2, 3, 8)
EINVAL, EFORMAT = -1, -4
F32 = np.float32


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    yield g
    _streams.clear()        # EncodedAudio objects: released while the library is still loaded


def encode_chunk_frames(ch):        # glc_api.hip: frames per encode round
    return 8192 if ch == 1 else 4096


# ------------------------------------------------------------------------------------------ oracle, cached

_enc_cache, _dec_cache = {}, {}


def oracle_glc(x, ch) -> bytes:
    x = np.ascontiguousarray(x, F32)
    key = (hashlib.sha1(x.tobytes()).digest(), ch)
    if key not in _enc_cache:
        _enc_cache[key] = O.encode(x, SR, ch).glc
    return _enc_cache[key]


def oracle_pcm(glc: bytes) -> np.ndarray:
    key = hashlib.sha1(glc).digest()
    if key not in _dec_cache:
        _dec_cache[key] = O.decode(glc)[0]
    return _dec_cache[key]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------ clips

def frames_of(per_channel):
    return -(-(512 + per_channel) // HOP) - 1       # src/codec.rs:433-455


def noise(ch, per_channel, seed):
    x = cf.gen_noise(SR, ch, (per_channel + 8) / SR, seed)
    assert x.size >= per_channel * ch
    return x[:per_channel * ch].copy()


def sine(ch, per_channel, f0=440.0):
    x = cf.gen_tone("sine", f0, SR, ch, (per_channel + 8) / SR)
    assert x.size >= per_channel * ch
    return x[:per_channel * ch].copy()


_mixed = {}


def mixed_clips(ch):
    """The batch of the issue's first encode case: (name, samples)."""
    if ch not in _mixed:
        clips = [(f"len{L}", cf.gen_chord(SR, ch, L, seed=L)) for L in (513, 1024, 1535, 1536, 1537, 2049)]
        clips.append(("config1-sine", cf.gen_tone("sine", 440.0, SR, ch, 2.0)))
        clips.append(("noise", cf.gen_noise(SR, ch, 0.25, 11)))
        clips.append(("chord3000", cf.gen_chord(SR, ch, 3000 * HOP - 100, seed=3, n_tones=4)))
        clips.append(("silence", np.zeros(5000 * ch, F32)))
        clips.append(("ragged", cf.gen_chord(SR, ch, 3000, seed=5)[:3000 * ch - 1].copy()))
        if ch in (1, 2):
            nf = encode_chunk_frames(ch) + 37
            clips.append(("longer-than-a-round", sine(ch, nf * HOP + 100, 523.25)))
            assert frames_of(nf * HOP + 100) == nf
        assert frames_of(3000 * HOP - 100) == 3000
        _mixed[ch] = clips
    return _mixed[ch]


_pool = {}


def small_pool(ch):
    """Distinct clips of 1 .. 12 frames, three signals each, lengths off the frame grid."""
    if ch not in _pool:
        pool = []
        for nf in range(1, 13):
            for v in range(3):
                L = nf * HOP + 512 - (37 * (v + 1) * nf) % 1000
                assert frames_of(L) == nf
                x = (cf.gen_chord(SR, ch, L, seed=100 + nf), noise(ch, L, 200 + nf), sine(ch, L, 200.0 + 50 * nf))[v]
                pool.append(x)
        _pool[ch] = pool
    return _pool[ch]


def check_batch(glc_amd, enc, clips, ch, names=None):
    out = enc.encode_batch(clips, ch)
    assert len(out) == len(clips)
    for i, (x, ea) in enumerate(zip(clips, out)):
        assert ea.to_bytes() == oracle_glc(x, ch), (i, names[i] if names else None)
    return out


# ------------------------------------------------------------------------------------------ encode

@pytest.mark.parametrize("ch", CHANNELS)
def test_encode_mixed_batch(glc_amd, ch):
    names, clips = zip(*mixed_clips(ch))
    check_batch(glc_amd, glc_amd.Encoder(SR), list(clips), ch, names)


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("neighbour", ("1e30", "nan"))
def test_encode_isolation(glc_amd, ch, neighbour):
    """A probe between two loud clips keeps the oracle's bytes; the staging memory between the slots is stale
    from a long, loud encode just before."""
    enc = glc_amd.Encoder(SR)
    loud = np.full(2000 * ch, 1e30 if neighbour == "1e30" else np.nan, F32)
    enc.encode(np.full(300000 * ch, 1e30, F32), ch)
    probes = [cf.gen_chord(SR, ch, 513, seed=1), cf.gen_chord(SR, ch, 1537, seed=2), noise(ch, 3000, 3),
              sine(ch, 4410), np.zeros(2049 * ch, F32)]
    batch = [loud]
    for p in probes:
        batch += [p, loud]
    out = enc.encode_batch(batch, ch)
    alone = enc.encode(loud, ch).to_bytes()         # equal to the single call, on purpose
    for i, ea in enumerate(out):
        if i % 2:
            assert ea.to_bytes() == oracle_glc(batch[i], ch), i
        else:
            assert ea.to_bytes() == alone, i


@pytest.mark.parametrize("ch", CHANNELS)
def test_encode_order_and_reuse(glc_amd, ch):
    enc = glc_amd.Encoder(SR)
    clips = [x for _, x in mixed_clips(ch)[:8]] + small_pool(ch)[:9]
    first = [ea.to_bytes() for ea in check_batch(glc_amd, enc, clips, ch)]
    perm = np.random.default_rng(ch).permutation(len(clips))
    assert [ea.to_bytes() for ea in enc.encode_batch([clips[i] for i in perm], ch)] == [first[i] for i in perm]
    assert [ea.to_bytes() for ea in enc.encode_batch(clips, ch)] == first         # the same batch again: buffers reused
    for x in (clips[0], clips[6]):
        one = enc.encode_batch([x], ch)
        assert len(one) == 1 and one[0].to_bytes() == enc.encode(x, ch).to_bytes() == oracle_glc(x, ch)


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("n", (1, 2, 64, 700))
def test_encode_sizes(glc_amd, ch, n):
    """Many clips per round, rows past one scan block of the compaction, clip boundaries everywhere inside a
    transform tile and a quantiser wave."""
    pool = small_pool(ch)
    pick = np.random.default_rng(1000 * ch + n).integers(0, len(pool), n)
    check_batch(glc_amd, glc_amd.Encoder(SR), [pool[i] for i in pick], ch)


def _raw_encode_batch(glc_amd, enc, arrays, lens, ch, null_at=None):
    n = len(arrays)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrays])
    if null_at is not None:
        ptrs[null_at] = None
    ln = (C.c_uint64 * max(n, 1))(*lens)
    outs = (C.c_void_p * max(n, 1))(*([0xDEAD0] * n))
    rc = glc_amd.lib.glc_encode_batch(enc._h, ptrs, ln, n, ch, outs)
    msg = (glc_amd.lib.glc_last_error(enc._h) or b"").decode()
    return rc, msg, [outs[i] for i in range(n)]


@pytest.mark.parametrize("ch", CHANNELS)
def test_encode_errors(glc_amd, ch):
    enc = glc_amd.Encoder(SR)
    good = small_pool(ch)[:5]
    for bad_len in (1, 511, 512):                   # per-channel samples the reference slices out of bounds on
        for at in (0, 2, 5):
            arrays = good[:at] + [np.zeros(bad_len * ch, F32)] + good[at:]
            rc, msg, outs = _raw_encode_batch(glc_amd, enc, arrays, [a.size for a in arrays], ch)
            assert rc == EINVAL and f"clip {at}" in msg and all(o is None for o in outs), (bad_len, at, rc, msg, outs)
    rc, msg, outs = _raw_encode_batch(glc_amd, enc, good, [a.size for a in good], ch, null_at=3)
    assert rc == EINVAL and "clip 3" in msg and all(o is None for o in outs), (rc, msg)
    rc, msg, outs = _raw_encode_batch(glc_amd, enc, good, [a.size for a in good], 0)
    assert rc == EINVAL and "channels == 0" in msg and all(o is None for o in outs), (rc, msg)
    rc, msg, outs = _raw_encode_batch(glc_amd, enc, [], [], ch)
    assert rc == 0
    assert glc_amd.lib.glc_encode_batch(enc._h, None, None, 0, ch, None) == 0
    check_batch(glc_amd, enc, good, ch)             # the context still encodes correctly


# ------------------------------------------------------------------------------------------ decode

def crafted_streams(ch):
    """(name, Stream): the decode edges of a batch, per channel count."""
    out = []
    values = next(c for c in DE.cases() if c.family == "values").stream.rows
    rows = list(values) + [DE.EMPTY] * ((-len(values)) % ch)
    out.append(("values", DE.Stream(SR, ch, rows)))
    pal = DE._palette(900 + ch)
    rng = np.random.default_rng(910 + ch)

    def plain(nf, salt):
        return [DE._pick(pal, ch, salt, m) for m in range(nf * ch)]
    lengths = [0, 1, ch, FRAME * ch - 1, FRAME * ch, FRAME * ch + 1]
    raws = [None] + [DE._raw_vec(rng, ch, n) for n in lengths] + [None, DE._raw_vec(rng, ch)]
    out.append(("raw", DE.Stream(48000, ch, plain(len(raws), 1), raws)))
    P = HOP * ch

    def trimmed(name, nf, delay, orig, salt):
        st = DE.Stream(SR, ch, plain(nf, salt))
        st.delay, st.orig, st.total = delay, orig, orig
        out.append((name, st))
    nf = 5
    total = (nf + 1) * P
    trimmed("cut-first-and-tail", nf, 101, total - 101 - 299, 2)
    trimmed("cut-by-one", nf, 1, total - 2, 3)
    trimmed("delay-several-hops", nf, 2 * P + 77, total - (2 * P + 77) - 5, 4)
    trimmed("delay-whole-hops", nf, 3 * P, total - 3 * P, 5)
    trimmed("ends-mid-stream", nf, 3, 2 * P + 11, 6)
    trimmed("inside-one-hop", nf, P + 10, 7, 7)
    trimmed("delay-equals-length", nf, total, total - 300, 8)      # :758: nothing is dropped in front
    trimmed("delay-beyond-length", nf, total + 1000, total, 9)
    trimmed("nothing-left", nf, 512, 0, 10)
    trimmed("one-frame", 1, 512, 2 * P - 512 - 300, 11)
    trimmed("one-frame-untrimmed", 1, 0, 2 * P, 12)
    return out


def noncanonical_glc(ch) -> bytes:
    """Duplicates (last write wins), descending order and indices >= 1024 (ignored), src/codec.rs:659-665."""
    lists = [[(5, 100), (5, -200), (7, 300)],
             [(900, 10), (300, 20), (2, 30)],
             [(1024, 999), (3, 50), (65535, -7), (2000, 5)],
             [(10, 1), (11, 0), (10, 0), (1023, -32768), (0, 32767)],
             [(4, 4), (3, 3), (4, 5), (1500, 1), (3, -3)]]
    nf = 4
    out = [struct.pack("<IHQQ", SR, ch, 0, nf)]
    k = 0
    for f in range(nf):
        out.append(struct.pack("<Q", ch))
        for c in range(ch):
            lst = lists[k % len(lists)] if (f, c) != (2, 0) else []
            k += 1
            out.append(struct.pack("<Q", len(lst)))
            out.append(b"".join(struct.pack("<Hh", i, q) for i, q in lst))
        out += [struct.pack("<Q", ch), np.linspace(0.1, 0.9, ch).astype(F32).tobytes(), b"\x00"]
    out.append(struct.pack("<IIQ", 300, 0, (nf + 1) * HOP * ch - 300 - 41))
    return b"".join(out)


_streams = {}


def batch_streams(glc_amd, ch):
    """[(name, EncodedAudio, expected float32)]"""
    if ch not in _streams:
        got = []
        for name, x in mixed_clips(ch):
            glc = oracle_glc(x, ch)
            got.append((name, glc_amd.EncodedAudio.from_bytes(glc), oracle_pcm(glc)))
        for name, st in crafted_streams(ch):
            got.append((name, st.to_encoded(glc_amd), DE.expected_run(st, DE.Run("decode"))))
        nc = noncanonical_glc(ch)
        got.append(("non-canonical", glc_amd.EncodedAudio.from_bytes(nc), oracle_pcm(nc)))
        # interleave the hand-made streams with the encoder's
        order = np.random.default_rng(77 + ch).permutation(len(got))
        _streams[ch] = [got[i] for i in order]
    return _streams[ch]


def _decode_batch_raw(glc_amd, dec, encs, byte_offset=0, slack=333, cap=None):
    """glc_decode_batch into a sentinel-filled buffer `byte_offset` bytes past a 16-byte boundary.
    -> rc, offsets, the buffer (slack included)."""
    n = len(encs)
    lens = [int(glc_amd.lib.glc_decoded_len(e._h)) for e in encs]
    room = sum(lens) + slack
    store = DE.sentinel(room + 8)
    skew = ((-store.ctypes.data) % 16 + byte_offset) // 4
    buf = store[skew:skew + room]
    assert buf.ctypes.data % 16 == byte_offset
    handles = (C.c_void_p * max(n, 1))(*[e._h for e in encs])
    offsets = (C.c_uint64 * (n + 1))(*([0xABCDEF] * (n + 1)))
    rc = glc_amd.lib.glc_decode_batch(dec._h, handles, n, buf.ctypes.data_as(C.c_void_p), room if cap is None else cap,
                                      offsets)
    return rc, [int(o) for o in offsets], buf, lens


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("byte_offset", DE.OFFSETS)
def test_decode_batch(glc_amd, ch, byte_offset):
    streams = batch_streams(glc_amd, ch)
    dec = glc_amd.Decoder(ch, SR)
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, [e for _, e, _ in streams], byte_offset)
    assert rc == 0, glc_amd.lib.glc_last_error(dec._h)
    assert offsets == [0] + list(np.cumsum(lens)), "offsets are the running sums of glc_decoded_len"
    for i, (name, _, want) in enumerate(streams):
        got = buf[offsets[i]:offsets[i + 1]]
        assert got.size == want.size, (name, got.size, want.size)
        assert np.array_equal(bits(got), bits(want)), (name, int(np.flatnonzero(bits(got) != bits(want))[0]))
    assert (bits(buf[offsets[-1]:]) == DE.SENTINEL_BITS).all(), "written past offsets[n]"
    assert dec.resident_stream() == 0


@pytest.mark.parametrize("ch", CHANNELS)
def test_decode_small_batches(glc_amd, ch):
    """Batches of one, of two, and of every crafted stream alone between two encoder streams."""
    streams = batch_streams(glc_amd, ch)
    dec = glc_amd.Decoder(ch, SR)
    small = [s for s in streams if s[2].size < 200000]
    for group in [[s] for s in small] + [small[i:i + 2] for i in range(len(small) - 1)]:
        rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, [e for _, e, _ in group], 4, slack=17)
        assert rc == 0
        for i, (name, _, want) in enumerate(group):
            assert np.array_equal(bits(buf[offsets[i]:offsets[i + 1]]), bits(want)), [g[0] for g in group]
        assert (bits(buf[offsets[-1]:]) == DE.SENTINEL_BITS).all()


@pytest.mark.parametrize("ch", CHANNELS)
def test_decode_edge_batch(glc_amd, ch):
    """The float output of the descriptor overlap-add on the batch that test_batch_int decodes to 16 bits: 39 streams
    of 1-3 frames whose kept spans start at every residue of dst mod 4 with every residue of cnt mod 4."""
    import test_batch_int as TI                  # it imports this module: not at the top
    assert TI.all_sixteen(ch)
    streams = TI.edge_streams(ch)
    wants = [TI.oracle_pcm(g) for _, g in streams]
    dec = glc_amd.Decoder(ch, SR)
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, [glc_amd.EncodedAudio.from_bytes(g) for _, g in streams], 4)
    assert rc == 0, glc_amd.lib.glc_last_error(dec._h)
    assert offsets == [0] + list(np.cumsum(lens)) and lens == [w.size for w in wants]
    for i, ((name, _), want) in enumerate(zip(streams, wants)):
        got = buf[offsets[i]:offsets[i + 1]]
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, f"{name}: {bad.size} samples differ, first at {bad[0]}"
    assert (bits(buf[offsets[-1]:]) == DE.SENTINEL_BITS).all(), "written past offsets[n]"


@pytest.mark.parametrize("ch", CHANNELS)
def test_decode_state(glc_amd, ch):
    streams = [s for s in batch_streams(glc_amd, ch) if s[0] in ("config1-sine", "noise", "raw")]
    (_, a, want_a), (_, b, want_b), (_, c, want_c) = streams
    dec = glc_amd.Decoder(ch, SR)
    first = dec.decode(a).copy()
    assert np.array_equal(bits(first), bits(want_a)) and dec.resident_stream() == a.stream_id
    got = dec.decode_batch([b, c])
    assert np.array_equal(bits(got[0]), bits(want_b)) and np.array_equal(bits(got[1]), bits(want_c))
    assert dec.resident_stream() == 0
    assert np.array_equal(bits(dec.decode(a)), bits(first))
    # a batch decode closes an open streaming session, as glc_decode does
    lib = glc_amd.lib
    assert lib.glc_decode_stream_begin(dec._h, a._h) == 0
    assert dec.decode_batch([b])[0].size == want_b.size
    chunk = np.empty((glc_amd.FRAMES_PER_CHUNK + 1) * HOP * ch, F32)
    n, last = C.c_uint64(), C.c_int()
    assert lib.glc_decode_stream_next(dec._h, chunk.ctypes.data_as(C.c_void_p), chunk.size, C.byref(n), C.byref(last)) == EINVAL
    assert b"no stream open" in lib.glc_last_error(dec._h)
    assert np.array_equal(bits(dec.decode(a)), bits(first))


def test_decode_errors(glc_amd):
    lib = glc_amd.lib
    dec = glc_amd.Decoder(2, SR)
    two = [e for _, e, _ in batch_streams(glc_amd, 2) if e.info().n_frames < 100][:3]
    one = [e for _, e, _ in batch_streams(glc_amd, 1) if e.info().n_frames < 100][0]
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, two[:2] + [one] + two[2:])
    assert rc == EINVAL and b"stream 2" in lib.glc_last_error(dec._h)
    assert (bits(buf) == DE.SENTINEL_BITS).all()
    # cap == 0 sizes the buffer
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, two, cap=0)
    assert rc == EINVAL and b"output buffer too small" in lib.glc_last_error(dec._h)
    assert offsets == [0] + list(np.cumsum(lens)) and (bits(buf) == DE.SENTINEL_BITS).all()
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, two, cap=sum(lens) - 1)
    assert rc == EINVAL and (bits(buf) == DE.SENTINEL_BITS).all()
    # nothing to decode
    off0 = (C.c_uint64 * 1)(99)
    assert lib.glc_decode_batch(dec._h, None, 0, None, 0, off0) == 0 and off0[0] == 0
    # a frame with fewer channel vectors than header.channels (the reference panics, :652-653)
    bad = b"".join([struct.pack("<IHQQ", SR, 2, 0, 1), struct.pack("<Q", 1), struct.pack("<Q", 0), struct.pack("<Q", 1),
                    np.ones(1, F32).tobytes(), b"\x00", struct.pack("<IIQ", 512, 0, 100)])
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, [two[0], glc_amd.EncodedAudio.from_bytes(bad), two[1]])
    assert rc == EFORMAT, lib.glc_last_error(dec._h)
    # ... and the context still decodes
    rc, offsets, buf, lens = _decode_batch_raw(glc_amd, dec, two)
    assert rc == 0
    wants = {id(e): w for _, e, w in batch_streams(glc_amd, 2)}
    for i, e in enumerate(two):
        assert np.array_equal(bits(buf[offsets[i]:offsets[i + 1]]), bits(wants[id(e)]))


@pytest.mark.parametrize("ch", CHANNELS)
def test_round_trip_python(glc_amd, ch):
    clips = [x for name, x in mixed_clips(ch) if name not in ("chord3000", "longer-than-a-round")] + small_pool(ch)[::5]
    enc, dec = glc_amd.Encoder(SR), glc_amd.Decoder(ch, SR)
    encoded = enc.encode_batch(clips, ch)
    decoded = dec.decode_batch(encoded)
    assert len(decoded) == len(clips)
    for x, d in zip(clips, decoded):
        assert np.array_equal(bits(d), bits(oracle_pcm(oracle_glc(x, ch))))
    total = sum(d.size for d in decoded)
    out = DE.sentinel(total + 50)
    again = dec.decode_batch(encoded, out=out)
    assert all(np.shares_memory(a, out) and np.array_equal(bits(a), bits(d)) for a, d in zip(again, decoded))
    assert (bits(out[total:]) == DE.SENTINEL_BITS).all()
    assert dec.decode_batch([]) == [] and enc.encode_batch([], ch) == []
