"""Decode of compact blobs where they lie in device memory: glc_decode_device_compact,
glc_decode_batch_device_compact, glc_decode_compact_last_status (row tables built around the payload by the R2
kernels, DESIGN.md sections 3 and 4), and glc_frames_to_compact on the way in.

Every comparison is bit for bit - float32 viewed as uint32, tolerance 0.  Expected samples always come from the
path that existed before: glc_decode of glc_frames_from_compact of the same bytes (for a blob the device check
refuses parts of: of the blob of the same description with exactly those rows' lists emptied,
compact_decode_cases.emptied).  The small natural clips are also held to the oracle's decode of the oracle's
stream.  Blobs the check must refuse sit in buffers of glc_compact_bound bytes with every count inside the
buffer (compact_decode_cases.pack): the tests pin the defined result and provoke nothing."""
import ctypes as C

import numpy as np
import pytest

import compact_decode_cases as K
import conftest as cf
import roundtrip_cases as RC
from conftest import O

pytestmark = pytest.mark.gpu

HOP, FRAME = K.HOP, K.FRAME
F32 = np.float32
EINVAL = -1
NAN_BITS = 0x7FC00ABC        # a NaN payload nothing computes
ROUND = 4096                 # glc_api.hip kDecodeChunkFrames
SR = 44100


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_decode_device_compact")
    yield g
    _ctx.clear()             # contexts: released while the library is still loaded


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


_ctx = {}


def ctx(g, kind, ch=2, sr=SR):
    """One context per (kind, channels, sample rate) for the module.  "dec": decodes compact blobs on the device;
    "host": the host path the expectations come from, which sees nothing else."""
    key = (kind, ch, sr)
    if key not in _ctx:
        _ctx[key] = g.Encoder(sr) if kind == "enc" else g.Decoder(ch, sr)
    return _ctx[key]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def host_decode(g, blob, n_samples, ch, sr=SR):
    """glc_decode(glc_frames_from_compact(blob)): the expectation."""
    enc = g.EncodedAudio.from_compact(sr, n_samples, ch, [np.ascontiguousarray(blob, np.uint8)])
    return ctx(g, "host", ch, sr).decode(enc).copy()


def dev_decode(g, torch, blob, cap_bytes, n_samples, ch, sr=SR, lead=0, guard=64):
    """glc_decode_device_compact of a blob uploaded as it stands; NaN-pattern guards in front of and behind the
    output must survive.  -> (samples, status)."""
    dec = ctx(g, "dec", ch, sr)
    d_blob = blob if isinstance(blob, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(blob, np.uint8)).cuda()
    assert d_blob.data_ptr() % 64 == 0
    out = torch.from_numpy(np.full(lead + n_samples + guard, NAN_BITS, np.uint32).view(F32)).cuda()
    torch.cuda.synchronize()
    n = dec.decode_device_compact(d_blob.data_ptr(), cap_bytes, n_samples, ch, out.data_ptr() + 4 * lead, n_samples)
    dec.synchronize()
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    o = out.cpu().numpy()
    assert np.all(o[:lead].view(np.uint32) == NAN_BITS) and np.all(o[lead + n:].view(np.uint32) == NAN_BITS)
    st = dec.last_compact_status()
    assert len(st) == 1
    return o[lead:lead + n], st[0]


def clean(st):
    return (st.flags, st.n_bad_rows, st.first_bad_row) == (0, 0, 0)


# ------------------------------------------------------------------------------------------ 1: natural streams

def half_noise_half_tone(sr, ch):
    """white noise, then a tone: raw frames, then compressed ones"""
    return np.concatenate([RC.lcg_noise(6 * HOP * ch), cf.gen_tone("sine", 440.0, sr, ch, 6 * HOP / sr)])


NATURAL = [
    ("shortest-mono", 1, lambda: RC.chord(SR, 1, 513), None),
    ("shortest-6ch", 6, lambda: RC.chord(SR, 6, 513), None),
    ("tone-12-frames-stereo", 2, lambda: cf.gen_tone("sine", 440.0, SR, 2, 12 * HOP / SR)[:12 * HOP * 2], "tonal"),
    ("silence-stereo", 2, lambda: np.zeros(3 * HOP * 2 + 10, F32), "silence"),
    ("noise-then-tone-stereo", 2, lambda: half_noise_half_tone(SR, 2), "mixed"),
    ("chord-mono", 1, lambda: RC.chord(SR, 1, 5 * HOP + 300), None),
    ("chord-stereo", 2, lambda: RC.chord(SR, 2, 5 * HOP + 1), None),
    ("chord-3ch", 3, lambda: RC.chord(SR, 3, 4 * HOP + 300), None),
    ("chord-6ch", 6, lambda: RC.chord(SR, 6, 3 * HOP), None),
]


def blob_sections(blob, ch):
    nf = int(np.frombuffer(blob[8:16].tobytes(), np.uint64)[0])
    o_israw, o_scale, o_cnt, o_pairs, _ = K.layout(ch, nf)
    m = nf * ch
    return (nf, blob[o_israw:o_israw + nf], blob[o_scale:o_scale + 4 * m].view(np.uint32), blob[o_cnt:o_cnt + 4 * m].view(np.uint32),
            o_scale)


@pytest.mark.parametrize("name,ch,make,want", NATURAL, ids=[c[0] for c in NATURAL])
def test_natural_stream_from_both_packers(glc_amd, torch, name, ch, make, want):
    g = glc_amd
    x = np.ascontiguousarray(make(), F32)
    assert x.size % ch == 0
    enc = ctx(g, "enc")
    # the device's blob: encode + compaction on the device
    xt = torch.from_numpy(x).cuda()
    d_blob, info = enc.encode_compact_tensor(xt, ch)
    assert d_blob.numel() == info.bytes and d_blob.data_ptr() % 64 == 0
    dev_blob = d_blob.cpu().numpy()
    # the host's blob: glc_frames_to_compact of glc_encode's stream
    stream = enc.encode(x, ch)
    host_blob = np.frombuffer(g.frames_to_compact(stream), np.uint8).copy()
    nf, israw, scale, cnt, o_scale = blob_sections(dev_blob, ch)
    # byte for byte - but for the scale words of the rows of raw frames: the encoder's records keep the quantiser's
    # scale there, EncodedAudio holds none (no decoder reads it) and glc_frames_to_compact writes +0.0
    a, b = dev_blob.copy(), host_blob.copy()
    raw_rows = np.repeat(israw.astype(bool), ch)
    for blob in (a, b):
        blob[o_scale:o_scale + 4 * nf * ch].view(np.uint32)[raw_rows] = 0
    assert a.size == b.size and np.array_equal(a, b)
    if want == "silence":
        assert info.n_pairs == 0 and not cnt.any() and not israw.any()
        assert info.bytes == K.layout(ch, nf)[3]          # an empty pairs section, no raw section
    elif want == "mixed":
        assert israw.any() and not israw.all()
    elif want == "tonal":
        assert nf == 12 and not israw.any()
    ref = ctx(g, "host", ch).decode(stream).copy()
    assert np.array_equal(bits(ref), bits(host_decode(g, dev_blob, x.size, ch)))
    oracle = O.decode(O.encode(x, SR, ch).glc)[0]
    assert np.array_equal(bits(ref), bits(oracle))
    for blob in (dev_blob, host_blob):
        y, st = dev_decode(g, torch, blob, blob.size, x.size, ch, lead=1)     # 4-byte aligned, not 16
        assert y.size == x.size and np.array_equal(bits(y), bits(ref))
        assert clean(st)
    # the tensor call, on the blob where the encoder left it
    y = ctx(g, "dec", ch).decode_compact_tensor(d_blob, x.size)
    assert np.array_equal(bits(y.cpu().numpy()), bits(ref))


_long = {}


def long_clip(g, torch):
    """One frame more than a round, mono: (device blob, n_samples, glc_decode's samples), made once."""
    if not _long:
        n = (ROUND + 1) * HOP
        t = np.arange(n, dtype=np.float64)
        x = (0.3 * np.sin(2 * np.pi * 440.0 / SR * t) + 0.1 * np.sin(2 * np.pi * 1234.5 / SR * t)).astype(F32)
        enc = ctx(g, "enc")
        d_blob, info = enc.encode_compact_tensor(torch.from_numpy(x).cuda(), 1)
        assert info.n_frames == ROUND + 1
        ref = ctx(g, "host", 1).decode(enc.encode(x, 1)).copy()
        _long.update(blob=d_blob, n=n, ref=ref)
    return _long["blob"], _long["n"], _long["ref"]


def test_a_clip_of_one_frame_more_than_a_round(glc_amd, torch):
    d_blob, n, ref = long_clip(glc_amd, torch)
    y, st = dev_decode(glc_amd, torch, d_blob, d_blob.numel(), n, 1)
    assert np.array_equal(bits(y), bits(ref)) and clean(st)


# ------------------------------------------------------------------------------------------ 2: crafted blobs

def crafted():
    rng = np.random.RandomState(17)
    c = []
    # rows of 0, 1, 1023 and 1024 entries in every channel position
    lens = (0, 1, 1023, 1024, 63, 64, 65)
    c.append(("list-lengths-stereo", 2, [("c", [K.row(rng, lens[(f + 3 * ch_) % len(lens)]) for ch_ in range(2)]) for f in range(7)]))
    c.append(("raw-first-and-last-3ch", 3, [("raw", K.raw_planes(rng, 3))] + [("c", [K.row(rng, 20 + f) for _ in range(3)]) for f in range(4)] +
              [("raw", K.raw_planes(rng, 3))]))
    c.append(("alternating-raw-stereo", 2, [("raw", K.raw_planes(rng, 2)) if f % 2 else ("c", [K.row(rng, 10), K.row(rng, 0)])
                                            for f in range(9)]))
    c.append(("all-raw-mono", 1, [("raw", K.raw_planes(rng, 1)) for _ in range(3)]))
    ext = K.Row(np.array([0, 1, 511, 1022, 1023], np.uint16), np.array([-32768, 32767, -32768, 32767, -1], np.int16))
    inf = K.Row(np.array([5, 700], np.uint16), np.array([100, -100], np.int16), 0x7F800000)
    zero_q = K.Row(np.array([9], np.uint16), np.array([0], np.int16), 0x7F800000)      # a stored zero times inf: NaN
    c.append(("extremes-and-inf-stereo", 2, [("c", [ext, inf]), ("c", [zero_q, ext]), ("c", [K.row(rng, 3), K.row(rng, 4)])]))
    # row counts below, at and above a wave quartet (a k_r2_rows workgroup) and a scan block
    for rows in (3, 4, 5, K.SCAN_BLOCK - 1, K.SCAN_BLOCK, K.SCAN_BLOCK + 1, 2 * K.SCAN_BLOCK + 1):
        fr = [("raw", K.raw_planes(rng, 1)) if f in (1, K.SCAN_BLOCK - 1, K.SCAN_BLOCK) and f < rows - 1
              else ("c", [K.row(rng, (f * 7) % 5)]) for f in range(rows)]
        c.append((f"rows-{rows}-mono", 1, fr))
    c.append(("rows-1026-3ch", 3, [("raw", K.raw_planes(rng, 3)) if f == 341 else ("c", [K.row(rng, (f + k) % 4) for k in range(3)])
                                   for f in range(342)]))
    return c


CRAFTED = crafted()


@pytest.mark.parametrize("name,ch,frames", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted_blob_decodes_as_the_host_path(glc_amd, torch, name, ch, frames):
    g = glc_amd
    buf, nbytes = K.pack(ch, frames)
    n = K.n_samples_of(ch, len(frames))
    ref = host_decode(g, buf[:nbytes], n, ch)
    y, st = dev_decode(g, torch, buf[:nbytes], nbytes, n, ch)
    assert np.array_equal(bits(y), bits(ref)) and clean(st)
    if "inf" in name:
        assert np.isnan(y).any()
    # ... and the row tables themselves
    got = rows_of(g, torch, buf[:nbytes], nbytes, len(frames), ch)
    for a, b in zip(got[:3], K.tables(ch, frames)):
        assert np.array_equal(a, b)


def rows_of(g, torch, blob, cap_bytes, nf, ch):
    """(row_begin, row_cnt, row_raw, status) through glc_debug_rows_from_compact."""
    f = g.lib.glc_debug_rows_from_compact
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16] + [C.c_void_p] * 6
    m = nf * ch
    begin, cnt, raw = np.empty(m, np.uint64), np.empty(m, np.uint32), np.empty(m, np.int64)
    st = (C.c_uint64 * 3)()
    d = torch.from_numpy(np.ascontiguousarray(blob, np.uint8)).cuda()
    torch.cuda.synchronize()
    rc = f(ctx(g, "dec", ch)._h, d.data_ptr(), cap_bytes, nf, ch, begin.ctypes.data, cnt.ctypes.data, None, raw.ctypes.data, None,
           C.addressof(st))
    assert rc == 0
    return begin, cnt, raw, (st[0] & 0xFFFFFFFF, st[1], st[2])


def test_second_chunk_of_the_block_sum_scan(glc_amd, torch):
    """More than 1024 blocks of 1024 rows: the one-workgroup scan of the block sums takes a second chunk and
    carries the first one's total into it.  The tables are compared (decoding a million frames is no unit test)."""
    nf = K.SCAN_BLOCK * K.SCAN_BLOCK + K.SCAN_BLOCK + 7
    edge = K.SCAN_BLOCK * K.SCAN_BLOCK
    buf, nbytes, want = K.big_mono(nf, (0, 5, edge - 1, edge, edge + 1, nf - 1))
    begin, cnt, raw, st = rows_of(glc_amd, torch, buf, nbytes, nf, 1)
    assert st == (0, 0, 0)
    assert np.array_equal(cnt, want[1]) and np.array_equal(begin, want[0]) and np.array_equal(raw, want[2])


# ------------------------------------------------------------------------------------------ 3: the call's edges

def small_stream(seed=3, ch=2, nf=5):
    rng = np.random.RandomState(seed)
    return [("c", [K.row(rng, 10 + 3 * f + c) for c in range(ch)]) for f in range(nf)]


def test_cap_zero_sizes_the_output(glc_amd, torch):
    g = glc_amd
    dec = ctx(g, "dec", 2)
    buf, nbytes = K.pack(2, small_stream())
    d = torch.from_numpy(buf).cuda()
    n = K.n_samples_of(2, 5) - 3 * 2
    got = C.c_uint64(77)
    rc = g.lib.glc_decode_device_compact(dec._h, d.data_ptr(), nbytes, n, 2, None, 0, C.byref(got))
    assert rc == EINVAL and got.value == n


def test_arguments_refused_before_anything_is_queued(glc_amd, torch):
    g = glc_amd
    dec = ctx(g, "dec", 2)
    buf, nbytes = K.pack(2, small_stream())
    d = torch.from_numpy(buf).cuda()
    n = K.n_samples_of(2, 5)
    out = torch.from_numpy(np.full(n + 64, NAN_BITS, np.uint32).view(F32)).cuda()
    got = C.c_uint64()
    call = lambda blob, nb, ns, ch, o, cap: g.lib.glc_decode_device_compact(dec._h, blob, nb, ns, ch, o, cap, C.byref(got))
    o_pairs = K.layout(2, 5)[3]
    assert call(None, nbytes, n, 2, out.data_ptr(), n) == EINVAL
    assert call(d.data_ptr() + 32, nbytes - 32, n, 2, out.data_ptr(), n) == EINVAL          # not 64-byte aligned
    assert call(d.data_ptr(), o_pairs - 1, n, 2, out.data_ptr(), n) == EINVAL               # below the fixed sections
    assert call(d.data_ptr(), nbytes, n, 0, out.data_ptr(), n) == EINVAL
    assert call(d.data_ptr(), nbytes, 2 * 512, 2, out.data_ptr(), n) == EINVAL              # the encoder refuses it
    assert call(d.data_ptr(), nbytes, n, 2, out.data_ptr() + 2, n) == EINVAL
    assert call(d.data_ptr(), nbytes, n, 2, out.data_ptr(), n - 1) == EINVAL and got.value == n
    assert call(d.data_ptr(), nbytes, n, 2, d.data_ptr() + 64, n) == EINVAL                 # the output overlaps the blob
    hook = g.lib.glc_debug_rows_from_compact                                                # the R2 hook checks a blob as the call does
    hook.restype, hook.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16] + [C.c_void_p] * 6
    st = (C.c_uint64 * 3)()
    for blob_at, nb in ((d.data_ptr() + 32, nbytes - 32), (d.data_ptr(), o_pairs - 1), (None, nbytes)):
        assert hook(dec._h, blob_at, nb, 5, 2, None, None, None, None, None, C.addressof(st)) == EINVAL
        assert b"glc_debug_rows_from_compact" in g.lib.glc_last_error(dec._h)
    window = g.lib.glc_debug_rows_from_compact_window                                       # ... and so does its window twin
    window.restype, window.argtypes = C.c_int, hook.argtypes[:5] + [C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
    for blob_at, nb in ((d.data_ptr() + 32, nbytes - 32), (d.data_ptr(), o_pairs - 1), (None, nbytes)):
        assert window(dec._h, blob_at, nb, 5, 2, 1, 3, None, None, None, None, None, C.addressof(st)) == EINVAL
        assert b"glc_debug_rows_from_compact_window" in g.lib.glc_last_error(dec._h)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)
    assert call(d.data_ptr(), o_pairs, n, 2, out.data_ptr(), n) == 0                        # the minimum passes the host
    dec.synchronize()


def test_context_state_afterwards(glc_amd, torch):
    """No stream is resident, and a glc_decode of another stream that follows is what it always was."""
    g = glc_amd
    dec = ctx(g, "dec", 2)
    x = RC.chord(SR, 2, 4 * HOP + 100)
    stream = ctx(g, "enc").encode(x, 2)
    before = dec.decode(stream).copy()
    assert g.lib.glc_ctx_resident_stream(dec._h) != 0
    buf, nbytes = K.pack(2, small_stream())
    dev_decode(g, torch, buf[:nbytes], nbytes, K.n_samples_of(2, 5), 2)
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    assert np.array_equal(bits(dec.decode(stream)), bits(before))


def test_status_needs_a_call(glc_amd):
    dec = glc_amd.Decoder(2, SR)
    st = glc_amd._lib.GlcCompactStatus()
    assert glc_amd.lib.glc_decode_compact_last_status(dec._h, C.byref(st), 1) == EINVAL
    dec.close()


# ------------------------------------------------------------------------------------------ 4: batches

_clips = {}


def clip_pool(g, torch, ch):
    """A few clips of mixed lengths, raw frames among them: (device blob, n_samples, samples of the single call)."""
    if ch not in _clips:
        enc = ctx(g, "enc")
        xs = [RC.chord(SR, ch, 513), RC.chord(SR, ch, 2 * HOP + 77, seed=2), RC.lcg_noise((HOP + 5) * ch), RC.chord(SR, ch, 5 * HOP, seed=5),
              np.concatenate([RC.lcg_noise(2 * HOP * ch, seed=9), RC.chord(SR, ch, 3 * HOP + 1, seed=6)]), np.zeros(700 * ch, F32)]
        pool = []
        for x in xs:
            d_blob, _ = enc.encode_compact_tensor(torch.from_numpy(np.ascontiguousarray(x, F32)).cuda(), ch)
            d_blob = d_blob.clone()                       # a tensor of exactly the blob's bytes
            y, st = dev_decode(g, torch, d_blob, d_blob.numel(), x.size, ch)
            assert clean(st)
            assert np.array_equal(bits(y), bits(host_decode(g, d_blob.cpu().numpy(), x.size, ch)))
            pool.append((d_blob, x.size, y))
        _clips[ch] = pool
    return _clips[ch]


def check_batch(g, torch, ch, clips, planar, margin=0):
    """Decode `clips` into a NaN-pattern tensor (a slice of a bigger one when margin > 0) and hold every element to
    the single call's samples / to the pattern."""
    dec = ctx(g, "dec", ch)
    b = len(clips)
    t_max = max(n // ch for _, n, _ in clips)
    shape = (b + margin, ch + margin, t_max + 3 * margin) if planar else (b + margin, t_max + margin, ch)
    big = torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(F32)).cuda()
    out = big[:b, :ch, margin:margin + t_max] if planar else big[:b, :t_max, :]
    got = dec.decode_compact_batch_tensor([c[0] for c in clips], [c[1] for c in clips], planar=planar, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    host = big.cpu().numpy()
    want = np.full(shape, NAN_BITS, np.uint32)
    for i, (_, n, y) in enumerate(clips):
        per = n // ch
        if planar:
            want[i, :ch, margin:margin + per] = bits(y).reshape(per, ch).T
        else:
            want[i, :per, :] = bits(y).reshape(per, ch)
    assert np.array_equal(host.view(np.uint32), want)
    st = dec.last_compact_status()
    assert len(st) == b and all(clean(s) for s in st)


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("n_clips", (1, 2, 64, 300))
def test_batch_equals_the_single_call(glc_amd, torch, n_clips, planar):
    pool = clip_pool(glc_amd, torch, 2)
    clips = [pool[(i * 5 + 1) % len(pool)] for i in range(n_clips)]
    check_batch(glc_amd, torch, 2, clips, planar)


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_batch_into_a_slice_of_a_bigger_tensor(glc_amd, torch, planar):
    pool = clip_pool(glc_amd, torch, 3)
    check_batch(glc_amd, torch, 3, [pool[i % len(pool)] for i in range(7)], planar, margin=2)


def test_batch_of_several_rounds(glc_amd, torch):
    """More frames than a round holds: 900 clips of up to 6 frames."""
    pool = clip_pool(glc_amd, torch, 1)
    check_batch(glc_amd, torch, 1, [pool[(i * 7 + 3) % len(pool)] for i in range(900)], True)


def test_batch_with_a_clip_longer_than_a_round(glc_amd, torch):
    d_blob, n, ref = long_clip(glc_amd, torch)
    pool = clip_pool(glc_amd, torch, 1)
    check_batch(glc_amd, torch, 1, [pool[1], (d_blob, n, ref), pool[4], pool[0]], True)


def test_batch_arguments(glc_amd, torch):
    g = glc_amd
    dec = ctx(g, "dec", 2)
    pool = clip_pool(g, torch, 2)
    assert g.lib.glc_decode_batch_device_compact(dec._h, None, None, None, None, C.byref(g._lib.GlcClipLayout(0, 2, 1, 0, 0, 0, None))) == 0
    blobs, ns = [pool[0][0], pool[1][0]], [pool[0][1], pool[1][1]]
    with pytest.raises(g.GlcError) as e:      # a length that is not the decoded length
        dec.decode_compact_batch_tensor(blobs, ns, lengths=[ns[0] // 2, ns[1] // 2 - 1])
    assert e.value.code == EINVAL
    with pytest.raises(g.GlcError) as e:      # a blob that is not 64-byte aligned
        dec.decode_compact_batch_tensor([blobs[0], torch.cat([blobs[1], blobs[1]])[32:32 + blobs[1].numel()]], ns)
    assert e.value.code == EINVAL


# ------------------------------------------------------------------------------------------ 5: blobs the check refuses

def refused():
    rng = np.random.RandomState(23)
    ch = 2
    base = [("c", [K.row(rng, 12 + f), K.row(rng, 30 - f)]) for f in range(5)]
    with_raw = [("c", [K.row(rng, 8), K.row(rng, 9)]), ("raw", K.raw_planes(rng, 2)), ("c", [K.row(rng, 5), K.row(rng, 6)]),
                ("raw", K.raw_planes(rng, 2)), ("c", [K.row(rng, 7), K.row(rng, 3)])]
    m = 10
    o_pairs = K.layout(ch, 5)[3]
    n_true = sum(len(r.idx) for _, body in base for r in body)
    c = []
    # (name, frames, pack overrides, capacity (None: the buffer), rows that decode empty (None: all), flags, n_bad, first)
    c.append(("wrong-magic", base, dict(magic=K.MAGIC ^ 0x100), None, None, K.BAD_HEADER, m, 0))
    c.append(("wrong-frame-count", base, dict(n_frames=4), None, None, K.BAD_HEADER, m, 0))
    c.append(("bytes-above-the-capacity", base, {}, "short", None, K.BAD_HEADER, m, 0))
    c.append(("bytes-not-the-sum-of-the-sections", base, dict(bytes_field=K.align64(o_pairs + 4 * n_true) + 64), None, None,
              K.BAD_HEADER, m, 0))
    # the header promises one pair less than the rows hold: the last row ends behind n_pairs
    c.append(("row-behind-n_pairs", base, dict(n_pairs=n_true - 1, bytes_field=K.align64(o_pairs + 4 * (n_true - 1))), None, [9],
              K.ROW_BOUNDS | K.PAIR_SUM, 1, 9))
    c.append(("sum-one-short-of-n_pairs", base, dict(n_pairs=n_true + 1, bytes_field=K.align64(o_pairs + 4 * (n_true + 1))), None, [],
              K.PAIR_SUM, 0, 0))
    bad_lists = {"repeated-bin": [3, 40, 40, 900], "descending": [3, 900, 40, 1000], "bin-1024": [3, 40, 900, 1024],
                 "bin-0xFFFF": [3, 40, 0xFFFF], "first-bin-1024": [1024], "descending-across-a-stride": list(range(64)) + [63]}
    for name, idx in bad_lists.items():
        fr = [(k, list(body)) for k, body in base]
        fr[2][1][1] = K.Row(np.array(idx, np.uint16), np.arange(1, len(idx) + 1, dtype=np.int16))
        c.append((name, fr, {}, None, [5], K.NOT_CANONICAL, 1, 5))
    # two raw frames, a header (and a raw section) that hold one
    bufr, nb = K.pack(ch, with_raw)
    c.append(("raw-row-beyond-n_raw_rows", with_raw, dict(n_raw_rows=2, bytes_field=nb - 2 * 4096), None, [6, 7],
              K.RAW_RANGE | K.RAW_SUM, 2, 6))
    return c


REFUSED = refused()


@pytest.mark.parametrize("name,frames,over,cap,empty,flags,n_bad,first", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_blob_has_a_defined_result(glc_amd, torch, name, frames, over, cap, empty, flags, n_bad, first):
    g = glc_amd
    ch = 2
    buf, nbytes = K.pack(ch, frames, **over)
    assert buf.size == g.compact_bound(ch, len(frames))
    n = K.n_samples_of(ch, len(frames))
    # the expectation: the same description with the rejected rows' lists emptied, through the host path
    good, gbytes = K.pack(ch, K.emptied(ch, frames, empty or (), all_rows=empty is None))
    ref = host_decode(g, good[:gbytes], n, ch)
    if empty is None:
        assert not bits(ref).any()          # all lists empty, scale 0, no raw frames: +0.0 everywhere
    y, st = dev_decode(g, torch, buf, nbytes - 64 if cap == "short" else buf.size, n, ch)
    assert np.array_equal(bits(y), bits(ref))
    assert (st.flags, st.n_bad_rows, st.first_bad_row) == (flags, n_bad, first)


def test_refused_blob_in_a_batch_leaves_its_neighbours_alone(glc_amd, torch):
    g = glc_amd
    pool = clip_pool(g, torch, 2)
    name, frames, over, cap, empty, flags, n_bad, first = next(c for c in REFUSED if c[0] == "descending")
    buf, nbytes = K.pack(2, frames, **over)
    good, gbytes = K.pack(2, K.emptied(2, frames, empty))
    n = K.n_samples_of(2, len(frames))
    bad = (torch.from_numpy(buf).cuda(), n, host_decode(g, good[:gbytes], n, 2))
    dec = ctx(g, "dec", 2)
    clips = [pool[3], bad, pool[2]]
    out = dec.decode_compact_batch_tensor([c[0] for c in clips], [c[1] for c in clips], planar=False)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for i, (_, n_i, y) in enumerate(clips):
        assert np.array_equal(bits(host[i, :n_i // 2, :]).reshape(-1), bits(y))
    st = dec.last_compact_status()
    assert clean(st[0]) and clean(st[2]) and (st[1].flags, st[1].n_bad_rows, st[1].first_bad_row) == (flags, n_bad, first)
