"""The device round trip: glc_roundtrip / glc_roundtrip_device / glc_decode_device_records decode frame records
where the encoder left them (row tables built by a kernel, no stream on the host).

Every comparison is bit for bit - float32 viewed as uint32, tolerance 0.  The CPU oracle is the truth for
the round trip itself; the library's own two-step path (Encoder.encode + Decoder.decode, which the other
suites hold to the oracle) is the expectation for long streams, integer PCM and hand-made records."""
import ctypes as C

import numpy as np
import pytest

import conftest as cf
import roundtrip_cases as RC
from conftest import O

pytestmark = pytest.mark.gpu

HOP, FRAME = RC.HOP, RC.FRAME
F32 = np.float32
EINVAL = -1
NAN_BITS = 0x7FC00ABC        # a NaN payload nothing computes


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    yield g
    _ctx.clear()             # contexts: released while the library is still loaded


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


_ctx = {}


def ctx(g, kind, sr):
    """One context per (kind, sample rate) for the module: its tables take longer to build than a test runs."""
    if (kind, sr) not in _ctx:
        _ctx[(kind, sr)] = {"rt": lambda: g.RoundTrip(sr), "enc": lambda: g.Encoder(sr), "dec": lambda: g.Decoder(2, sr)}[kind]()
    return _ctx[(kind, sr)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def two_step(g, sr, x, ch, bits_=None, dtype=F32):
    """The library's own encode, then decode, on contexts that see nothing else of the test."""
    enc = ctx(g, "enc", sr).encode(x, ch, bits=bits_)
    return enc, ctx(g, "dec", sr).decode(enc, dtype=dtype).copy()


# ------------------------------------------------------------------------------------------ 1: the oracle

CASES = RC.oracle_cases()
_oracle = {}


def oracle_of(name):
    if name not in _oracle:
        _, sr, ch, x, _ = next(c for c in CASES if c[0] == name)
        glc = O.encode(x, sr, ch).glc
        _oracle[name] = (glc, O.decode(glc)[0])
    return _oracle[name]


@pytest.mark.parametrize("name,sr,ch,x,want", CASES, ids=[c[0] for c in CASES])
def test_apply_equals_oracle_decode_of_oracle_encode(glc_amd, name, sr, ch, x, want):
    glc, ref = oracle_of(name)
    raw = [f["raw"] is not None for f in cf.parse_glc(glc)["frames"]]
    if want == "tonal":
        assert not any(raw)
    elif want == "noise":
        assert any(raw)
    elif want == "mixed":
        assert any(raw) and not all(raw)
        assert any(raw[i] != raw[i + 1] for i in range(len(raw) - 1))
    rt = ctx(glc_amd, "rt", sr)
    y = rt.apply(x, ch)
    assert y.dtype == F32 and y.size == ref.size == x.size
    assert np.array_equal(bits(y), bits(ref))
    assert rt.resident_stream() == 0


@pytest.mark.parametrize("name,sr,ch,x,want", CASES, ids=[c[0] for c in CASES])
def test_last_info_equals_info_of_encode(glc_amd, name, sr, ch, x, want):
    rt = ctx(glc_amd, "rt", sr)
    rt.apply(x, ch)
    got = rt.last_info()
    enc = ctx(glc_amd, "enc", sr).encode(x, ch)
    i = enc.info()
    assert (got.n_frames, got.n_raw_frames, got.total_nnz) == (i.n_frames, i.n_raw_frames, i.total_nnz)
    assert got.serialized_bytes == glc_amd.lib.glc_serialized_size(enc._h) == len(oracle_of(name)[0])


def test_last_info_needs_a_round_trip(glc_amd):
    rt = glc_amd.RoundTrip(44100)
    with pytest.raises(glc_amd.GlcError) as e:
        rt.last_info()
    assert e.value.code == EINVAL
    rt.close()


# ------------------------------------------------------------------------------------------ 2: the two-step path

def device_roundtrip(g, torch, rt, x, ch, guard=64, lead=0):
    """glc_roundtrip_device through torch tensors: the result, and the guard words around it."""
    xt = torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()
    out = torch.from_numpy(np.full(lead + x.size + guard, NAN_BITS, np.uint32).view(F32)).cuda()
    torch.cuda.synchronize()
    n = g.RoundTrip.apply_device(rt, xt.data_ptr(), x.size, ch, out.data_ptr() + 4 * lead, x.size)
    rt.synchronize()
    assert g.lib.glc_ctx_resident_stream(rt._h) == 0
    o = out.cpu().numpy()
    assert np.all(o[:lead].view(np.uint32) == NAN_BITS) and np.all(o[lead + n:].view(np.uint32) == NAN_BITS)
    return o[lead:lead + n]


@pytest.mark.parametrize("name", ["sine-44k-stereo", "chord-96k-6ch", "noise-48k-stereo", "mixed-48k-stereo", "mixed-44k-mono",
                                  "shortest-44k-mono", "chord-48k-mono-hop+1"])
def test_device_and_host_calls_equal_encode_then_decode(glc_amd, torch, name):
    _, sr, ch, x, _ = next(c for c in CASES if c[0] == name)
    _, ref = two_step(glc_amd, sr, x, ch)
    rt = ctx(glc_amd, "rt", sr)
    assert np.array_equal(bits(rt.apply(x, ch)), bits(ref))
    assert np.array_equal(bits(device_roundtrip(glc_amd, torch, rt, x, ch)), bits(ref))
    # a destination 4 bytes off a 16-byte boundary
    assert np.array_equal(bits(device_roundtrip(glc_amd, torch, rt, x, ch, lead=1)), bits(ref))
    # ... and into a caller's array
    buf = np.zeros(x.size + 5, F32)
    y = rt.apply(x, ch, out=buf)
    assert y.base is buf and np.array_equal(bits(y), bits(ref)) and not buf[x.size:].any()


@pytest.mark.parametrize("name", ["sine-44k-stereo", "noise-48k-stereo", "mixed-44k-mono", "chord-96k-6ch"])
def test_int16_output_equals_decode_i16(glc_amd, name):
    _, sr, ch, x, _ = next(c for c in CASES if c[0] == name)
    _, ref = two_step(glc_amd, sr, x, ch, dtype=np.int16)
    y = ctx(glc_amd, "rt", sr).apply(x, ch, dtype=np.int16)
    assert y.dtype == np.int16 and np.array_equal(y, ref)


@pytest.mark.parametrize("dtype,nbits", [(np.int16, 16), (np.int16, 12), (np.int32, 24), (np.int32, 32), (np.int32, 16)])
@pytest.mark.parametrize("out_dtype", [F32, np.int16])
def test_integer_input_equals_encode_int_then_decode(glc_amd, dtype, nbits, out_dtype):
    sr, ch = 48000, 2
    x = RC.mixed_clip(sr, ch)
    lim = float(2 ** (nbits - 1))
    xi = np.clip(np.round(x.astype(np.float64) * lim), -lim, lim - 1).astype(dtype)
    _, ref = two_step(glc_amd, sr, xi, ch, bits_=nbits, dtype=out_dtype)
    y = ctx(glc_amd, "rt", sr).apply(xi, ch, bits=nbits, dtype=out_dtype)
    assert y.dtype == out_dtype and y.size == ref.size
    assert np.array_equal(y.view(np.uint32 if out_dtype == F32 else np.int16), ref.view(np.uint32 if out_dtype == F32 else np.int16))


# (two rounds, the last of a single frame: the integer samples of the second go up, and are widened, on the helper thread)
@pytest.mark.parametrize("ch,n_frames,dtype,nbits,out_dtype", [(1, 4097, np.int16, 16, F32), (2, 2049, np.int32, 24, np.int16)])
def test_integer_input_over_two_rounds_equals_encode_int_then_decode(glc_amd, ch, n_frames, dtype, nbits, out_dtype):
    sr = 44100
    per_channel = n_frames * HOP - 100
    assert RC.frames_of(per_channel) == n_frames
    seg = np.concatenate([cf.gen_chord(sr, ch, 3 * HOP, seed=9), RC.lcg_noise(2 * HOP * ch)])
    x = np.resize(seg, per_channel * ch).astype(F32)
    lim = float(2 ** (nbits - 1))
    xi = np.clip(np.round(x.astype(np.float64) * lim), -lim, lim - 1).astype(dtype)
    _, ref = two_step(glc_amd, sr, xi, ch, bits_=nbits, dtype=out_dtype)
    y = ctx(glc_amd, "rt", sr).apply(xi, ch, bits=nbits, dtype=out_dtype)
    view = np.uint32 if out_dtype == F32 else np.int16
    assert y.dtype == out_dtype and y.size == ref.size == xi.size
    assert np.array_equal(y.view(view), ref.view(view))


def test_ten_minutes_of_stereo_cross_several_rounds(glc_amd, torch):
    sr, ch = 48000, 2
    seg = cf.gen_chord(sr, ch, 480000)
    x = np.tile(seg.reshape(-1, ch), (60, 1)).reshape(-1)
    assert RC.frames_of(x.size // ch) > 6 * 4096
    enc, ref = two_step(glc_amd, sr, x, ch)
    rt = ctx(glc_amd, "rt", sr)
    y = rt.apply(x, ch)
    assert np.array_equal(bits(y), bits(ref))
    i, got = enc.info(), rt.last_info()
    assert (got.n_frames, got.n_raw_frames, got.total_nnz) == (i.n_frames, i.n_raw_frames, i.total_nnz)
    assert got.serialized_bytes == glc_amd.lib.glc_serialized_size(enc._h)
    assert np.array_equal(bits(device_roundtrip(glc_amd, torch, rt, x, ch)), bits(ref))
    y16 = rt.apply(x, ch, dtype=np.int16)
    assert np.array_equal(y16, ctx(glc_amd, "dec", sr).decode(enc, dtype=np.int16))


# (glc_roundtrip_device works in rounds of 4096 frames, glc_roundtrip in rounds of 4096 rows)
@pytest.mark.parametrize("ch,n_frames", [(1, 4097), (2, 4097), (2, 4096), (1, 8193), (2, 2049), (6, 683), (3, 1366)])
def test_last_round_of_a_single_frame(glc_amd, torch, ch, n_frames):
    sr = 44100
    per_channel = n_frames * HOP - 100
    assert RC.frames_of(per_channel) == n_frames
    seg = np.concatenate([cf.gen_chord(sr, ch, 3 * HOP, seed=9), RC.lcg_noise(2 * HOP * ch)])
    x = np.resize(seg, per_channel * ch).astype(F32)
    _, ref = two_step(glc_amd, sr, x, ch)
    rt = ctx(glc_amd, "rt", sr)
    assert np.array_equal(bits(rt.apply(x, ch)), bits(ref))
    assert np.array_equal(bits(device_roundtrip(glc_amd, torch, rt, x, ch)), bits(ref))


# ------------------------------------------------------------------------------------------ 3: the kernel's edges

def decode_records_on_device(g, torch, dec, sr, ch, frames, sentinel=0, lead=1, guard=64):
    """glc_decode_device_records of hand-made records against glc_decode(glc_frames_from_records(them))."""
    records, per_channel = RC.build_records(ch, frames)
    n_samples = per_channel * ch
    ref = dec.decode(g.EncodedAudio.from_records(sr, n_samples, ch, records)).copy()
    assert ref.size == n_samples
    dev = np.concatenate([records, np.full(sentinel, 0xA5, np.uint8)])     # bytes behind the records: never rows
    rt = torch.from_numpy(dev).cuda()
    out = torch.from_numpy(np.full(lead + n_samples + guard, NAN_BITS, np.uint32).view(F32)).cuda()
    torch.cuda.synchronize()
    assert rt.data_ptr() % 16 == 0 and (out.data_ptr() + 4 * lead) % 16 == (4 * lead) % 16
    n = dec.decode_device_records(rt.data_ptr(), len(frames), n_samples, ch, out.data_ptr() + 4 * lead, n_samples)
    dec.synchronize()
    assert n == n_samples and dec.resident_stream() == 0
    o = out.cpu().numpy()
    assert np.all(o[:lead].view(np.uint32) == NAN_BITS), "written in front of d_out"
    assert np.all(o[lead + n:].view(np.uint32) == NAN_BITS), "written behind d_out[*n_out)"
    assert np.array_equal(bits(o[lead:lead + n]), bits(ref))
    return o[lead:lead + n]


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_row_edges(glc_amd, torch, ch):
    """0 / 1 / 63 / 64 / 65 / 1023 / 1024 non-zeros, k = 0 and k = 1023 alone, alternating entries, q = -32768 and 32767,
    scale 0 and denormal scales, an nnz field below the row's non-zeros - in every channel position; sentinel bytes behind
    the records, NaN guards around an output that starts 4 bytes off a 16-byte boundary."""
    y = decode_records_on_device(glc_amd, torch, ctx(glc_amd, "dec", 44100), 44100, ch, RC.edge_stream(ch), sentinel=8192)
    assert np.isfinite(y).all() and np.abs(y).max() > 0


@pytest.mark.parametrize("name", [r[0] for r in RC.edge_rows()])
def test_single_edge_row_alone(glc_amd, torch, name):
    """n_frames = 1, mono: the row is the whole stream."""
    row = next(r for r in RC.edge_rows() if r[0] == name)
    decode_records_on_device(glc_amd, torch, ctx(glc_amd, "dec", 48000), 48000, 1, [("c", [row[1:]])], sentinel=4096)


@pytest.mark.parametrize("where", ["first", "last", "every-other", "all", "none"])
@pytest.mark.parametrize("ch,n_frames", [(2, 5), (1, 1), (6, 2), (1, 9)])
def test_raw_frame_placement(glc_amd, torch, where, ch, n_frames):
    decode_records_on_device(glc_amd, torch, ctx(glc_amd, "dec", 96000), 96000, ch, RC.raw_placement(ch, n_frames, where),
                             sentinel=4096, lead=0 if where == "all" else 1)


def test_records_of_an_encode_decode_where_they_are(glc_amd, torch):
    """The use the call is for: encode_range_device, then the decode of its records, nothing crossing to the host."""
    sr, ch = 48000, 2
    x = RC.mixed_clip(sr, ch)
    enc_ref, ref = two_step(glc_amd, sr, x, ch)
    e = ctx(glc_amd, "rt", sr)
    nf = glc_amd.plan_encode(x.size, ch).n_frames
    xt = torch.from_numpy(x).cuda()
    recs = torch.zeros(nf * glc_amd.lib.glc_record_bytes(ch), dtype=torch.uint8, device="cuda")
    out = torch.zeros(x.size, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    glc_amd.Encoder.encode_range_device(e, xt.data_ptr(), 0, x.size // ch, x.size, ch, 0, nf, recs.data_ptr())
    n = glc_amd.Decoder.decode_device_records(e, recs.data_ptr(), nf, x.size, ch, out.data_ptr(), x.size)
    e.synchronize()
    assert n == x.size and np.array_equal(bits(out.cpu().numpy()), bits(ref))


# ------------------------------------------------------------------------------------------ 4: context state

def test_context_state_after_a_round_trip(glc_amd, torch):
    sr, ch = 44100, 2
    a = cf.gen_tone("sine", 440.0, sr, ch, 0.2)
    b = RC.mixed_clip(sr, ch)
    c = cf.gen_noise(sr, ch, 0.1, 3)
    enc_a, ref_a = two_step(glc_amd, sr, a, ch)
    enc_b, ref_b = two_step(glc_amd, sr, b, ch)
    glc_c = ctx(glc_amd, "enc", sr).encode(c, ch).to_bytes()
    one = glc_amd.Decoder(ch, sr)                    # ONE context does everything below
    RT, ENC = glc_amd.RoundTrip, glc_amd.Encoder
    assert np.array_equal(bits(one.decode(enc_a)), bits(ref_a))
    assert one.resident_stream() == enc_a.stream_id != 0
    # a round trip of other audio: nothing is resident afterwards ...
    assert np.array_equal(bits(RT.apply(one, b, ch)), bits(ref_b))
    assert one.resident_stream() == 0
    # ... the stream that was resident is uploaded again, not decoded from stale tables
    assert np.array_equal(bits(one.decode(enc_a)), bits(ref_a))
    assert one.resident_stream() == enc_a.stream_id
    assert np.array_equal(bits(device_roundtrip(glc_amd, torch, one, b, ch)), bits(ref_b))
    assert one.resident_stream() == 0
    # an unrelated stream decodes, an unrelated encode encodes
    assert np.array_equal(bits(one.decode(enc_b)), bits(ref_b))
    RT.apply(one, a, ch, dtype=np.int16)
    assert one.resident_stream() == 0
    assert ENC.encode(one, c, ch).to_bytes() == glc_c
    assert np.array_equal(bits(RT.apply(one, a, ch)), bits(ref_a))
    assert np.array_equal(bits(one.decode(enc_b)), bits(ref_b))
    # an open streaming session is closed by the call
    glc_amd.lib.glc_decode_stream_begin(one._h, enc_a._h)
    RT.apply(one, a, ch)
    n, last = C.c_uint64(), C.c_int()
    buf = np.empty(501 * HOP * ch, F32)
    assert glc_amd.lib.glc_decode_stream_next(one._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n), C.byref(last)) == EINVAL
    one.close()


# ------------------------------------------------------------------------------------------ 6: torch

@pytest.mark.parametrize("two_d", [False, True])
@pytest.mark.parametrize("name", ["mixed-48k-stereo", "chord-96k-6ch", "sine-44k-stereo"])
def test_apply_tensor_on_torchs_current_stream(glc_amd, torch, name, two_d):
    _, sr, ch, x, _ = next(c for c in CASES if c[0] == name)
    assert len(glc_amd._lib.hip_runtimes_mapped()) == 1
    rt = ctx(glc_amd, "rt", sr)
    ref = rt.apply(x, ch).copy()
    half = torch.from_numpy(x * F32(0.5)).cuda()
    if two_d:
        half = half.reshape(-1, ch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xt = half + half            # filled by a kernel on this stream: x * 0.5 * 2 is x exactly
        yt = rt.apply_tensor(xt, ch)
        zt = yt.clone()             # ... and read by one, with no synchronisation in between
    assert glc_amd.lib.glc_ctx_stream(rt._h) != side.cuda_stream      # the private stream is back
    side.synchronize()
    assert yt.shape == xt.shape and yt.device == xt.device and yt.dtype == torch.float32
    assert np.array_equal(bits(zt.cpu().numpy().reshape(-1)), bits(ref))
    assert np.array_equal(bits(xt.cpu().numpy().reshape(-1)), bits(x))


def test_apply_tensor_refuses_what_it_cannot_take(glc_amd, torch):
    rt = ctx(glc_amd, "rt", 44100)
    x = torch.zeros(4096, 2, device="cuda")
    with pytest.raises(TypeError):
        rt.apply_tensor(x.cpu(), 2)
    with pytest.raises(TypeError):
        rt.apply_tensor(x.double(), 2)
    with pytest.raises(TypeError):
        rt.apply_tensor(x.t(), 4096)
    with pytest.raises(glc_amd.GlcError):
        rt.apply_tensor(x, 3)
    with pytest.raises(glc_amd.GlcError):
        rt.apply_tensor(x.reshape(2, 2048, 2), 2)


# ------------------------------------------------------------------------------------------ 7: errors

def _roundtrip_rc(g, rt, x, fmt, nbits, ch, out, out_fmt, cap):
    n = C.c_uint64(12345)
    rc = g.lib.glc_roundtrip(rt._h, x.ctypes.data_as(C.c_void_p), fmt, nbits, x.size, ch, out.ctypes.data_as(C.c_void_p), out_fmt,
                             cap, C.byref(n))
    return rc, n.value, g.lib.glc_last_error(rt._h).decode()


def test_host_call_errors_write_nothing(glc_amd):
    rt = ctx(glc_amd, "rt", 44100)
    S16, S32, F = 1, 2, 3
    x = cf.gen_chord(44100, 2, 3000)
    xi = (x * 1000).astype(np.int16)
    out = np.full(x.size + 8, NAN_BITS, np.uint32)
    for args in [(x, F, 32, 0, out, F, out.size),                 # channels == 0
                 (x[:1024], F, 32, 2, out, F, out.size),          # 512 samples per channel: the reference panics
                 (x[:1025], F, 32, 2, out, F, out.size),          # ragged
                 (x, F, 32, 2, out, S32, out.size),               # no 32-bit integer output
                 (x, F, 32, 2, out, 0, out.size), (x, 7, 32, 2, out, F, out.size),
                 (xi, S16, 0, 2, out, F, out.size), (xi, S16, 17, 2, out, F, out.size), (xi.astype(np.int32), S32, 33, 2, out, F, out.size)]:
        rc, n, msg = _roundtrip_rc(glc_amd, rt, *args)
        assert rc == EINVAL and msg, args[1:4]
        assert np.all(out == NAN_BITS)
    for out_fmt in (F, S16):
        rc, n, msg = _roundtrip_rc(glc_amd, rt, x, F, 32, 2, out, out_fmt, x.size - 1)
        assert rc == EINVAL and "output buffer too small" in msg and n == x.size
        assert np.all(out == NAN_BITS)
    with pytest.raises(TypeError):
        rt.apply(x.astype(np.float64), 2)
    with pytest.raises(TypeError):
        rt.apply(x, 2, dtype=np.int32)
    with pytest.raises(glc_amd.GlcError):
        rt.apply(x, 2, out=np.empty(x.size - 1, F32))


def test_device_call_errors_write_nothing(glc_amd, torch):
    sr, ch = 44100, 2
    rt = ctx(glc_amd, "rt", sr)
    x = cf.gen_chord(sr, ch, 3000)
    nf = glc_amd.plan_encode(x.size, ch).n_frames
    xt = torch.from_numpy(x).cuda()
    recs = torch.zeros(nf * glc_amd.lib.glc_record_bytes(ch) + 16, dtype=torch.uint8, device="cuda")
    out = torch.from_numpy(np.full(x.size + 8, NAN_BITS, np.uint32).view(F32)).cuda()
    torch.cuda.synchronize()
    L, h = glc_amd.lib, rt._h
    n = C.c_uint64(777)

    def rtd(d_pcm, n_samples, c, d_out, cap):
        return L.glc_roundtrip_device(h, C.c_void_p(d_pcm), n_samples, c, C.c_void_p(d_out), cap, C.byref(n))

    def ddr(d_recs, frames, n_samples, c, d_out, cap):
        return L.glc_decode_device_records(h, C.c_void_p(d_recs), frames, n_samples, c, C.c_void_p(d_out), cap, C.byref(n))

    assert rtd(xt.data_ptr(), x.size, 0, out.data_ptr(), x.size) == EINVAL
    assert rtd(xt.data_ptr(), 1024, 2, out.data_ptr(), x.size) == EINVAL
    assert rtd(None, x.size, 2, out.data_ptr(), x.size) == EINVAL
    assert rtd(xt.data_ptr(), x.size, 2, None, x.size) == EINVAL
    assert rtd(xt.data_ptr(), x.size, 2, out.data_ptr() + 2, x.size) == EINVAL
    assert rtd(xt.data_ptr(), x.size, 2, out.data_ptr(), x.size - 1) == EINVAL and n.value == x.size
    assert "output buffer too small" in L.glc_last_error(h).decode()
    assert ddr(recs.data_ptr(), nf, x.size, 0, out.data_ptr(), x.size) == EINVAL
    assert ddr(recs.data_ptr(), nf + 1, x.size, 2, out.data_ptr(), x.size) == EINVAL
    assert ddr(recs.data_ptr(), nf - 1, x.size, 2, out.data_ptr(), x.size) == EINVAL
    assert ddr(None, nf, x.size, 2, out.data_ptr(), x.size) == EINVAL
    assert ddr(recs.data_ptr() + 8, nf, x.size, 2, out.data_ptr(), x.size) == EINVAL
    assert ddr(recs.data_ptr(), nf, x.size, 2, out.data_ptr(), x.size - 1) == EINVAL and n.value == x.size
    assert "output buffer too small" in L.glc_last_error(h).decode()
    rt.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)
