"""Integer PCM at the host boundary: glc_audio_load_pcm, the `_i16` writers, glc_pcm_widen_device,
glc_encode_int, glc_decode_i16 / glc_decode_stream_next_i16 / glc_decode_range_device_i16 and the CLI
that runs on them.

Expected values are numpy restatements of the reference's two expressions, written here and nowhere else:

  widen   load_wav / load_flac, src/audio.rs:52-60, :72-81:  s as f32 / (1 << (bits - 1)) as f32
          (the literal is an i32: at 32 bits the divisor is i32::MIN, quirk Q11)
  narrow  convert_f32_to_i16, src/audio.rs:11-16 = src/flac.rs:955-958:
          (s * 32767.0).clamp(-32768.0, 32767.0) as i16   - NaN gives 0, truncation toward zero

and every comparison is bit for bit.  Nothing here takes an expected value from the library under test;
where the issue asks for equality with a float twin (a loader, a writer, glc_encode, glc_decode), that
twin's output is one side of the comparison and the restatement applied to it the other.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import decode_edges as D
import flac_synth as S
import glc_amd
from conftest import ROOT, gen_chord, gen_noise, gen_tone
from oracle import flac_oracle as FO
from oracle import oracle as O

F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "build", "glc")
lib = glc_amd.lib
EINVAL, EIO = -1, -6
S16, S32, PF32 = 1, 2, 3


def widen(s, bits):
    mx = F32(-2147483648.0) if bits == 32 else F32(1 << (bits - 1))
    return np.asarray(s).astype(F32) / mx


def narrow(x):
    with np.errstate(all="ignore"):
        v = np.asarray(x, F32) * F32(32767.0)
    v = np.where(np.isnan(v), F32(0.0), v)
    return np.trunc(np.clip(v, F32(-32768.0), F32(32767.0))).astype(np.int16)


def bits_of(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def quantise16(x):
    """A float signal as the 16-bit file a user would have: finite, rounded, clipped."""
    return np.clip(np.rint(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=1.0, neginf=-1.0) * 32767.0),
                   -32768, 32767).astype(np.int16)


def _write_wav(path, fmt, bits, ch, sr, raw: bytes):
    block = ch * bits // 8
    body = struct.pack("<HHIIHH", fmt, ch, sr, sr * block, block, bits)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(body) + 8 + len(raw)) + b"WAVE" + b"fmt " +
                 struct.pack("<I", len(body)) + body + b"data" + struct.pack("<I", len(raw)) + raw)


# ----------------------------------------------------------------------------------------------------
# CPU 1: glc_audio_load_pcm
# ----------------------------------------------------------------------------------------------------

def _edges(lo, hi, rng, n):
    v = rng.integers(lo, hi + 1, n, dtype=np.int64)
    v[:6] = [lo, hi, 0, 1, -1, lo + 1]
    return v


def test_load_pcm_wav_keeps_the_integers(tmp_path):
    rng = np.random.default_rng(1)
    for bits, dt in [(8, np.int16), (16, np.int16), (24, np.int32), (32, np.int32)]:
        v = _edges(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, rng, 3001)
        if bits == 32:                           # beyond 24 bits: `as f32` rounds, ties to even
            v[6:12] = [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 30) + 64, (1 << 30) + 192, (1 << 31) - 1]
        if bits == 8:
            raw = (v + 128).astype(np.uint8).tobytes()        # WAV 8-bit is unsigned
        elif bits == 24:
            raw = b"".join(int(s).to_bytes(3, "little", signed=True) for s in v)
        else:
            raw = v.astype(dt).tobytes()
        p = tmp_path / f"i{bits}.wav"
        _write_wav(p, 1, bits, 3, 48000, raw)
        got, gbits, sr, ch = glc_amd.load_audio_file_pcm(p)
        assert (got.dtype, gbits, sr, ch) == (np.dtype(dt), bits, 48000, 3)
        assert np.array_equal(got.astype(np.int64), v)
        x, sr2, ch2 = glc_amd.load_wav(p)
        assert (sr2, ch2) == (sr, ch) and np.array_equal(bits_of(widen(got, gbits)), bits_of(x))
        if bits == 32:                           # inverted (quirk Q11), and -0.0 for a zero sample
            assert x[1] < 0 < x[0] and bits_of(x[2:3])[0] == 0x80000000
    f = rng.uniform(-2, 2, 2000).astype(F32)
    f[:4] = [np.nan, np.inf, -0.0, 1e-45]
    _write_wav(tmp_path / "f32.wav", 3, 32, 2, 44100, f.tobytes())
    got, gbits, sr, ch = glc_amd.load_audio_file_pcm(tmp_path / "f32.wav")
    assert (got.dtype, gbits, sr, ch) == (np.dtype(F32), 32, 44100, 2) and np.array_equal(bits_of(got), bits_of(f))
    assert np.array_equal(bits_of(glc_amd.load_wav(tmp_path / "f32.wav")[0]), bits_of(f))
    os.rename(tmp_path / "i16.wav", tmp_path / "UPPER.WAV")          # lower-cased extension, src/audio.rs:26
    assert glc_amd.load_audio_file_pcm(tmp_path / "UPPER.WAV")[1] == 16


def test_load_pcm_flac_golden_and_synthetic(tmp_path):
    names = sorted(n for n in os.listdir(GOLDEN) if n.endswith(".flac"))
    assert len(names) >= 5
    for n in names:
        p = os.path.join(GOLDEN, n)
        got, gbits, sr, ch = glc_amd.load_audio_file_pcm(p)
        x, sr2, ch2 = glc_amd.load_flac(p)
        assert (got.dtype, gbits, sr, ch) == (np.dtype(np.int16), 16, sr2, ch2)
        assert np.array_equal(bits_of(widen(got, 16)), bits_of(x)), n
    rng = np.random.default_rng(2)
    for bps, chn in [(8, 1), (12, 2), (16, 2), (20, 1), (24, 3), (32, 2)]:
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        pcm = _edges(lo, hi, rng, 256 * chn)
        if bps == 32:
            pcm[6:10] = [(1 << 24) + 1, (1 << 24) + 3, (1 << 30) + 64, (1 << 30) + 192]
        data = S.stream(pcm, chn, bps, 32000, [256], lambda i: [dict(kind="verbatim")] * chn)
        p = tmp_path / f"s{bps}.flac"
        p.write_bytes(data)
        got, gbits, sr, ch = glc_amd.load_audio_file_pcm(p)
        assert (got.dtype, gbits, sr, ch) == (np.dtype(np.int16 if bps <= 16 else np.int32), bps, 32000, chn)
        assert np.array_equal(got.astype(np.int64), pcm)
        x = glc_amd.load_flac(p)[0]
        assert np.array_equal(bits_of(widen(got, bps)), bits_of(x)) and np.array_equal(bits_of(x), bits_of(glc_amd.decode_flac(data)[0]))


# ----------------------------------------------------------------------------------------------------
# CPU 2: the writers without their conversion step
# ----------------------------------------------------------------------------------------------------

def hostile_vector():
    """Floats on every decision of the narrowing: NaN, the infinities, signed zeros, full scale, the first
    float whose product passes 32767, one ulp either side of k / 32767, products within an ulp of the clamps."""
    one = F32(1.0)
    v = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1.0000305, -1.0000305, 1e-45, -1e-45, 3.4e38, -3.4e38]
    for k in (1, 2, 3, 100, 12345, 16384, 32766, 32767, 32768):
        for s in (1, -1):
            c = F32(s * k) / F32(32767.0)
            v += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    for target in (32767.0, -32767.0, -32768.0, 32766.0, 0.5, -0.5, 0.99999, -0.99999, 1.5, -1.5):
        c = F32(target) / F32(32767.0)
        for _ in range(3):
            c = np.nextafter(c, F32(-np.inf))
        for _ in range(7):
            v.append(c)
            c = np.nextafter(c, F32(np.inf))
    v += [np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), np.nextafter(-one, F32(0)), np.nextafter(-one, F32(-2))]
    return np.array(v, F32)


def test_the_restated_narrowing_hits_its_decisions():
    x = hostile_vector()
    q = narrow(x)
    with np.errstate(all="ignore"):
        v = x * F32(32767.0)
    fin = np.isfinite(v) & (np.abs(v) < 32767)
    assert q.min() == -32768 and q.max() == 32767 and (q[np.isnan(x)] == 0).all()
    assert (np.rint(v[fin]) != np.trunc(v[fin])).any() and (q[np.isinf(x)] != 0).all()
    assert {32766, -32767, 0, 1, -1} <= set(q.tolist())


def _flac_inputs():
    yield "hostile", np.tile(hostile_vector(), 3), 44100, 2
    for n in sorted(os.listdir(GOLDEN)):
        if n.endswith(".flac"):
            x, sr, ch = glc_amd.load_flac(os.path.join(GOLDEN, n))
            yield n, x, sr, ch
    yield "tone+noise", np.concatenate([gen_tone("sine", 440.0, 44100, 2, 0.3) * F32(1.2), gen_noise(44100, 2, 0.1, 4)]), 44100, 2


def test_i16_writers_equal_the_float_writers(tmp_path):
    for name, x, sr, ch in _flac_inputs():
        x = x[:x.size // ch * ch]
        q = narrow(x)
        for level in (0, 5, 8):
            a = glc_amd.encode_flac_with_level(q, sr, ch, level)
            assert a == glc_amd.encode_flac_with_level(x, sr, ch, level), (name, level)
            assert a == FO.encode_flac_with_level(x, sr, ch, level), (name, level)
        glc_amd.export_to_flac(tmp_path / "a.flac", q, sr, ch)
        glc_amd.export_to_flac(tmp_path / "b.flac", x, sr, ch)
        assert (tmp_path / "a.flac").read_bytes() == (tmp_path / "b.flac").read_bytes() == glc_amd.encode_flac(x, sr, ch)
        glc_amd.export_to_wav(tmp_path / "a.wav", q, sr, ch)
        glc_amd.export_to_wav(tmp_path / "b.wav", x, sr, ch)
        wa = (tmp_path / "a.wav").read_bytes()
        assert wa == (tmp_path / "b.wav").read_bytes() and wa[44:] == q.tobytes() and len(wa) == 44 + 2 * q.size, name
        # the file read back: the integers again, no float in between
        back, bbits, bsr, bch = glc_amd.load_audio_file_pcm(tmp_path / "a.wav")
        assert back.dtype == np.int16 and bbits == 16 and (bsr, bch) == (sr, ch) and np.array_equal(back, q)
        back = glc_amd.load_audio_file_pcm(tmp_path / "a.flac")[0]
        assert back.dtype == np.int16 and np.array_equal(back, q)


# ----------------------------------------------------------------------------------------------------
# CPU 3: argument checks that need no device
# ----------------------------------------------------------------------------------------------------

def test_binding_argument_checks_without_a_device(tmp_path):
    enc = glc_amd.Encoder.__new__(glc_amd.Encoder)      # no context: a check that reached the library would fail differently
    enc._h = None
    for bad in (np.zeros(4096, np.float64), np.zeros(4096, np.int64), np.zeros(4096, np.uint8), np.zeros(4096, np.uint16),
                np.zeros(4096, np.float16), np.zeros(4096, bool)):
        with pytest.raises(TypeError):
            enc.encode(bad, 1)
    for arr, b in [(np.zeros(4096, np.int16), 0), (np.zeros(4096, np.int16), 17), (np.zeros(4096, np.int32), 33),
                   (np.zeros(4096, np.int32), -1)]:
        with pytest.raises(glc_amd.GlcError) as e:
            enc.encode(arr, 1, bits=b)
        assert e.value.code == EINVAL
    with pytest.raises(TypeError):
        enc.encode(np.zeros(4096, F32), 1, bits=16)
    dec = glc_amd.Decoder.__new__(glc_amd.Decoder)
    dec._h = None
    with pytest.raises(TypeError):
        dec.decode(None, dtype=np.int32)
    with pytest.raises(TypeError):
        next(dec.decode_streaming(None, dtype=np.float64))
    # the C ABI: null contexts / pointers, unknown formats
    out = C.c_void_p()
    n = C.c_uint64()
    last = C.c_int()
    buf = np.zeros(4096, np.int16)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.glc_encode_int(None, p, S16, 16, buf.size, 1, C.byref(out)) == EINVAL
    assert lib.glc_decode_i16(None, None, p, buf.size, C.byref(n)) == EINVAL
    assert lib.glc_decode_range_device_i16(None, None, 0, 1, p, buf.size) == EINVAL
    assert lib.glc_decode_stream_next_i16(None, p, buf.size, C.byref(n), C.byref(last)) == EINVAL
    assert lib.glc_pcm_widen_device(None, p, S16, 16, 4, p) == EINVAL
    assert lib.glc_wav_save16_i16(None, p, 4, 44100, 1) == EINVAL
    assert lib.glc_wav_save16_i16(str(tmp_path / "x.wav").encode(), None, 4, 44100, 1) == EINVAL
    assert lib.glc_wav_save16_i16(str(tmp_path / "x.wav").encode(), p, 4, 44100, 0) == EINVAL
    assert lib.glc_flac_save_i16(None, p, 64, 44100, 1, 5) == EINVAL
    assert lib.glc_flac_save_i16(str(tmp_path / "x.flac").encode(), None, 64, 44100, 1, 5) == EINVAL
    ptr = C.c_void_p()
    assert lib.glc_flac_encode_i16(None, 64, 44100, 1, 5, C.byref(ptr), C.byref(n)) == EINVAL
    assert lib.glc_flac_encode_i16(p, 64, 44100, 1, 5, None, C.byref(n)) == EINVAL
    for count, ch, level in [(15, 1, 5), (64, 0, 5), (64, 1, 9), (0, 1, 5)]:     # the float writer's own refusals
        assert lib.glc_flac_encode_i16(p, count, 44100, ch, level, C.byref(ptr), C.byref(n)) == EINVAL
        assert lib.glc_flac_encode(np.zeros(64, F32).ctypes.data_as(C.c_void_p), count, 44100, ch, level, C.byref(ptr), C.byref(n)) == EINVAL
    assert not os.path.exists(tmp_path / "x.wav") and not os.path.exists(tmp_path / "x.flac")
    # zero samples: the header-only file of the float writer
    glc_amd.export_to_wav(tmp_path / "z16.wav", np.zeros(0, np.int16), 8000, 1)
    glc_amd.export_to_wav(tmp_path / "zf.wav", np.zeros(0, F32), 8000, 1)
    assert (tmp_path / "z16.wav").read_bytes() == (tmp_path / "zf.wav").read_bytes() and os.path.getsize(tmp_path / "z16.wav") == 44
    got, gbits, sr, ch = glc_amd.load_audio_file_pcm(tmp_path / "z16.wav")
    assert got.size == 0 and got.dtype == np.int16 and (gbits, sr, ch) == (16, 8000, 1)
    # glc_audio_load_pcm: nulls, extensions (src/audio.rs:21-35), a missing file
    fmt = C.c_int()
    b = C.c_uint32()
    sr_ = C.c_uint32()
    ch_ = C.c_uint16()
    full = [C.byref(ptr), C.byref(fmt), C.byref(b), C.byref(n), C.byref(sr_), C.byref(ch_)]
    assert lib.glc_audio_load_pcm(None, *full) == EINVAL
    for k in range(6):
        args = list(full)
        args[k] = None
        assert lib.glc_audio_load_pcm(str(tmp_path / "z16.wav").encode(), *args) == EINVAL
    for name, msg in [("noext", "No file extension"), ("a.mp3", "Unsupported file format: mp3"), ("dir.wav/noext", "No file extension")]:
        with pytest.raises(glc_amd.GlcError, match=msg) as e:
            glc_amd.load_audio_file_pcm(tmp_path / name)
        assert e.value.code == EINVAL
    for name in ("missing.wav", "missing.flac"):
        with pytest.raises(glc_amd.GlcError) as e:
            glc_amd.load_audio_file_pcm(tmp_path / name)
        assert e.value.code == EIO


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    return torch


PAD = 64          # sentinel elements in front of and behind every destination (a multiple of 8: keeps the 16-byte phase)
I16_SENTINEL = -21846   # 0xAAAA


def _widen_on_device(torch, enc, src, bits, src_off=0, dst_off=0):
    """src (int16 / int32 numpy) -> floats through glc_pcm_widen_device; the source starts src_off elements and
    the destination dst_off elements past a 16-byte boundary; sentinels around the destination are checked."""
    n = src.size
    tdt = torch.int16 if src.dtype == np.int16 else torch.int32
    d_src = torch.zeros(n + 8, dtype=tdt, device="cuda")
    d_dst = torch.full((PAD + dst_off + n + PAD,), D.SENTINEL_BITS, dtype=torch.int32, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    if n:
        d_src[src_off:src_off + n] = torch.from_numpy(src)
    torch.cuda.synchronize()
    at = PAD + dst_off
    enc.widen_device(d_src.data_ptr() + src_off * src.dtype.itemsize, src.dtype, bits, n, d_dst.data_ptr() + 4 * at)
    enc.synchronize()
    out = d_dst.cpu().numpy().view(np.uint32)
    assert (out[:at] == D.SENTINEL_BITS).all() and (out[at + n:] == D.SENTINEL_BITS).all(), \
        f"floats around the destination were written (n {n}, offsets {src_off}/{dst_off})"
    return out[at:at + n]


def _assert_widened(got, src, bits, what):
    exp = bits_of(widen(src, bits))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (f"{what}: {bad.size} of {exp.size} differ, first at {bad[0]}: sample {int(src[bad[0]])} got "
                           f"{got[bad[0]]:#010x} want {exp[bad[0]]:#010x}")


def _int32_values(bits, rng, n):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    sp = [lo, lo + 1, lo + 2, hi, hi - 1, hi - 2, 0, 1, -1, 2, -2]
    for base in ((1 << 24), (1 << 25), (1 << 26), (1 << 30)):
        step = base >> 23                                   # spacing of f32 above `base`
        for k in (-2, -1, 0, 1, 2):
            sp += [base + k, -base + k, base + step // 2 + k, base + 3 * step // 2 + k, -(base + step // 2) + k,
                   -(base + 3 * step // 2) + k, base + step + k]
    sp += [(1 << 31) - 1, (1 << 31) - 64, (1 << 31) - 65, (1 << 31) - 127, (1 << 31) - 128, (1 << 31) - 129, -(1 << 31),
           -(1 << 31) + 1, -(1 << 31) + 127, -(1 << 31) + 128, -(1 << 31) + 129]
    sp = [v for v in sp if lo <= v <= hi]
    v = rng.integers(lo, hi + 1, n, dtype=np.int64)
    v[:len(sp)] = sp
    return v.astype(np.int32)


@pytest.mark.gpu
def test_gpu_widen_every_int16_value_and_int32_edges(gpu):
    enc = glc_amd.Encoder(48000)
    every = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    for bits in (16, 8, 12, 1):
        _assert_widened(_widen_on_device(gpu, enc, every, bits), every, bits, f"int16 bits {bits}")
    rng = np.random.default_rng(7)
    for bits in (8, 12, 16, 20, 24, 32):
        v = _int32_values(bits, rng, 5000)
        got = _widen_on_device(gpu, enc, v, bits)
        _assert_widened(got, v, bits, f"int32 bits {bits}")
    v = _int32_values(32, rng, 5000)
    w = widen(v, 32)
    assert w[0] == 1.0 and (w[np.flatnonzero(v == 0)].view(np.uint32) == 0x80000000).all()      # inverted, -0.0 (Q11)
    assert (np.abs(v.astype(np.int64)) > (1 << 24)).sum() > 2000 and \
        (v.astype(F32).astype(np.int64) != v).sum() > 2000                                      # `as f32` had to round


@pytest.mark.gpu
@pytest.mark.parametrize("dt,bits", [(np.int16, 16), (np.int32, 24), (np.int32, 32)])
def test_gpu_widen_lengths_and_alignments(gpu, dt, bits):
    enc = glc_amd.Encoder(44100)
    rng = np.random.default_rng(11)
    lo, hi = (-(1 << 15), (1 << 15) - 1) if dt == np.int16 else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    for n in (0, 1, 3, 255, 256, 257, 1048577):
        src = rng.integers(lo, hi + 1, n, dtype=np.int64).astype(dt)
        offs = [(a, b) for a in range(4) for b in range(4)] if n < 1000 else [(0, 0), (1, 0), (0, 3), (2, 2), (3, 1), (1, 2)]
        for so, do in offs:
            _assert_widened(_widen_on_device(gpu, enc, src, bits, so, do), src, bits, f"n {n} offsets {so}/{do}")
    # argument checks that need a context
    src = gpu.zeros(64, dtype=gpu.int32, device="cuda")
    for b in (0, 17 if dt == np.int16 else 33):
        with pytest.raises(glc_amd.GlcError) as e:
            enc.widen_device(src.data_ptr(), dt, b, 8, src.data_ptr())
        assert e.value.code == EINVAL
    assert lib.glc_pcm_widen_device(enc._h, C.c_void_p(src.data_ptr()), 7, 16, 8, C.c_void_p(src.data_ptr())) == EINVAL
    assert lib.glc_pcm_widen_device(enc._h, C.c_void_p(src.data_ptr() + 1), S16, 16, 8, C.c_void_p(src.data_ptr() + 64)) == EINVAL
    assert lib.glc_pcm_widen_device(enc._h, None, S16, 16, 8, C.c_void_p(src.data_ptr())) == EINVAL
    assert lib.glc_pcm_widen_device(enc._h, None, S16, 16, 0, None) == 0


def _encode_cases():
    from test_gpu_parity import CASES
    for name, make, sr, ch in CASES:
        yield name, make, sr, ch
    yield "chord_48k_16ch", lambda: gen_chord(48000, 16, 3000), 48000, 16
    yield "min_len_8ch", lambda: gen_chord(48000, 8, 513), 48000, 8
    yield "lcg_noise_44k_stereo", lambda: gen_noise(44100, 2, 0.4, 12345), 44100, 2
    yield "chord_then_noise_5ch", lambda: np.concatenate([gen_chord(44100, 5, 7000), gen_noise(44100, 5, 0.15, 9)]), 44100, 5


ENCODE_CASES = list(_encode_cases())
_seen = {"raw": 0, "compressed": 0, "channels": set(), "cases": set()}


def _encode_three_ways(enc, s, bits, sr, ch):
    w = widen(s, bits)
    ref = O.encode(w, sr, ch)
    a = enc.encode(s, ch, bits=bits)
    assert a.to_bytes() == enc.encode(w, ch).to_bytes(), "glc_encode_int differs from glc_encode of the widened samples"
    assert a.to_bytes() == ref.glc, "glc_encode_int differs from the oracle"
    info = a.info()
    _seen["raw"] += info.n_raw_frames
    _seen["compressed"] += info.n_frames - info.n_raw_frames
    _seen["channels"].add(ch)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,sr,ch", ENCODE_CASES, ids=[c[0] for c in ENCODE_CASES])
def test_gpu_encode_int_equals_float_encode_and_oracle(gpu, name, make, sr, ch):
    s = quantise16(make())
    enc = glc_amd.Encoder(sr)
    _encode_three_ways(enc, s, 16, sr, ch)
    _seen["cases"].add(name)
    odd = np.empty(s.size + 1, np.int16)         # the same samples at an odd element offset on the host
    odd[1:] = s
    assert odd[1:].ctypes.data % 4 == 2
    assert enc.encode(odd[1:], ch).to_bytes() == enc.encode(s, ch).to_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [24, 32, 20])
def test_gpu_encode_int_s32(gpu, bits):
    sr, ch = 48000, 2
    x = np.concatenate([gen_chord(sr, ch, 9000, amp=0.04), gen_noise(sr, ch, 0.1, 3)]).astype(np.float64)
    s = np.clip(np.rint(x * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int32)
    if bits == 32:                                               # low bits a float32 signal never had: `as f32` must round
        s ^= np.random.default_rng(5).integers(0, 256, s.size, dtype=np.int32)
        assert (s.astype(F32).astype(np.int64) != s).sum() > s.size // 2
    a = _encode_three_ways(glc_amd.Encoder(sr), s, bits, sr, ch)
    assert 0 < a.info().n_raw_frames < a.info().n_frames
    with pytest.raises(glc_amd.GlcError) as e:                   # 16-bit samples cannot hold 24 bits
        glc_amd.Encoder(sr).encode(s.astype(np.int16), ch, bits=24)
    assert e.value.code == EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("ch,frames", [(2, 4096 + 1024 + 300), (1, 8192 + 700)])
def test_gpu_encode_int_more_than_one_round(gpu, ch, frames):
    """Opening rounds, then rounds of 4096 (8192 mono) frames: every round's upload increment and its halo."""
    sr = 48000
    per = frames * 1024 + 77
    x = gen_chord(sr, ch, per, n_tones=6, amp=0.1)
    x[per // 3 * ch:(per // 3 + 30000) * ch] = gen_noise(sr, ch, 30000 / sr + 0.01, 21)[:30000 * ch] * F32(0.5)
    s = quantise16(x)
    a = _encode_three_ways(glc_amd.Encoder(sr), s, 16, sr, ch)
    assert a.info().n_frames >= frames and 0 < a.info().n_raw_frames < a.info().n_frames


@pytest.mark.gpu
def test_gpu_encode_int_covered_both_frame_kinds_and_argument_checks(gpu):
    """Over the encode cases (those of this session, the rest encoded here): both kinds of frame and the
    channel counts were produced."""
    for name, make, sr, ch in ENCODE_CASES:
        if name not in _seen["cases"]:
            _encode_three_ways(glc_amd.Encoder(sr), quantise16(make()), 16, sr, ch)
            _seen["cases"].add(name)
    assert _seen["raw"] > 0 and _seen["compressed"] > 0, _seen
    assert {1, 2, 3, 5, 8, 16} <= _seen["channels"], _seen
    enc = glc_amd.Encoder(44100)
    s = np.zeros(4096, np.int16)
    out = C.c_void_p()
    p = s.ctypes.data_as(C.c_void_p)
    for fmt, b, n, ch in [(S16, 0, 4096, 1), (S16, 17, 4096, 1), (S32, 33, 2048, 1), (0, 16, 4096, 1), (4, 16, 4096, 1),
                          (S16, 16, 512, 1), (S16, 16, 4096, 0), (S16, 16, 1024, 2), (S16, 16, 0, 1)]:
        assert lib.glc_encode_int(enc._h, p, fmt, b, n, ch, C.byref(out)) == EINVAL, (fmt, b, n, ch)
        assert not out.value
    assert lib.glc_encode_int(enc._h, None, S16, 16, 4096, 1, C.byref(out)) == EINVAL
    assert lib.glc_encode_int(enc._h, p, S16, 16, 4096, 1, None) == EINVAL
    f = np.zeros(4096, F32)                                       # GLC_PCM_F32 forwards to glc_encode
    assert lib.glc_encode_int(enc._h, f.ctypes.data_as(C.c_void_p), PF32, 0, 4096, 1, C.byref(out)) == 0
    assert glc_amd.EncodedAudio(out.value).to_bytes() == enc.encode(f, 1).to_bytes()


# ---- decode ----------------------------------------------------------------------------------------

def _decode_streams():
    for n in sorted(os.listdir(GOLDEN)):
        if n.endswith(".glc"):
            yield n, open(os.path.join(GOLDEN, n), "rb").read()
    by = {c.name: c for c in D.cases()}
    for name in ["values", "raw-ch2", "overlap-long"] + [f"overlap-ch{c}" for c in D.OVERLAP_CHANNELS]:
        yield name, by[name].stream.to_glc()


DECODE_STREAMS = None


def decode_streams():
    global DECODE_STREAMS
    if DECODE_STREAMS is None:
        DECODE_STREAMS = list(_decode_streams())
    return DECODE_STREAMS


def _coverage(floats):
    """What the expected int16 data must contain, judged from float decodes."""
    x = np.concatenate(floats)
    q = narrow(x)
    with np.errstate(all="ignore"):
        v = x * F32(32767.0)
    fin = np.isfinite(v) & (np.abs(v) < 32767)
    return dict(lowest=bool((q == -32768).any()), highest=bool((q == 32767).any()),
                nan_to_zero=bool(np.isnan(x).any() and (q[np.isnan(x)] == 0).all()),
                inf=bool(np.isinf(x).any()), beyond_one=bool((np.abs(x[np.isfinite(x)]) > 1).any()),
                trunc_is_not_round=bool((np.rint(v[fin]) != np.trunc(v[fin])).any()))


def test_decode_streams_cover_the_narrowing_on_the_oracle():
    """CPU: the oracle's decode of the streams the GPU tests use holds every case of the narrowing."""
    cov = _coverage([O.decode(glc)[0] for _, glc in decode_streams()])
    assert all(cov.values()), cov
    chans = {struct.unpack_from("<H", glc, 4)[0] for _, glc in decode_streams()}
    assert {1, 2, 3, 4, 5, 8, 9} <= chans                       # every specialisation of the kernel and the generic one
    frames = [struct.unpack_from("<Q", glc, 14)[0] for _, glc in decode_streams()]
    assert max(frames) > 4096 and sum(f > 500 for f in frames) >= 1


@pytest.mark.gpu
def test_gpu_decode_i16_equals_the_narrowed_float_decode(gpu):
    floats = []
    for name, glc in decode_streams():
        ref = O.decode(glc)[0]                                   # CPU first
        floats.append(ref)
    assert all(_coverage(floats).values())
    for (name, glc), ref in zip(decode_streams(), floats):
        ea = glc_amd.EncodedAudio.from_bytes(glc)
        dec = glc_amd.Decoder(ea.header.channels, ea.header.sample_rate)
        f = dec.decode(ea)
        assert np.array_equal(bits_of(f), bits_of(ref)), name
        out = np.full(f.size + 64, I16_SENTINEL, np.int16)
        got = dec.decode(ea, out=out, dtype=np.int16)
        assert got.dtype == np.int16 and got.size == f.size, name
        exp = narrow(f)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: float {f[bad[0]]!r} got {got[bad[0]]} want {exp[bad[0]]}"
        assert (out[f.size:] == I16_SENTINEL).all(), name
        # through the streaming rule of the reference (decode with a progress sender), and a fresh context
        again = glc_amd.Decoder(ea.header.channels, ea.header.sample_rate).decode(ea, progress_sender=lambda k, v: None, dtype=np.int16)
        assert np.array_equal(again, exp), name
        with pytest.raises(glc_amd.GlcError) as e:               # buffer too small / wrong dtype
            dec.decode(ea, out=np.zeros(max(f.size - 1, 0), np.int16), dtype=np.int16)
        assert e.value.code == EINVAL
        with pytest.raises(glc_amd.GlcError):
            dec.decode(ea, out=np.zeros(f.size, F32), dtype=np.int16)


@pytest.mark.gpu
def test_gpu_decode_streaming_i16_chunk_by_chunk(gpu):
    seen_chunks = 0
    for name, glc in decode_streams():
        ea = glc_amd.EncodedAudio.from_bytes(glc)
        ch, sr = ea.header.channels, ea.header.sample_rate
        fl = list(glc_amd.Decoder(ch, sr).decode_streaming(ea))
        dec = glc_amd.Decoder(ch, sr)
        it = list(dec.decode_streaming(ea, dtype=np.int16))
        assert len(it) == len(fl) == -(-ea.info().n_frames // 500) + (1 if ea.info().n_frames % 500 == 0 else 0), name
        for k, (a, b) in enumerate(zip(it, fl)):
            assert a.is_last == b.is_last and a.samples.dtype == np.int16, (name, k)
            assert np.array_equal(a.samples, narrow(b.samples)), (name, k)
        seen_chunks = max(seen_chunks, len(it))
        # the same context decodes floats afterwards, and int16 again
        assert np.array_equal(np.concatenate([c.samples for c in dec.decode_streaming(ea, dtype=np.int16)]),
                              np.concatenate([c.samples for c in it])), name
        assert np.array_equal(bits_of(np.concatenate([c.samples for c in dec.decode_streaming(ea)])),
                              bits_of(np.concatenate([c.samples for c in fl]))), name
    assert seen_chunks > 8                                       # a stream of several chunks was among them


@pytest.mark.gpu
def test_gpu_decode_stream_formats_do_not_mix(gpu):
    glc = dict(decode_streams())["overlap-long"]
    ea = glc_amd.EncodedAudio.from_bytes(glc)
    dec = glc_amd.Decoder(1, 48000)
    cap = 500 * 1024
    f = np.zeros(cap, F32)
    q = np.zeros(cap, np.int16)
    n = C.c_uint64()
    last = C.c_int()
    fp, qp = f.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)
    assert lib.glc_decode_stream_next_i16(dec._h, qp, cap, C.byref(n), C.byref(last)) == EINVAL       # nothing open
    ref = list(glc_amd.Decoder(1, 48000).decode_streaming(ea))
    assert lib.glc_decode_stream_begin(dec._h, ea._h) == 0
    assert lib.glc_decode_stream_next_i16(dec._h, qp, cap, C.byref(n), C.byref(last)) == 0
    assert np.array_equal(q[:n.value], narrow(ref[0].samples))
    assert lib.glc_decode_stream_next(dec._h, fp, cap, C.byref(n), C.byref(last)) == EINVAL           # float on an int16 stream
    assert lib.glc_decode_stream_next_i16(dec._h, qp, cap, C.byref(n), C.byref(last)) == 0            # ... which goes on undisturbed
    assert np.array_equal(q[:n.value], narrow(ref[1].samples))
    assert lib.glc_decode_stream_begin(dec._h, ea._h) == 0
    assert lib.glc_decode_stream_next(dec._h, fp, cap, C.byref(n), C.byref(last)) == 0
    assert np.array_equal(bits_of(f[:n.value]), bits_of(ref[0].samples))
    assert lib.glc_decode_stream_next_i16(dec._h, qp, cap, C.byref(n), C.byref(last)) == EINVAL       # int16 on a float stream
    assert lib.glc_decode_stream_next(dec._h, fp, cap, C.byref(n), C.byref(last)) == 0
    assert np.array_equal(bits_of(f[:n.value]), bits_of(ref[1].samples))


def _range_i16(torch, dec, ea, h0, h1, ch, off2):
    """decode_range_device_i16 of hops [h0, h1) to a destination off2 int16 elements past a 16-byte boundary."""
    n = (h1 - h0) * 1024 * ch
    d = torch.full((PAD + off2 + n + PAD,), I16_SENTINEL, dtype=torch.int16, device="cuda")
    assert d.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    at = PAD + off2
    dec.decode_range_device_i16(ea, h0, h1, d.data_ptr() + 2 * at, n)
    dec.synchronize()
    out = d.cpu().numpy()
    assert (out[:at] == I16_SENTINEL).all() and (out[at + n:] == I16_SENTINEL).all(), \
        f"samples around the destination were written (hops [{h0}, {h1}), offset {off2})"
    return out[at:at + n]


def _range_f32(torch, dec, ea, h0, h1, ch):
    n = (h1 - h0) * 1024 * ch
    d = torch.zeros(max(n, 1), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_range_device(ea, h0, h1, d.data_ptr(), n)
    dec.synchronize()
    return d.cpu().numpy()[:n]


@pytest.mark.gpu
def test_gpu_decode_range_device_i16(gpu):
    for name, glc in decode_streams():
        ea = glc_amd.EncodedAudio.from_bytes(glc)
        ch, nf = ea.header.channels, ea.info().n_frames
        dec = glc_amd.Decoder(ch, ea.header.sample_rate)
        whole = _range_f32(gpu, dec, ea, 0, nf + 1, ch)
        if not name.endswith(".glc"):
            st = {c.name: c for c in D.cases()}[name].stream
            assert np.array_equal(bits_of(whole), bits_of(D.expected_hops(st, 0, nf + 1))), name
        exp = narrow(whole).reshape(nf + 1, 1024 * ch)
        if nf > 4096:
            ranges = [(0, nf + 1, 0), (4095, 4098, 3), (1, 4097, 5), (nf, nf + 1, 1)]
        else:
            ranges = [(0, nf + 1, o) for o in range(8)] + [(0, 1, 1), (nf, nf + 1, 2), (nf - 1, nf + 1, 7), (1, min(3, nf), 6),
                                                           (2, 2, 0)]
        for h0, h1, off in ranges:
            got = _range_i16(gpu, dec, ea, h0, h1, ch, off)
            want = exp[h0:h1].reshape(-1)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{name} hops [{h0}, {h1}) offset {off}: {bad.size} differ, first at {bad[0]}"
        d = gpu.zeros(1024 * ch * 2 + 8, dtype=gpu.int16, device="cuda")
        for a, b, ptr, cap in [(0, nf + 2, d.data_ptr(), 1 << 40), (2, 1, d.data_ptr(), 1 << 40), (0, 1, 0, 1 << 40),
                               (0, 1, d.data_ptr(), 1024 * ch - 1), (0, 1, d.data_ptr() + 1, 1024 * ch)]:
            with pytest.raises(glc_amd.GlcError) as e:
                dec.decode_range_device_i16(ea, a, b, ptr, cap)
            assert e.value.code == EINVAL, (name, a, b)


# ---- CLI ---------------------------------------------------------------------------------------------

def _cli_inputs(tmp_path):
    sr, ch = 44100, 2
    x = np.concatenate([gen_tone("sine", 440.0, sr, ch, 0.5), gen_noise(sr, ch, 0.1, 5), gen_chord(sr, ch, 6000, amp=0.4)])
    s16 = quantise16(x)
    _write_wav(tmp_path / "a16.wav", 1, 16, ch, sr, s16.tobytes())
    s24 = np.clip(np.rint(x.astype(np.float64) * (1 << 23)), -(1 << 23), (1 << 23) - 1).astype(np.int32)
    _write_wav(tmp_path / "b24.wav", 1, 24, ch, sr, b"".join(int(v).to_bytes(3, "little", signed=True) for v in s24))
    (tmp_path / "c.flac").write_bytes(glc_amd.encode_flac(x, sr, ch))
    return ["a16.wav", "b24.wav", "c.flac"]


@pytest.mark.gpu
def test_gpu_cli_files_equal_the_float_path(gpu, tmp_path):
    assert os.path.exists(CLI), "build/glc missing: run __graft_entry__.build()"
    for name in _cli_inputs(tmp_path):
        src = tmp_path / name
        x, sr, ch = glc_amd.load_audio_file_lossless(src)        # the float loader: what the reference encodes
        ref = O.encode(x, sr, ch)
        r = subprocess.run([CLI, str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"Encoding: {sr} Hz, {ch} channels, {x.size} samples" in r.stdout
        stem = os.path.splitext(name)[0]
        glc = tmp_path / (stem + ".glc")
        assert glc.read_bytes() == ref.glc, name
        os.remove(src)
        ea = glc_amd.load_encoded(glc)
        f = glc_amd.Decoder(ch, sr).decode(ea)                   # glc_decode + the float writers
        assert np.array_equal(bits_of(f), bits_of(O.decode(ref.glc)[0]))
        r = subprocess.run([CLI, "-d", str(glc)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"Decoded {f.size} samples" in r.stdout, r.stderr
        glc_amd.export_to_flac(tmp_path / "want.flac", f, sr, ch)
        assert (tmp_path / (stem + ".flac")).read_bytes() == (tmp_path / "want.flac").read_bytes(), name
        r = subprocess.run([CLI, "-d", "--flac-level", "8", str(glc)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / (stem + ".flac")).read_bytes() == glc_amd.encode_flac_with_level(f, sr, ch, 8), name
        r = subprocess.run([CLI, "-d", "--wav", str(glc)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        glc_amd.export_to_wav(tmp_path / "want.wav", f, sr, ch)
        got = (tmp_path / (stem + ".wav")).read_bytes()
        assert got == (tmp_path / "want.wav").read_bytes() and got[44:] == narrow(f).tobytes(), name
