"""The streaming decode: glc_stream_dec_push_device (segments in a device arena, many lanes per launch chain) and
glc_stream_dec_push (host blobs).

The contract is bit equality and nothing else: the concatenation of a lane's outputs over ANY chunking equals glc_decode
of glc_frames_from_compact of the same segments, and the oracle's decode of the oracle's encode.  Segments of chosen
frame ranges are made with glc_encode_range_device + glc_compact_device_records (what the stream encoder stores, byte
for byte - tests/test_stream_encode.py holds it to that), once per (signal, range), and shared; references are computed
once per signal (`want`).  Output layouts have odd strides and a sentinel in every element no lane owns."""
import ctypes as C
import gc
import hashlib
import os
import subprocess

import numpy as np
import pytest

import stream_decode_cases as DC
from conftest import O, ROOT, gen_chord, gen_noise, gen_tone

pytestmark = pytest.mark.gpu

F32 = np.float32
HOP, SR = DC.HOP, DC.SR
S16, PF32 = DC.S16, DC.PF32
EINVAL = -1
NAN_BITS = np.uint32(0x7FC12345)          # the float sentinel: a NaN with a payload of its own
I16_SENTINEL = np.int16(-12345)


def chord(ch, L, seed):
    return gen_chord(SR, ch, L, seed=seed)


def noise(ch, L, seed):
    return gen_noise(SR, ch, L / SR + 0.01, seed)[:L * ch].copy()


def tone(ch, L, f=440.0):
    return gen_tone("sine", f, SR, ch, L / SR + 0.01)[:L * ch].copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


class Env:
    def __init__(self):
        import torch
        import glc_amd
        assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
        self.torch, self.g, self.lib, self.L = torch, glc_amd, glc_amd.lib, glc_amd._lib
        self.ctx = glc_amd.Encoder(SR)         # the context the sessions live on
        self.enc = glc_amd.Encoder(SR)         # makes the segments
        self.ref = glc_amd.Decoder(2, SR)      # the yardstick's context: glc_decode
        self.blobs, self.wants = {}, {}

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    @staticmethod
    def key(x, ch):
        return hashlib.sha1(np.ascontiguousarray(x, F32).tobytes()).digest(), ch

    def range_blob(self, x, ch, f0, n):
        """glc_encode_range_device + glc_compact_device_records of frames [f0, f0 + n) of the whole float stream."""
        k = self.key(x, ch) + (f0, n)
        if k not in self.blobs:
            torch = self.torch
            L = x.size // ch
            d = self.dev(np.ascontiguousarray(x, F32))
            rec = torch.empty(n * int(self.lib.glc_record_bytes(ch)), dtype=torch.uint8, device="cuda")
            blob = torch.zeros(self.g.compact_bound(ch, n), dtype=torch.uint8, device="cuda")
            self.enc.encode_range_device(d.data_ptr(), 0, L, L * ch, ch, f0, f0 + n, rec.data_ptr())
            info = self.enc.compact_device_records(rec.data_ptr(), n, ch, blob.data_ptr(), blob.numel())
            self.blobs[k] = blob[:info.bytes].cpu().numpy().tobytes()
        return self.blobs[k]

    def decode_blobs(self, blobs, n_samples, ch, dtype=F32):
        return self.ref.decode(self.g.EncodedAudio.from_compact(SR, n_samples, ch, blobs), dtype=dtype).copy()

    def want(self, x, ch):
        """(float32, int16) samples of glc_decode of the stream's segments, the floats held to the oracle; once."""
        k = self.key(x, ch)
        if k not in self.wants:
            nf = DC.num_frames(x.size // ch)
            whole = [self.range_blob(x, ch, 0, nf)]
            f = self.decode_blobs(whole, x.size, ch)
            oracle, _, _ = O.decode(O.encode(np.ascontiguousarray(x, F32), SR, ch).glc)
            assert f.size == x.size and np.array_equal(bits(f), bits(np.asarray(oracle, F32))), "glc_decode differs from the oracle"
            self.wants[k] = (f, self.decode_blobs(whole, x.size, ch, np.int16))
        return self.wants[k]


@pytest.fixture(scope="module")
def E():
    e = Env()
    yield e
    e.blobs.clear()
    e.wants.clear()
    e.ctx = e.enc = e.ref = None


class OutLayout:
    """A flat output buffer in which lane i's `lens[i]` samples per channel lie as a glc_clip_layout says: one element
    in front, odd strides, a sentinel in every element."""

    def __init__(self, ch, lens, planar, fmt):
        self.ch, self.lens, self.planar, self.fmt = ch, [int(v) for v in lens], planar, fmt
        longest = max(self.lens + [1])
        self.planes = planar and ch > 1
        if self.planes:
            self.channel_stride = longest + 3
            self.clip_stride = self.channel_stride * ch + 5
        else:
            self.channel_stride = 0
            self.clip_stride = longest * ch + 3
        if self.clip_stride % 2 == 0:
            self.clip_stride += 1
        self.off = 1
        self.size = self.off + self.clip_stride * len(self.lens) + 5
        if fmt == PF32:
            self.flat = np.full(self.size, NAN_BITS, np.uint32).view(F32)
        else:
            self.flat = np.full(self.size, I16_SENTINEL, np.int16)

    def owned(self):
        m = np.zeros(self.size, bool)
        for i, n in enumerate(self.lens):
            base = self.off + i * self.clip_stride
            if self.planes:
                for c in range(self.ch):
                    m[base + c * self.channel_stride: base + c * self.channel_stride + n] = True
            else:
                m[base: base + n * self.ch] = True
        return m

    def lane(self, got, i):
        """Lane i's samples of `got` (the buffer after the push), interleaved."""
        n, base = self.lens[i], self.off + i * self.clip_stride
        if self.planes:
            return np.stack([got[base + c * self.channel_stride: base + c * self.channel_stride + n] for c in range(self.ch)], 1).reshape(-1)
        return got[base: base + n * self.ch].copy()


def make_store(E, blobs, stored=None, gap=64):
    """An arena holding `blobs` at multiples of 64 with `gap` bytes of a pattern between them, and the (n, 4) entry words."""
    at, offs = 64, []
    for b in blobs:
        offs.append(at)
        at += (len(b) + 63) // 64 * 64 + gap
    image = ((np.arange(at, dtype=np.uint64) * np.uint64(131)) % np.uint64(251)).astype(np.uint8)
    ent = np.zeros((max(len(blobs), 1), 4), np.int64)
    for j, b in enumerate(blobs):
        image[offs[j]: offs[j] + len(b)] = np.frombuffer(b, np.uint8)
        ent[j] = [offs[j], len(b), 0, (1 if stored is None or stored[j] else 0) << 32]
    return E.dev(image), E.dev(ent[:len(blobs)] if blobs else ent)


class Session:
    """glc_stream_dec_* through ctypes, on a context of the caller's."""

    def __init__(self, E, ch, n, ctx=None):
        self.E, self.ch, self.n, self.ctx = E, ch, n, ctx or E.ctx
        s = C.c_void_p()
        assert E.lib.glc_stream_dec_open(self.ctx._h, ch, n, C.byref(s)) == 0, self.err()
        self.s = s
        self.done = [0] * n

    def err(self):
        return self.E.lib.glc_last_error(self.ctx._h)

    def close(self):
        if self.s:
            self.E.lib.glc_stream_dec_close(self.s)
        self.s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def frames_done(self, i):
        n = C.c_uint64(99)
        assert self.E.lib.glc_stream_dec_frames_done(self.s, i, C.byref(n)) == 0
        return n.value

    def plan(self, segs, finish, total):
        """Per lane the samples per channel the model says the push emits."""
        frames = [0] * self.n
        for (lane, _, nf) in segs:
            if lane < self.n:
                frames[lane] += nf
        lens = []
        for i in range(self.n):
            fin = bool(finish and finish[i])
            p = DC.model_plan(self.done[i], frames[i], fin, total[i] if fin else 0) if frames[i] or fin else (0, 0)
            lens.append(p[1] if p else 0)          # (None: a push the library must refuse)
        return frames, lens

    def raw(self, arena, entries, segs, finish, total, lay, d_out, arena_bytes=None, fmt=None, n_segs=None, n_clips=None, lay_ch=None,
            lens=None, null_total=False, arena_ptr=None, entries_ptr=None, out_ptr=None, null_lay=False):
        """One glc_stream_dec_push_device; every argument can be bent for the refusals."""
        Lc = self.E.L
        arr = (C.c_uint64 * self.n)(*(lay.lens if lens is None else lens))
        cl = Lc.GlcClipLayout(self.n if n_clips is None else n_clips, lay_ch or self.ch, 1 if lay.planar else 0, lay.clip_stride,
                              lay.channel_stride, 0, C.cast(arr, C.POINTER(C.c_uint64)))
        c_segs = (Lc.GlcStreamSeg * max(len(segs), 1))(*[Lc.GlcStreamSeg(a, b, c) for (a, b, c) in segs])
        fin = None if finish is None else (C.c_uint8 * self.n)(*[1 if f else 0 for f in finish])
        tot = None if null_total or total is None else (C.c_uint64 * self.n)(*total)
        ap = arena.data_ptr() if arena_ptr is None else arena_ptr
        ep = (entries.data_ptr() if entries is not None else 0) if entries_ptr is None else entries_ptr
        op = d_out.data_ptr() + lay.off * d_out.element_size() if out_ptr is None else out_ptr
        return self.E.lib.glc_stream_dec_push_device(self.s, C.c_void_p(ap), arena.numel() if arena_bytes is None else arena_bytes,
                                                     C.c_void_p(ep), c_segs, len(segs) if n_segs is None else n_segs, fin, tot,
                                                     C.c_void_p(op), lay.fmt if fmt is None else fmt, None if null_lay else C.byref(cl))

    def push_store(self, arena, entries, segs, finish, total, planar=False, fmt=PF32):
        """A push of segs [(lane, first_frame, n_frames)] whose entries are on the device -> per lane its samples.  Checks
        that no element outside the lanes' spans was written and that frames_done follows."""
        frames, lens = self.plan(segs, finish, total)
        lay = OutLayout(self.ch, lens, planar, fmt)
        d_out = self.E.dev(lay.flat)
        rc = self.raw(arena, entries, segs, finish, total, lay, d_out)
        assert rc == 0, self.err()
        self.ctx.synchronize()
        assert self.E.lib.glc_ctx_resident_stream(self.ctx._h) == 0
        got = d_out.cpu().numpy()
        keep = ~lay.owned()
        assert np.array_equal(bits(got)[keep], bits(lay.flat)[keep]), "an element outside the lanes' spans was written"
        for i in range(self.n):
            self.done[i] = 0 if finish and finish[i] else self.done[i] + frames[i]
            assert self.frames_done(i) == self.done[i]
        return [lay.lane(got, i) for i in range(self.n)]

    def push(self, blob_segs, finish, total, planar=False, fmt=PF32, stored=None):
        """blob_segs: [(lane, first_frame, n_frames, blob bytes)] -> per lane its samples."""
        arena, entries = make_store(self.E, [b for (_, _, _, b) in blob_segs], stored)
        return self.push_store(arena, entries, [(a, b, c) for (a, b, c, _) in blob_segs], finish, total, planar, fmt)

    def push_host(self, blob_segs, finish, total, fmt=PF32):
        Lc = self.E.L
        n = len(blob_segs)
        frames, lens = self.plan([(a, b, c) for (a, b, c, _) in blob_segs], finish, total)
        keep = [np.frombuffer(b, np.uint8).copy() for (_, _, _, b) in blob_segs]
        ptrs = (C.c_void_p * max(n, 1))(*[k.ctypes.data for k in keep])
        sizes = (C.c_uint64 * max(n, 1))(*[k.size for k in keep])
        c_segs = (Lc.GlcStreamSeg * max(n, 1))(*[Lc.GlcStreamSeg(a, b, c) for (a, b, c, _) in blob_segs])
        fin = (C.c_uint8 * self.n)(*[1 if f else 0 for f in (finish or [0] * self.n)])
        tot = (C.c_uint64 * self.n)(*total)
        outs = [np.full(v * self.ch + 2, 7, F32 if fmt == PF32 else np.int16) for v in lens]
        optrs = (C.c_void_p * self.n)(*[o.ctypes.data for o in outs])
        n_out = (C.c_uint64 * self.n)()
        rc = self.E.lib.glc_stream_dec_push(self.s, ptrs, sizes, c_segs, n, fin, tot, optrs, fmt, n_out)
        if rc:
            return rc, None
        for i in range(self.n):
            assert n_out[i] == lens[i] * self.ch and (outs[i][lens[i] * self.ch:] == 7).all()
            self.done[i] = 0 if fin[i] else self.done[i] + frames[i]
        return 0, [o[:v * self.ch] for o, v in zip(outs, lens)]


def pushes_for(E, x, ch, mode):
    """The pushes of one stream: [([(first_frame, n_frames, blob)], finish)]."""
    nf = DC.num_frames(x.size // ch)
    seg = lambda f0, n: (f0, n, E.range_blob(x, ch, f0, n))
    if mode == "one":       # one frame per push: the carry's save role reads the staged copy of the block it loaded
        return [([seg(f, 1)], f == nf - 1) for f in range(nf)]
    if mode == "two":
        return [([seg(f, min(2, nf - f))], f + 2 >= nf) for f in range(0, nf, 2)]
    if mode == "all":       # all segments of a clip in ONE push with the finish
        return [([seg(f, 1) for f in range(nf)], True)]
    if mode == "late":      # every frame first, then a finish that brings none: decoded from the carry alone
        return [([seg(0, nf)], False), ([], True)]
    raise ValueError(mode)


def drive(E, S, streams, mode, planar=False, fmt=PF32, host=False, between=None):
    """streams[i]: lane i's interleaved float stream.  Every lane goes through its pushes of `mode`, a lane that is done
    gets nothing.  -> per lane the concatenation of what its pushes emitted."""
    plans = [pushes_for(E, x, S.ch, mode) for x in streams]
    got = [[] for _ in streams]
    for k in range(max(len(p) for p in plans)):
        blob_segs, fin, tot = [], [], []
        for i, p in enumerate(plans):
            segs, f = p[k] if k < len(p) else ([], False)
            blob_segs += [(i, f0, n, b) for (f0, n, b) in segs]
            fin.append(f)
            tot.append(streams[i].size // S.ch if f else 0)
        if host:
            rc, outs = S.push_host(blob_segs, fin, tot, fmt)
            assert rc == 0, S.err()
        else:
            outs = S.push(blob_segs, fin, tot, planar, fmt)
        for i, o in enumerate(outs):
            got[i].append(o)
        if between:
            between()
    return [np.concatenate(g) for g in got]


def check_lanes(E, got, streams, ch, fmt=PF32):
    for i, x in enumerate(streams):
        w = E.want(x, ch)[0 if fmt == PF32 else 1]
        assert got[i].size == w.size and np.array_equal(bits(got[i]), bits(w)), f"lane {i} ({x.size // ch} samples) differs from glc_decode"


def edge_streams(ch):
    """The lengths at which the emission arithmetic turns, with a tone, a chord, noise (raw frames), silence and a noise
    burst inside a chord (raw frames next to compressed ones across a push boundary)."""
    burst = np.concatenate([chord(ch, 2900, 3), noise(ch, 1100, 4), chord(ch, 1000, 5)])
    return [tone(ch, 513), chord(ch, 1536, 1), tone(ch, 1537, 1000.0), chord(ch, 2047, 2), noise(ch, 2048, 6),
            np.zeros(2049 * ch, F32), burst]


# ------------------------------------------------------------------------------------------ 1. lengths, channels, chunkings

CASES = [(1, False, PF32), (2, True, PF32), (2, False, S16), (3, True, PF32), (3, False, PF32), (8, False, S16), (8, True, PF32),
         (5, False, PF32), (5, True, S16)]


@pytest.mark.parametrize("mode", ["one", "two", "all", "late"])
@pytest.mark.parametrize("ch,planar,fmt", CASES)
def test_every_chunking_decodes_to_the_same_samples(E, ch, planar, fmt, mode):
    """Seven lanes of different lengths in one session: they finish in different pushes, and the finished ones get nothing."""
    streams = edge_streams(ch)
    assert [DC.num_frames(x.size // ch) for x in streams] == [1, 1, 2, 2, 2, 2, 5]
    with Session(E, ch, len(streams)) as S:
        check_lanes(E, drive(E, S, streams, mode, planar, fmt), streams, ch, fmt)
        # a finished lane is fresh: the same session decodes the streams again, the other way round
        back = streams[::-1]
        check_lanes(E, drive(E, S, back, "two", planar, fmt), back, ch, fmt)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_lanes_through_host_pushes(E, n):
    ch = 2
    streams = edge_streams(ch)[-n:]
    with Session(E, ch, n) as S:
        check_lanes(E, drive(E, S, streams, "one", host=True), streams, ch)
        check_lanes(E, drive(E, S, streams, "late", fmt=S16, host=True), streams, ch, S16)


# ------------------------------------------------------------------------------------------ 2. rounds

def test_more_segments_than_a_round_holds(E):
    """600 lanes x 7 frames as three segments each: 1800 segments of 2 + 1, 2 + 1 and 3 + 1 slots against the 4097 of a
    round.  409 lanes fill 4090 slots and two more segments 4096, so lane 409 straddles the round boundary and hands its
    carry from one round's save to the next round's load."""
    ch, n, L = 2, 600, 7 * HOP - 200
    clips = [chord(ch, L, 21), np.concatenate([tone(ch, 3000), noise(ch, L - 3000, 22)]), tone(ch, L, 300.0)]
    parts = ((0, 2), (2, 2), (4, 3))
    assert DC.num_frames(L) == 7 and n * 10 > 4097 and 4097 - 409 * 10 == 3 + 3 + 1
    blobs = [E.range_blob(x, ch, f0, k) for x in clips for (f0, k) in parts]
    arena, ent9 = make_store(E, blobs)
    idx = E.torch.tensor([3 * (i % 3) + s for i in range(n) for s in range(3)], device="cuda")
    entries = ent9[idx].contiguous()                                 # the same nine blobs named by 1800 entries
    segs = [(i, f0, k) for i in range(n) for (f0, k) in parts]
    with Session(E, ch, n) as S:
        got = S.push_store(arena, entries, segs, [True] * n, [L] * n)
        st = (E.L.GlcCompactStatus * len(segs))()
        assert E.lib.glc_decode_compact_last_status(S.ctx._h, st, len(segs)) == 0
        assert all(s.flags == 0 and s.n_bad_rows == 0 for s in st)
    for i in range(n):
        w = E.want(clips[i % 3], ch)[0]
        assert np.array_equal(bits(got[i]), bits(w)), i


def test_one_lane_at_max_push(E):
    ch = 1
    nf = int(E.lib.glc_stream_dec_max_push(ch))
    assert nf == 4096 and E.lib.glc_stream_dec_max_push(0) == 0
    L = nf * HOP
    assert DC.num_frames(L) == nf
    t = np.arange(L, dtype=np.float64) / SR
    x = (0.4 * np.sin(2 * np.pi * 441.0 * t)).astype(F32)
    enc = E.enc.encode(x, ch)
    blob = E.g.frames_to_compact(enc)
    want = E.ref.decode(enc)
    with Session(E, ch, 1) as S:
        arena, entries = make_store(E, [blob])
        lay = OutLayout(ch, [L], False, PF32)
        d_out = E.dev(lay.flat)
        assert S.raw(arena, entries, [(0, 0, nf + 1)], [True], [L + HOP], lay, d_out, lens=[L + HOP]) == EINVAL   # a frame too many
        assert b"glc_stream_dec_max_push" in S.err()
        got = S.push_store(arena, entries, [(0, 0, nf)], [True], [L])
    assert np.array_equal(bits(got[0]), bits(want))


# ------------------------------------------------------------------------------------------ 3. the two encoders' segments

def test_segments_straight_from_the_stream_encoders_arena(E):
    """StreamEncoder.push_tensor -> StreamDecoder.push_tensor: arena, entries and segs go from one to the other as they
    are, nothing comes down.  Lane 1 has L + 512 a multiple of 1024: its finish brings no frames."""
    torch = E.torch
    ch, lens = 2, [4 * HOP + 9, 2 * HOP + 512, 6000]
    n = len(lens)
    xs = [chord(ch, lens[0], 31), tone(ch, lens[1], 700.0), np.concatenate([chord(ch, 3000, 32), noise(ch, 3000, 33)])]
    se = E.g.StreamEncoder(SR, ch, n_streams=n)
    sd = E.g.StreamDecoder(SR, ch, n_streams=n)
    arena = torch.zeros(1 << 21, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    cuts = [0, 1500, 1500, 2560, 3800, 5000, 6000]
    got, finished = [[] for _ in range(n)], [False] * n
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        take = [min(hi, L) - min(lo, L) for L in lens]
        fin = [hi >= L and not finished[i] for i, L in enumerate(lens)]
        t = torch.full((n, ch, max(max(take), 1) + 3), float("nan"), dtype=torch.float32, device="cuda")
        for i, x in enumerate(xs):
            if take[i]:
                a = min(lo, lens[i])
                t[i, :, :take[i]] = torch.from_numpy(x.reshape(-1, ch)[a:a + take[i]].T.copy()).cuda()
        entries, segs = se.push_tensor(t, take, fin, arena, cursor)
        planar = k % 2 == 0
        out, emitted = sd.push_tensor(arena, entries, segs, finish=fin, total_len=[L if f else 0 for L, f in zip(lens, fin)], planar=planar)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        for i in range(n):
            got[i].append((o[i, :, :emitted[i]].T if planar else o[i, :emitted[i], :]).reshape(-1).copy())
            finished[i] = finished[i] or fin[i]
        assert all(s.flags == 0 for s in sd.last_compact_status())
    assert all(finished) and [sd.frames_done(i) for i in range(n)] == [0] * n
    check_lanes(E, [np.concatenate(g) for g in got], xs, ch)
    with pytest.raises(E.g.GlcError):
        sd.push([None] * n)                                          # device pushes decided


def test_a_clip_stored_as_k_segments_decodes_in_one_call(E):
    torch = E.torch
    ch, L = 2, 5 * HOP + 77
    x = np.concatenate([chord(ch, 2000, 35), noise(ch, 1300, 36), chord(ch, L - 3300, 37)])
    se = E.g.StreamEncoder(SR, ch)
    arena = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    ents, segs = [], []
    cuts = [0, 1700, 2600, 4800, L]
    for lo, hi in zip(cuts, cuts[1:]):
        t = torch.from_numpy(x.reshape(-1, ch)[lo:hi].copy()).cuda().reshape(1, hi - lo, ch)
        e, s = se.push_tensor(t, None, [hi == L], arena, cursor, planar=False)
        ents.append(e)
        segs += s
    assert len(segs) >= 3 and sum(s[2] for s in segs) == DC.num_frames(L)
    entries = torch.cat(ents).contiguous()
    for dtype, k in ((None, 0), (np.int16, 1)):
        sd = E.g.StreamDecoder(SR, ch)
        out, emitted = sd.push_tensor(arena, entries, segs, finish=True, total_len=L, planar=False, dtype=dtype)
        torch.cuda.synchronize()
        assert emitted == [L]
        w = E.want(x, ch)[k]
        assert np.array_equal(bits(out.cpu().numpy()[0].reshape(-1)), bits(w))


def test_python_stream_decoder_host_pushes(E):
    """StreamEncoder.push -> .segments -> StreamDecoder.push, segment lists as they appear."""
    ch, L = 2, 7 * HOP + 3
    xs = [chord(ch, L, 41), noise(ch, 3 * HOP, 42)]
    se = E.g.StreamEncoder(SR, ch, n_streams=2)
    for dtype, k in ((F32, 0), (np.int16, 1)):
        sd = E.g.StreamDecoder(SR, ch, n_streams=2)
        assert sd.max_push == E.lib.glc_stream_dec_max_push(ch)
        got, seen = [[], []], [0, 0]
        cuts = [0, 900, 2600, 2600, 5100, L]
        for lo, hi in zip(cuts, cuts[1:]):
            Ls = [x.size // ch for x in xs]
            fin = [hi >= n and lo < n for n in Ls]
            se.push([x[min(lo, n) * ch: min(hi, n) * ch] for x, n in zip(xs, Ls)], finish=fin)
            new = []
            for i in range(2):
                s = se.segments(i)
                new.append(s[seen[i]:])
                seen[i] = len(s)
            outs = sd.push(new, finish=fin, total_len=[n if f else 0 for n, f in zip(Ls, fin)], dtype=dtype)
            for i in range(2):
                assert outs[i].dtype == dtype
                got[i].append(outs[i])
        for i, x in enumerate(xs):
            assert np.array_equal(bits(np.concatenate(got[i])), bits(E.want(x, ch)[k])), i
            se.encoded(i)                                            # takes the lane: the next round starts from nothing
        with pytest.raises(E.g.GlcError):
            sd.push_tensor(E.torch.zeros(64, dtype=E.torch.uint8, device="cuda"), None, [], finish=None)   # host pushes decided
    one = E.g.StreamDecoder(SR, 1)
    x = tone(1, 2000)
    segs = [(0, 2, E.range_blob(x, 1, 0, 2))]
    assert np.array_equal(bits(one.push(segs, finish=True, total_len=2000)[0]), bits(E.want(x, 1)[0]))   # a single lane takes a bare list
    p = E.g.plan_stream_dec_push(1, 2)
    assert (p.first_sample, p.n_samples) == (512, 2048)
    with pytest.raises(E.g.GlcError):
        E.g.plan_stream_dec_push(0, 2, True, 513)


# ------------------------------------------------------------------------------------------ 4. damage

def status(E, S, n):
    st = (E.L.GlcCompactStatus * n)()
    assert E.lib.glc_decode_compact_last_status(S.ctx._h, st, n) == 0, S.err()
    return [(s.flags, s.n_bad_rows, s.first_bad_row) for s in st]


@pytest.mark.parametrize("damage", ["magic", "frames", "unstored", "misaligned", "outside", "descending"])
def test_a_damaged_segment_is_silence_and_its_neighbours_are_not_affected(E, damage):
    """Lane 0's middle segment is damaged; the yardstick is the same stream with that segment replaced by a valid blob of
    the same frame count whose rows are all empty lists.  Lane 1 carries the undamaged stream."""
    ch, L = 2, 5000
    x = np.concatenate([chord(ch, 2900, 51), noise(ch, 1100, 52), chord(ch, 1000, 53)])
    parts = [(0, 2), (2, 2), (4, 1)]
    good = [E.range_blob(x, ch, f0, k) for (f0, k) in parts]
    empty = DC.compact_blob(ch, 2)
    flags, bad_rows = DC.BAD_HEADER, (4, 0)
    stored, gap, mid = None, 64, good[1]
    if damage == "magic":
        mid = DC.with_magic_flipped(good[1])
    elif damage == "frames":
        assert DC.header_frames(good[1]) == 2
        mid = DC.with_header_frames(good[1], 3)
    elif damage == "unstored":
        stored, flags, bad_rows = [True, False, True] + [True] * 3, DC.BAD_HEADER | DC.NO_BLOB, (0, 0)
    elif damage in ("misaligned", "outside"):
        flags, bad_rows = DC.BAD_HEADER | DC.NO_BLOB, (0, 0)
    elif damage == "descending":   # row 0 of the segment: two pairs whose bins do not ascend - rejected by R2's rule, the rest stands
        pair = lambda k, q: k | ((q & 0xFFFF) << 16)
        mid = DC.compact_blob(ch, 2, cnt=[2, 1, 0, 0], pairs=[pair(9, 40), pair(9, -3), pair(100, 50)], scale=[0.01, 0.02, 0, 0])
        empty = DC.compact_blob(ch, 2, cnt=[0, 1, 0, 0], pairs=[pair(100, 50)], scale=[0.01, 0.02, 0, 0])
        flags, bad_rows = DC.NOT_CANONICAL, (1, 0)
    blobs = [good[0], mid, good[2]] + good
    segs = [(0, f0, k) for (f0, k) in parts] + [(1, f0, k) for (f0, k) in parts]
    yard = E.decode_blobs([good[0], empty, good[2]], L * ch, ch)
    with Session(E, ch, 2) as S:
        arena, entries = make_store(E, blobs, stored)
        if damage == "misaligned":
            entries[1, 0] += 32
        if damage == "outside":
            entries[1, 1] = arena.numel() - int(entries[1, 0].item()) + 1
        got = S.push_store(arena, entries, segs, [True, True], [L, L])
        st = status(E, S, 6)
        assert st[1] == (flags,) + bad_rows and [s for j, s in enumerate(st) if j != 1] == [(0, 0, 0)] * 5, st
        assert np.array_equal(bits(got[0]), bits(yard)), "the damaged segment is not the empty one"
        assert np.array_equal(bits(got[1]), bits(E.want(x, ch)[0]))
        # ... and the same through the stream decoder itself, one segment per push, the empty blob in the damaged one's place
        a = [S.push([(0, f0, k, b)], [f0 == 4, False], [L, 0])[0] for (f0, k), b in zip(parts, [good[0], empty, good[2]])]
        assert np.array_equal(bits(np.concatenate(a)), bits(yard))
        if damage in ("magic", "frames", "descending"):
            b = [S.push([(0, f0, k, b)], [f0 == 4, False], [L, 0])[0] for (f0, k), b in zip(parts, [good[0], mid, good[2]])]
            assert np.array_equal(bits(np.concatenate(b)), bits(yard))
            assert status(E, S, 1) == [(0, 0, 0)]                   # the last push held the clean last segment alone


# ------------------------------------------------------------------------------------------ 5. sessions and the context

def test_two_sessions_on_one_context_and_other_calls_between_pushes(E):
    """No workspace of the context holds lane state: between two pushes the context encodes, decodes, fills a store and
    evicts from it, and a second session on the same context is pushed in between as well."""
    torch, lib = E.torch, E.lib
    ch = 2
    xa = [np.concatenate([chord(ch, 6000, 61), noise(ch, 1500, 62)]), tone(ch, 5000, 410.0)]
    xb = [chord(ch, 7000, 63)]
    other = chord(ch, 3 * HOP + 50, 64)
    frames = E.enc.encode(other, ch)
    want_other = E.ref.decode(frames)
    T = other.size // ch
    d_other = E.dev(np.stack([other, other * F32(0.5)]).reshape(2, T, ch))

    def between():
        h = E.ctx._h
        out = np.empty(other.size, F32)
        n = C.c_uint64()
        assert lib.glc_decode(h, frames._h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)) == 0
        assert np.array_equal(bits(out), bits(want_other))
        assert E.ctx.encode(other, ch).to_bytes() == frames.to_bytes()
        arena, cursor, entries = E.ctx.encode_compact_batch_tensor(d_other, planar=False)
        E.ctx.compact_store_tensor(arena, entries, None, torch.tensor([0, 1], dtype=torch.uint8, device="cuda"))

    with Session(E, ch, 2) as SA, Session(E, ch, 1) as SB:
        plan_b = pushes_for(E, xb[0], ch, "one")
        gb = []

        def both():
            between()
            if len(gb) < len(plan_b):
                segs, f = plan_b[len(gb)]
                gb.append(SB.push([(0, f0, k, b) for (f0, k, b) in segs], [f], [xb[0].size // ch if f else 0], fmt=S16)[0])

        ga = drive(E, SA, xa, "two", planar=True, between=both)
        while len(gb) < len(plan_b):
            both()
    check_lanes(E, ga, xa, ch)
    check_lanes(E, [np.concatenate(gb)], xb, ch, S16)


def test_a_push_leaves_the_context_as_the_compact_decode_does(E):
    """An accepted push clears the resident stream, closes an open decode session and drops the kept plan; a refused one,
    open, reset, close and the getters change nothing."""
    lib, ch = E.lib, 2
    h = E.ctx._h
    x = chord(ch, 3 * HOP, 65)
    frames = E.enc.encode(x, ch)
    chunk = np.empty(8 * HOP * ch, F32)
    n, last = C.c_uint64(), C.c_int()
    seg = (0, 0, 1, E.range_blob(x, ch, 0, 1))

    def begin():
        assert lib.glc_decode_stream_begin(h, frames._h) == 0
        assert lib.glc_ctx_resident_stream(h) != 0

    def next_chunk():
        return lib.glc_decode_stream_next(h, chunk.ctypes.data_as(C.c_void_p), chunk.size, C.byref(n), C.byref(last))

    begin()
    with Session(E, ch, 1) as S:
        arena, entries = make_store(E, [seg[3]])
        lay = OutLayout(ch, [512], False, PF32)
        d_out = E.dev(lay.flat)
        assert lib.glc_stream_dec_reset(S.s, 0) == 0 and S.frames_done(0) == 0
        assert S.raw(arena, entries, [(0, 1, 1)], None, None, lay, d_out) == EINVAL          # refused: not at frames_done
        assert lib.glc_ctx_resident_stream(h) != 0 and next_chunk() == 0                     # the session is still open
        begin()
        assert S.raw(arena, entries, [(0, 0, 1)], None, None, lay, d_out) == 0, S.err()      # accepted
        assert lib.glc_ctx_resident_stream(h) == 0 and next_chunk() == EINVAL
        st = (E.L.GlcCompactStatus * 1)()
        assert lib.glc_decode_compact_last_status(h, st, 1) == 0 and st[0].flags == 0        # one status per segment
        assert lib.glc_decode_compact_last_status(h, st, 2) == EINVAL
        begin()
    assert lib.glc_ctx_resident_stream(h) != 0                                               # close changes nothing
    assert next_chunk() == 0


def live(E):
    c = (C.c_uint64 * 4)()
    assert E.lib.glc_debug_live_resources(c) == 0
    return tuple(int(v) for v in c)


def test_a_stream_decoder_releases_everything_it_created(E):
    """The counts of tests/test_ctx_resources.py with the new family: after glc_stream_dec_close + glc_ctx_destroy they are
    what they were before glc_ctx_create, for a session of host pushes and one of device pushes."""
    ch, L = 2, 3000
    x = chord(ch, L, 66)
    nf = DC.num_frames(L)
    seg = (0, 0, nf, E.range_blob(x, ch, 0, nf))
    E.want(x, ch)
    gc.collect()
    before = live(E)
    for cycle in range(2):
        ctx = E.g.Encoder(SR)
        created = live(E)
        host, devp = Session(E, ch, 1, ctx), Session(E, ch, 1, ctx)
        opened = live(E)
        assert opened[0] == created[0] + 2                           # a session's carry is a device buffer of its own
        rc, outs = host.push_host([seg], [True], [L])
        assert rc == 0 and np.array_equal(bits(outs[0]), bits(E.want(x, ch)[0]))
        assert np.array_equal(bits(devp.push([seg], [True], [L])[0]), bits(E.want(x, ch)[0]))
        alive = live(E)
        assert alive[0] > opened[0] and alive[1] > opened[1], f"cycle {cycle}: {alive} against {opened}"
        host.close()
        devp.close()
        ctx.close()
        gc.collect()
        assert live(E) == before, f"cycle {cycle}: (device, pinned, streams, events) {live(E)} after destroy, {before} before create"


# ------------------------------------------------------------------------------------------ 6. refusals

def test_device_refusals_change_nothing(E):
    torch, lib = E.torch, E.lib
    ch, L = 2, 5000
    x = np.concatenate([chord(ch, 2900, 71), noise(ch, 2100, 72)])
    y = tone(ch, 3000, 900.0)
    with Session(E, ch, 2) as S:
        first = S.push([(0, 0, 2, E.range_blob(x, ch, 0, 2))], None, [0, 0], planar=True)
        assert S.done == [2, 0]
        blobs = [E.range_blob(x, ch, 2, 2), E.range_blob(y, ch, 0, 1)]
        arena, entries = make_store(E, blobs)
        segs = [(0, 2, 2), (1, 0, 1)]
        lens = [2048, 512]
        lay = OutLayout(ch, lens, True, PF32)
        d_out = E.dev(lay.flat)
        image = d_out.cpu().numpy().copy()
        ok = dict(arena=arena, entries=entries, segs=segs, finish=None, total=None, lay=lay, d_out=d_out)

        def refused(what=None, **bend):
            assert S.raw(**{**ok, **bend}) == EINVAL, bend
            if what:
                assert what in S.err(), (S.err(), bend)
            assert [S.frames_done(0), S.frames_done(1)] == [2, 0]

        refused(out_ptr=0)                                                                      # null output
        refused(null_lay=True)
        refused(entries_ptr=0)
        refused(arena_ptr=0)
        refused(b"64-byte", arena_ptr=arena.data_ptr() + 32)
        refused(b"8-byte", entries_ptr=entries.data_ptr() + 4)
        refused(b"aligned", out_ptr=d_out.data_ptr() + 2)
        refused(b"ascend", segs=[(1, 0, 1), (0, 2, 2)])                                         # out of lane order
        refused(b"ascend", segs=[(0, 2, 1), (1, 0, 1), (0, 3, 1)], lens=[2048, 512])            # a lane in two runs
        refused(b"does not start", segs=[(0, 3, 2), (1, 0, 1)])                                 # not at frames_done
        refused(b"does not start", segs=[(0, 2, 1), (0, 4, 1), (1, 0, 1)])                      # a gap inside the lane
        refused(b"no frames", segs=[(0, 2, 0), (1, 0, 1)])
        refused(b"no such stream", segs=[(0, 2, 2), (2, 0, 1)])
        refused(b"glc_stream_dec_max_push", segs=[(0, 2, int(lib.glc_stream_dec_max_push(ch)) + 1), (1, 0, 1)])
        refused(b"total_len", finish=[True, False], total=[L, 0])                               # 5 frames, the lane would have 4
        refused(b"total_len", finish=[True, False], total=[4 * HOP + 513, 0])
        refused(b"total_len", finish=[False, True], total=[0, 512 + HOP + 1], lens=[2048, 513 + HOP])   # 2 frames, the lane has 1
        refused(b"without total_len", finish=[True, False], total=[4 * HOP, 0], null_total=True)
        refused(b"n_clips", n_clips=3)
        refused(b"n_clips", lay_ch=3)
        refused(b"length", lens=[2049, 512])
        refused(b"length", lens=[2048, 0])
        narrow = OutLayout(ch, lens, True, PF32)
        narrow.channel_stride = 2047
        refused(b"channel_stride", lay=narrow)
        tight = OutLayout(ch, lens, True, PF32)
        tight.clip_stride = lay.channel_stride + 2047
        refused(b"clip_stride", lay=tight)
        refused(b"overlaps the arena", out_ptr=arena.data_ptr() + 128)
        big = torch.zeros(lay.size * 4 + 256, dtype=torch.uint8, device="cuda")                 # entries inside the output extent
        big[64:64 + 64] = entries.view(torch.uint8).reshape(-1)
        refused(b"overlaps the entries", entries_ptr=big.data_ptr() + 64, out_ptr=big.data_ptr())
        refused(b"out_fmt", fmt=2)
        refused(b"out_fmt", fmt=7)
        rc, _ = S.push_host([(0, 2, 2, blobs[0])], None, [0, 0])
        assert rc == EINVAL and b"device pushes" in S.err()
        S.done = [2, 0]                                                                        # (push_host's bookkeeping ran before the call)
        S.ctx.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(image)), "a refused push wrote to the output"
        # the carry is what it was: the streams continue to the reference's samples
        second = S.push([(0, 2, 2, blobs[0]), (1, 0, 1, blobs[1])], None, [0, 0], planar=True)
        third = S.push([(0, 4, 1, E.range_blob(x, ch, 4, 1)), (1, 1, 2, E.range_blob(y, ch, 1, 2))], [True, True], [L, 3000])
        check_lanes(E, [np.concatenate([first[0], second[0], third[0]]), np.concatenate([second[1], third[1]])], [x, y], ch)
        assert lib.glc_stream_dec_reset(S.s, 2) == EINVAL and lib.glc_stream_dec_frames_done(S.s, 2, C.byref(C.c_uint64())) == EINVAL
    s = C.c_void_p()
    assert lib.glc_stream_dec_open(E.ctx._h, 0, 1, C.byref(s)) == EINVAL and lib.glc_stream_dec_open(E.ctx._h, 2, 0, C.byref(s)) == EINVAL
    assert lib.glc_stream_dec_open(E.ctx._h, 2, 1, None) == EINVAL and lib.glc_stream_dec_open(E.ctx._h, 2, 1 << 60, C.byref(s)) == EINVAL


def test_host_refusals_change_nothing(E):
    ch, L = 2, 5000
    x = np.concatenate([chord(ch, 2900, 71), noise(ch, 2100, 72)])
    with Session(E, ch, 1) as S:
        rc, a = S.push_host([(0, 0, 2, E.range_blob(x, ch, 0, 2))], None, [0])
        assert rc == 0
        mid = (0, 2, 2, E.range_blob(x, ch, 2, 2))
        for bad in ([(0, 3, 2, mid[3])], [(0, 2, 0, mid[3])], [(1, 2, 2, mid[3])]):
            keep = list(S.done)
            assert S.push_host(bad, None, [0])[0] == EINVAL
            S.done = keep
        keep = list(S.done)
        assert S.push_host([mid], [True], [L])[0] == EINVAL and b"total_len" in S.err()
        assert S.push_host([mid], None, [0], fmt=2)[0] == EINVAL and b"out_fmt" in S.err()
        S.done = keep
        lay = OutLayout(ch, [2048], False, PF32)
        arena, entries = make_store(E, [mid[3]])
        assert S.raw(arena, entries, [(0, 2, 2)], None, None, lay, E.dev(lay.flat)) == EINVAL and b"host pushes" in S.err()
        assert S.frames_done(0) == 2
        rc, b = S.push_host([mid], None, [0])
        rc2, c = S.push_host([(0, 4, 1, E.range_blob(x, ch, 4, 1))], [True], [L])
        assert rc == 0 and rc2 == 0
        check_lanes(E, [np.concatenate([a[0], b[0], c[0]])], [x], ch)


# ------------------------------------------------------------------------------------------ 7. the carry kernel alone

@pytest.mark.parametrize("ch", [1, 3])
def test_the_carry_keeps_the_sign_of_zero(E, ch):
    """No decode produces -0.0 (the inverse transform accumulates from +0.0), so the carry kernel is driven alone: a
    carried sum of -0.0 + -0.0 is -0.0 and comes back from the load as -0.0 in the SECOND half of its pseudo-slot, where
    D2 adds nothing to it; with the frame before absent the sum starts from +0.0, as D2's does."""
    torch, lib = E.torch, E.lib
    f = lib.glc_debug_stream_dec_carry_device
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_uint16, C.c_void_p, C.c_uint64, C.c_void_p]
    h = E.ctx._h
    rng = np.random.default_rng(5)
    blocks = rng.standard_normal((4, ch, 2048)).astype(F32)
    blocks[0, :, 1024:1024 + 700] = -0.0       # second half of the frame before
    blocks[1, :, :600] = -0.0                  # first half of the last frame: -0.0 + -0.0 on [0, 600), x + -0.0 behind
    blocks[1, :, 1024:1030] = -0.0             # its second half: part (b)
    d_blocks = E.dev(blocks)
    d_carry = torch.full((2 * ch * 1024,), float("nan"), dtype=torch.float32, device="cuda")
    assert f(h, 1, 0, 1, ch, d_blocks.data_ptr(), 4, d_carry.data_ptr()) == 0, lib.glc_last_error(h)
    carry = d_carry.cpu().numpy().reshape(2, ch, 1024)
    want_a = (blocks[0, :, 1024:] + blocks[1, :, :1024]).astype(F32)
    assert np.array_equal(bits(carry[0]), bits(want_a)) and np.signbit(carry[0][:, :600]).all() and (carry[0][:, :600] == 0).all()
    assert np.array_equal(bits(carry[1]), bits(blocks[1, :, 1024:]))
    assert np.array_equal(bits(d_blocks.cpu().numpy()), bits(blocks))                          # the save role writes no block
    assert f(h, 0, 2, -1, ch, d_blocks.data_ptr(), 4, d_carry.data_ptr()) == 0                 # load into slots 2 and 3
    got = d_blocks.cpu().numpy()
    assert np.array_equal(bits(got[2, :, 1024:]), bits(carry[0])) and np.array_equal(bits(got[3, :, 1024:]), bits(carry[1]))
    assert np.array_equal(bits(got[:2]), bits(blocks[:2])) and np.array_equal(bits(got[2:, :, :1024]), bits(blocks[2:, :, :1024]))
    # the frame before absent: +0.0 + -0.0 = +0.0, D2's first hop
    assert f(h, 1, -1, 1, ch, d_blocks.data_ptr(), 4, d_carry.data_ptr()) == 0
    first = d_carry.cpu().numpy().reshape(2, ch, 1024)[0]
    assert np.array_equal(bits(first), bits((F32(0.0) + blocks[1, :, :1024]).astype(F32))) and not np.signbit(first[:, :600]).any()
    for bad in ((1, 0, 4), (1, -2, 1), (0, 3, -1), (0, -1, -1)):
        assert f(h, bad[0], bad[1], bad[2], ch, d_blocks.data_ptr(), 4, d_carry.data_ptr()) == EINVAL
    for blocks_at, carry_at in ((8, 0), (0, 4)):                                               # float4 accesses: 16-byte pointers
        assert f(h, 1, 0, 1, ch, d_blocks.data_ptr() + blocks_at, 4, d_carry.data_ptr() + carry_at) == EINVAL
        assert b"glc_debug_stream_dec_carry_device" in lib.glc_last_error(h) and b"16-byte" in lib.glc_last_error(h)


# ------------------------------------------------------------------------------------------ 8. the C++ mirror

def test_cpp_stream_decoder(E, tmp_path):
    exe = os.path.join(ROOT, "build", "glc_cpp_roundtrip")
    assert os.path.exists(exe), "build/glc_cpp_roundtrip missing: run __graft_entry__.build()"
    ch, L = 2, 9 * HOP + 41
    x = np.concatenate([chord(ch, L - 2100, 95), noise(ch, 2100, 10)])
    (tmp_path / "in.f32").write_bytes(x.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.f32"), str(SR), str(ch), str(tmp_path / "o.glc"), str(tmp_path / "o.f32"), "1000",
                        str(tmp_path / "s.glc"), str(tmp_path / "s.f32")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "s.f32").read_bytes(), F32)
    assert np.array_equal(bits(got), bits(E.want(x, ch)[0]))
