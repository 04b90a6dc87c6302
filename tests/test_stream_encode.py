"""The streaming encode: glc_stream_enc_push (host chunks) and glc_stream_enc_push_device (device chunks, many lanes per
launch chain).

The contract is equality of bytes and nothing else: a lane pushed in ANY chunking serialises to `O.encode` of the
concatenation (the CPU oracle) and to glc_encode of it; a device push stores, per segment, the blob that
glc_encode_range_device + glc_compact_device_records give for that frame range of the whole stream.  References are
computed once per signal and shared (`want`).  Layout padding holds NaN (floats) or full-scale integers."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import stream_encode_cases as SC
from conftest import O, ROOT, gen_chord, gen_noise, gen_tone

pytestmark = pytest.mark.gpu

F32 = np.float32
HOP, SR = SC.HOP, SC.SR
S16, S32, PF32 = SC.S16, SC.S32, SC.PF32
EINVAL = -1


class Env:
    def __init__(self):
        import torch
        import glc_amd
        assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
        self.torch, self.g, self.lib, self.L = torch, glc_amd, glc_amd.lib, glc_amd._lib
        self.enc = glc_amd.Encoder(SR)        # the context the sessions live on
        self.ref = glc_amd.Encoder(SR)        # the yardstick's context: glc_encode, range encode + compaction
        self.cache = {}

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    def want(self, x, ch):
        """(.glc bytes of the oracle, of glc_encode) of a float stream, computed once."""
        x = np.ascontiguousarray(x, F32)
        key = (hashlib.sha1(x.tobytes()).digest(), ch)
        if key not in self.cache:
            self.cache[key] = (O.encode(x, SR, ch).glc, self.ref.encode(x, ch).to_bytes())
        return self.cache[key]

    def range_blob(self, x, ch, f0, n):
        """glc_encode_range_device + glc_compact_device_records of frames [f0, f0 + n) of the whole float stream."""
        torch = self.torch
        L = x.size // ch
        d = self.dev(np.ascontiguousarray(x, F32))
        rec = torch.empty(n * int(self.lib.glc_record_bytes(ch)), dtype=torch.uint8, device="cuda")
        blob = torch.zeros(self.g.compact_bound(ch, n), dtype=torch.uint8, device="cuda")
        self.ref.encode_range_device(d.data_ptr(), 0, L, L * ch, ch, f0, f0 + n, rec.data_ptr())
        info = self.ref.compact_device_records(rec.data_ptr(), n, ch, blob.data_ptr(), blob.numel())
        return blob[:info.bytes].cpu().numpy().tobytes()

    def assemble(self, blobs, n_samples, ch):
        arrs = [np.frombuffer(b, np.uint8).copy() for b in blobs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_uint64 * len(arrs))(*[a.size for a in arrs])
        out = C.c_void_p()
        rc = self.lib.glc_frames_from_compact(SR, n_samples, ch, ptrs, sizes, len(arrs), C.byref(out))
        assert rc == 0, self.lib.glc_last_error(None)
        return self.g.EncodedAudio(out.value).to_bytes()


@pytest.fixture(scope="module")
def E():
    e = Env()
    yield e
    e.cache.clear()
    e.enc = e.ref = None


class Session:
    """glc_stream_enc_* through ctypes, on a context of the caller's."""

    def __init__(self, E, ch, n, ctx=None):
        self.E, self.ch, self.n, self.ctx = E, ch, n, ctx or E.enc
        s = C.c_void_p()
        assert E.lib.glc_stream_enc_open(self.ctx._h, ch, n, C.byref(s)) == 0, self.err()
        self.s = s

    def err(self):
        return self.E.lib.glc_last_error(self.ctx._h)

    def close(self):
        if self.s:
            self.E.lib.glc_stream_enc_close(self.s)
        self.s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, chunks, finish, fmt=PF32, bits=32):
        dt = SC.np_dtype(fmt) if fmt in (S16, S32, PF32) else F32
        arrs = [None if c is None or len(c) == 0 else np.ascontiguousarray(c, dt) for c in chunks]
        ptrs = (C.c_void_p * self.n)(*[a.ctypes.data if a is not None else None for a in arrs])
        ns = (C.c_uint64 * self.n)(*[a.size if a is not None else 0 for a in arrs])
        fin = None if finish is None else (C.c_uint8 * self.n)(*[1 if f else 0 for f in finish])
        return self.E.lib.glc_stream_enc_push(self.s, ptrs, fmt, bits, ns, fin)

    def segments(self, i):
        n = C.c_uint64()
        assert self.E.lib.glc_stream_enc_segments(self.s, i, C.byref(n)) == 0
        out = []
        for k in range(n.value):
            p, nb, f0, nf = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            assert self.E.lib.glc_stream_enc_segment(self.s, i, k, C.byref(p), C.byref(nb), C.byref(f0), C.byref(nf)) == 0
            out.append((f0.value, nf.value, C.string_at(p.value, nb.value)))
        return out

    def take(self, i):
        out = C.c_void_p()
        rc = self.E.lib.glc_stream_enc_frames(self.s, i, C.byref(out))
        assert rc == 0, self.err()
        return self.E.g.EncodedAudio(out.value).to_bytes()

    def push_device(self, lay, finish, arena, cursor, entries, bits=32, arena_bytes=None, ptr=None, lay_ch=None):
        """lay: SC.Layout already uploaded as lay.d -> (rc, [(lane, first_frame, n_frames)])."""
        Lc = self.E.L
        arr = (C.c_uint64 * self.n)(*lay.lens)
        cl = Lc.GlcClipLayout(self.n, lay_ch or self.ch, 1 if lay.planar else 0, lay.clip_stride, lay.channel_stride, 0,
                              C.cast(arr, C.POINTER(C.c_uint64)))
        fin = None if finish is None else (C.c_uint8 * self.n)(*[1 if f else 0 for f in finish])
        segs = (Lc.GlcStreamSeg * self.n)()
        n_segs = C.c_uint64(12345)
        p = lay.d.data_ptr() + lay.off * lay.d.element_size() if ptr is None else ptr
        rc = self.E.lib.glc_stream_enc_push_device(self.s, C.c_void_p(p), lay.fmt, bits, C.byref(cl), fin, C.c_void_p(arena.data_ptr()),
                                                   arena.numel() if arena_bytes is None else arena_bytes, C.c_void_p(cursor.data_ptr()),
                                                   C.c_void_p(entries.data_ptr()), segs, C.byref(n_segs))
        return rc, ([(g.stream, g.first_frame, g.n_frames) for g in segs[:n_segs.value]] if rc == 0 else None)


def schedule(lanes, ch):
    """lanes[i]: [(stream, sizes)] - stream i's interleaved samples and the per-channel sizes of its pushes, the last of
    which finishes it; the next stream of the lane starts with the push after.  Yields (chunks, finish) per push."""
    pos = [[0, 0, 0] for _ in lanes]
    while any(p[0] < len(l) for p, l in zip(pos, lanes)):
        chunks, fin = [], []
        for p, l in zip(pos, lanes):
            if p[0] >= len(l):
                chunks.append(None)
                fin.append(False)
                continue
            x, sizes = l[p[0]]
            n = sizes[p[1]]
            chunks.append(x[p[2] * ch:(p[2] + n) * ch])
            fin.append(p[1] == len(sizes) - 1)
            p[1] += 1
            p[2] += n
        yield chunks, fin
        for p, f in zip(pos, fin):
            if f:
                p[0], p[1], p[2] = p[0] + 1, 0, 0


def drive_host(S, lanes, fmt=PF32, bits=32):
    """-> per lane the .glc bytes of its streams, in order."""
    out = [[] for _ in lanes]
    for chunks, fin in schedule(lanes, S.ch):
        assert S.push(chunks, fin, fmt, bits) == 0, S.err()
        for i, f in enumerate(fin):
            if f:
                out[i].append(S.take(i))
    return out


def pattern(n, seed=0):
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    return ((i * np.uint64(167) + (i >> np.uint64(8)) * np.uint64(13)) % np.uint64(251) + np.uint64(3)).astype(np.uint8)


def drive_device(E, S, lanes, planar, fmt=PF32, bits=32, off=0, arena_size=1 << 22, between=None):
    """The same schedule through device pushes into ONE arena with one cursor.  -> (per lane, per stream: [(first_frame,
    n_frames, blob bytes)], the final arena, the intervals of its stored blobs)."""
    torch = E.torch
    image = pattern(arena_size, seed=5)
    arena = E.dev(image)
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = [[[]] for _ in lanes]
    received = [0] * len(lanes)
    spans, at = [], 0
    for chunks, fin in schedule(lanes, S.ch):
        lens = [0 if c is None else len(c) // S.ch for c in chunks]
        lay = SC.Layout(S.ch, lens, planar, fmt, off)
        for i, c in enumerate(chunks):
            if lens[i]:
                lay.put(i, np.asarray(c, SC.np_dtype(fmt)))
        lay.d = E.dev(lay.flat)
        entries = torch.full((S.n, 4), -1, dtype=torch.int64, device="cuda")
        rc, segs = S.push_device(lay, fin, arena, cursor, entries, bits)
        assert rc == 0, S.err()
        if between:
            between()
        S.ctx.synchronize()
        assert E.lib.glc_ctx_resident_stream(S.ctx._h) == 0
        assert torch.equal(lay.d.cpu(), torch.from_numpy(lay.flat)) or fmt == PF32      # (NaN != NaN: checked below for floats)
        if fmt == PF32:
            assert np.array_equal(lay.d.cpu().numpy().view(np.uint32), lay.flat.view(np.uint32))
        # the segments are the plan's, in lane order
        plan = []
        for i, n in enumerate(lens):
            if n or fin[i]:
                f0, nf, _ = SC.model_plan(received[i], n, fin[i], O.num_frames)
                if nf:
                    plan.append((i, f0, nf))
            received[i] = 0 if fin[i] else received[i] + n
        assert segs == plan, (segs, plan)
        ent = entries.cpu().numpy()
        assert (ent[len(segs):] == -1).all()                       # a lane that completes nothing writes no entry
        for j, (lane, f0, nf) in enumerate(segs):
            o, nb, _, rs = (int(v) for v in ent[j])
            assert rs >> 32 == 1 and o % 64 == 0 and o == at and nb % 64 == 0
            out[lane][-1].append((f0, nf, (o, o + nb)))
            spans.append((o, o + nb))
            at = o + nb
        assert int(cursor.item()) == at
        for i, f in enumerate(fin):
            if f:
                out[i].append([])
    a = arena.cpu().numpy()
    keep = np.ones(arena_size, bool)
    for lo, hi in spans:
        keep[lo:hi] = False
    assert np.array_equal(a[keep], image[keep])                     # no byte outside the stored blobs is written
    return [[[(f0, nf, a[lo:hi].tobytes()) for f0, nf, (lo, hi) in stream] for stream in o[:-1]] for o in out]


def chord(ch, L, seed):
    return gen_chord(SR, ch, L, seed=seed)


def noise(ch, L, seed):
    return gen_noise(SR, ch, L / SR + 0.01, seed)[:L * ch].copy()


def tone(ch, L, f=440.0):
    return gen_tone("sine", f, SR, ch, L / SR + 0.01)[:L * ch].copy()


def check_streams(E, got, lanes, ch, widen_bits=None):
    for i, l in enumerate(lanes):
        assert len(got[i]) == len(l)
        for k, (x, sizes) in enumerate(l):
            xf = x if widen_bits is None else SC.widen(x, widen_bits)
            oracle, single = E.want(xf, ch)
            assert got[i][k] == oracle, f"lane {i} stream {k} ({sum(sizes)} samples in {len(sizes)} pushes) differs from the oracle"
            assert got[i][k] == single, f"lane {i} stream {k} differs from glc_encode"


# ------------------------------------------------------------------------------------------ 1. chunkings, one lane, stereo

def test_every_push_one_sample_frame(E):
    ch, L = 2, 1700                                                 # a 2-frame stream
    assert O.num_frames(L, 1) == 2
    x = np.concatenate([chord(ch, 1200, 11), noise(ch, 500, 3)])
    with Session(E, ch, 1) as S:
        got = drive_host(S, [[(x, [1] * L)]])
    check_streams(E, got, [[(x, [1] * L)]], ch)


@pytest.mark.parametrize("size", [511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 5000])
def test_fixed_push_sizes(E, size):
    ch, L = 2, 12 * HOP + 777
    x = np.concatenate([chord(ch, L - 3000, 12), noise(ch, 3000, 4)])
    lanes = [[(x, SC.fixed_chunking(L, size)), (x, SC.fixed_chunking(L, size) + [0])]]       # ... and the finish as an empty push
    with Session(E, ch, 1) as S:
        got = drive_host(S, lanes)
        assert S.segments(0) == []
    check_streams(E, got, lanes, ch)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_pushes_at_the_completion_points(E, delta):
    ch, L = 2, 6 * HOP + 100
    x = chord(ch, L, 13)
    sizes = SC.boundary_chunking(L, delta)
    with Session(E, ch, 1) as S:
        # without the finish every push completes exactly the frames whose completion point it reaches
        received = 0
        for n in sizes[:-1]:
            assert S.push([x[received * ch:(received + n) * ch]], [False]) == 0, S.err()
            received += n
            assert sum(s[1] for s in S.segments(0)) == SC.frames_done(received)
        assert S.push([x[received * ch:]], [True]) == 0, S.err()
        segs = S.segments(0)
        assert [s[0] for s in segs] == list(np.cumsum([0] + [s[1] for s in segs[:-1]]))
        got = S.take(0)
    assert got == E.want(x, ch)[0] == E.want(x, ch)[1]


@pytest.mark.parametrize("L", [513, 1024, 1536, 1537, 2048, 2560, 2561])
def test_short_streams(E, L):
    ch = 2
    x = chord(ch, L, 14 + L)
    rng = np.random.default_rng(L)
    lanes = [[(x, [L]), (x, [L, 0]), (x, SC.random_chunking(rng, L, 700)), (x, SC.random_chunking(rng, L, 1100) + [0]),
              (x, SC.boundary_chunking(L, 0))]]
    with Session(E, ch, 1) as S:
        got = drive_host(S, lanes)
    check_streams(E, got, lanes, ch)


def test_a_finish_at_512_samples_is_refused_and_changes_nothing(E):
    ch, L = 2, 1800
    x = chord(ch, L, 15)
    with Session(E, ch, 1) as S:
        assert S.push([x[:512 * ch]], [False]) == 0
        assert S.push([None], [True]) == EINVAL and b"lane 0" in S.err()
        assert S.push([x[:0]], [True]) == EINVAL
        assert S.push([x[512 * ch:]], [True]) == 0, S.err()
        assert S.take(0) == E.want(x, ch)[0]
        assert S.push([x[:512 * ch]], [True]) == EINVAL              # ... in one push as well
        assert S.push([x], [True]) == 0
        assert S.take(0) == E.want(x, ch)[0]


# ------------------------------------------------------------------------------------------ 2. channels and formats

@pytest.mark.parametrize("ch", [1, 2, 3, 5, 8])
def test_channels_and_formats(E, ch):
    L = 4 * HOP + 321
    base = np.concatenate([chord(ch, L - 1500, 20 + ch), noise(ch, 1500, 5)]) * F32(0.9)
    rng = np.random.default_rng(ch)
    sizes = SC.random_chunking(rng, L, 1700)
    with Session(E, ch, 1) as S:
        lanes = [[(base, sizes)]]
        check_streams(E, drive_host(S, lanes), lanes, ch)
        for fmt, bits in ((S16, 16), (S16, 12), (S32, 24), (S32, 32)):
            xi = SC.to_int(base, fmt, bits)
            lanes = [[(xi, sizes), (xi, [L])]]
            got = drive_host(S, lanes, fmt, bits)
            check_streams(E, got, lanes, ch, widen_bits=bits)
            wide = SC.widen(xi, bits)
            assert drive_host(S, [[(wide, sizes)]])[0][0] == got[0][0]                       # the float push of the widened samples
            assert E.ref.encode(xi, ch, bits=bits).to_bytes() == got[0][0]                   # glc_encode_int


# ------------------------------------------------------------------------------------------ 3. many lanes

def lane_signal(i, ch, L):
    if i % 7 == 3:
        return noise(ch, L, 100 + i)                                # raw frames
    if i % 7 == 4:
        return np.zeros(L * ch, F32)                                # silence next to the noise
    if i % 7 == 5:
        return tone(ch, L, 300.0 + 10 * i)
    return chord(ch, L, 200 + i)


def many_lanes(n, ch, seed, biggest=2100):
    rng = np.random.default_rng(seed)
    lanes = []
    for i in range(n):
        streams = []
        for k in range(2 if i % 3 else 1):                          # most lanes start again after their first finish
            L = int(rng.integers(2 * HOP, 6 * HOP))
            streams.append((lane_signal(i + 64 * k, ch, L), SC.random_chunking(rng, L, biggest, zeros=0.3)))
        lanes.append(streams)
    return lanes


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_many_lanes_host(E, n):
    ch = 2
    lanes = many_lanes(n, ch, 31 + n)
    with Session(E, ch, n) as S:
        got = drive_host(S, lanes)
    check_streams(E, got, lanes, ch)


@pytest.mark.parametrize("planar,fmt,bits,off", [(False, PF32, 32, 0), (True, PF32, 32, 1), (True, S16, 16, 3), (False, S32, 24, 1)],
                         ids=("interleaved-f32", "planar-f32-odd-start", "planar-s16-odd-start", "interleaved-s32-odd-start"))
@pytest.mark.parametrize("n,ch", [(5, 2), (64, 2), (3, 3), (2, 5)])
def test_many_lanes_device(E, n, ch, planar, fmt, bits, off):
    if ("lanes", n, ch) not in E.cache:
        E.cache[("lanes", n, ch)] = many_lanes(n, ch, 41 + n)
    lanes = E.cache[("lanes", n, ch)]
    if fmt != PF32:
        lanes = [[(SC.to_int(x * F32(0.9), fmt, bits), sizes) for x, sizes in l] for l in lanes]
    with Session(E, ch, n) as S:
        got = drive_device(E, S, lanes, planar, fmt, bits, off, arena_size=(1 << 20) * max(4, n // 2))
    for i, l in enumerate(lanes):
        assert len(got[i]) == len(l)
        for k, (x, sizes) in enumerate(l):
            xf = x if fmt == PF32 else SC.widen(x, bits)
            assert E.assemble([b for _, _, b in got[i][k]], x.size, ch) == E.want(xf, ch)[0], (i, k)


def test_a_nan_lane_and_a_noise_lane_leave_their_neighbours_alone(E):
    ch, L = 2, 5 * HOP + 17
    rng = np.random.default_rng(77)
    xs = [tone(ch, L, 500.0), np.full(L * ch, np.nan, F32), tone(ch, L, 700.0), noise(ch, L, 9), np.zeros(L * ch, F32)]
    lanes = [[(x, SC.random_chunking(rng, L, 1500))] for x in xs]
    with Session(E, ch, 5) as S:
        got = drive_host(S, lanes)
    for i in (0, 2, 3, 4):
        assert got[i][0] == E.want(xs[i], ch)[0] == E.want(xs[i], ch)[1], i
    assert got[1][0] == E.ref.encode(xs[1], ch).to_bytes()          # the NaN lane itself: what glc_encode makes of it


def test_one_push_of_more_frames_than_a_round(E):
    ch, n, nf = 2, 5, 1000
    L = nf * HOP + 512
    assert O.num_frames(L, 1) == nf and n * (nf + 1) + 1 > 4096
    base = gen_chord(SR, ch, L + 4 * 999, seed=51, n_tones=4)
    xs = [(base[i * 999 * ch: (i * 999 + L) * ch] * F32(1.0 - 0.1 * i)).astype(F32) for i in range(n)]
    lanes = [[(x, [L])] for x in xs]
    with Session(E, ch, n) as S:
        got = drive_host(S, lanes)
        with Session(E, ch, n, ctx=E.ref) as S2:
            dev = drive_device(E, S2, lanes, True, arena_size=n * E.g.compact_bound(ch, nf) + 4096)
    for i, x in enumerate(xs):
        assert got[i][0] == E.want(x, ch)[0] == E.want(x, ch)[1], i
        assert [(f0, k) for f0, k, _ in dev[i][0]] == [(0, nf)]
        assert E.assemble([dev[i][0][0][2]], x.size, ch) == got[i][0]


def test_a_host_chunk_above_max_push_is_split(E):
    """One finishing push of more samples than a device push takes: several segments, the same bytes."""
    ch = 2
    L = int(E.lib.glc_stream_enc_max_push(ch)) + 5000
    second = chord(ch, SR, 52).reshape(SR, ch)
    x = np.tile(second, (L // SR + 1, 1))[:L]
    x = (x * np.linspace(0.2, 1.0, L, dtype=F32)[:, None]).astype(F32).reshape(-1)
    with Session(E, ch, 2) as S:
        assert S.push([None, x], [False, True]) == 0, S.err()
        segs = S.segments(1)
        assert len(segs) == 2 and segs[0][0] == 0 and segs[1][0] == segs[0][1]
        assert segs[0][1] + segs[1][1] == O.num_frames(L, 1) and S.segments(0) == []
        got = S.take(1)
    assert got == E.want(x, ch)[0] == E.want(x, ch)[1]


# ------------------------------------------------------------------------------------------ 4. device push

def test_device_blobs_equal_range_encode_plus_compaction(E):
    ch, n = 2, 3
    rng = np.random.default_rng(61)
    xs = [np.concatenate([chord(ch, 5000, 61), noise(ch, 2200, 6)]), tone(ch, 3 * HOP + 5, 610.0), chord(ch, 9000, 62)]
    lanes = [[(x, SC.random_chunking(rng, x.size // ch, 2600, zeros=0.2))] for x in xs]
    with Session(E, ch, n) as S:
        got = drive_device(E, S, lanes, False, off=1)
    for i, x in enumerate(xs):
        segs = got[i][0]
        assert [f0 for f0, _, _ in segs] == list(np.cumsum([0] + [k for _, k, _ in segs[:-1]]))
        assert sum(k for _, k, _ in segs) == O.num_frames(x.size // ch, 1)
        for f0, k, blob in segs:
            assert blob == E.range_blob(x, ch, f0, k), (i, f0, k)


def test_an_arena_that_is_too_small(E):
    torch = E.torch
    ch, n = 2, 3
    xs = [chord(ch, 3 * HOP, 63), noise(ch, 2 * HOP + 9, 7), chord(ch, 4 * HOP, 64)]
    lens = [x.size // ch for x in xs]

    def run(arena_bytes, size):
        image = pattern(size, seed=9)
        arena = E.dev(image)
        cursor = torch.tensor([70], dtype=torch.int64, device="cuda")
        entries = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
        lay = SC.Layout(ch, lens, True, PF32, 2)
        for i, x in enumerate(xs):
            lay.put(i, x)
        lay.d = E.dev(lay.flat)
        with Session(E, ch, n) as S:
            rc, segs = S.push_device(lay, [True] * n, arena, cursor, entries, arena_bytes=arena_bytes)
            assert rc == 0, S.err()
            E.enc.synchronize()
        return image, arena.cpu().numpy(), int(cursor.item()), entries.cpu().numpy(), segs

    size = 1 << 20
    image, a, cur, ent, segs = run(size, size)
    assert segs == [(i, 0, O.num_frames(lens[i], 1)) for i in range(n)]
    assert ent[0][0] == 128 and cur == int(ent[2][0] + ent[2][1]) and ((ent[:, 3] >> 32) == 1).all()
    cut = int(ent[2][0] + ent[2][1]) - 1                            # one byte short of the last blob
    image2, a2, cur2, ent2, _ = run(cut, size)
    assert cur2 == cur                                              # the size that would have sufficed
    assert np.array_equal(ent2[:, :3], ent[:, :3]) and list(ent2[:, 3] >> 32) == [1, 1, 0]
    assert np.array_equal(ent2[:, 3] & 0xFFFFFFFF, ent[:, 3] & 0xFFFFFFFF)
    lo = int(ent[2][0])
    assert np.array_equal(a2[:lo], a[:lo]) and np.array_equal(a2[lo:], image2[lo:])      # nothing of that blob was written


def test_two_sessions_on_one_context_and_other_calls_between_pushes(E):
    """The workspace rule: no workspace of the context holds lane state.  Between two pushes of lanes that hold samples
    back the context runs a batch round trip, a glc_encode, a store encode and a draw from that store; a second session on
    the same context is pushed in between as well."""
    torch, lib, Lc = E.torch, E.lib, E.L
    ch = 2
    rng = np.random.default_rng(71)
    xa = [np.concatenate([chord(ch, 6000, 71), noise(ch, 1500, 8)]), tone(ch, 5000, 410.0)]
    xb = [chord(ch, 7000, 72)]
    la = [[(x, SC.random_chunking(rng, x.size // ch, 1300, zeros=0.1))] for x in xa]
    lb = [[(x, SC.random_chunking(rng, x.size // ch, 900, zeros=0.1))] for x in xb]
    other = chord(ch, 3 * HOP + 50, 73)
    d_other = E.dev(np.stack([other, other * F32(0.5)]))             # (2, T * ch): two interleaved clips
    T = other.size // ch
    lay = Lc.GlcClipLayout(2, ch, 0, T * ch, 0, T, None)

    def between():
        h = E.enc._h
        out = torch.empty_like(d_other)
        assert lib.glc_roundtrip_batch_device(h, C.c_void_p(d_other.data_ptr()), C.byref(lay), C.c_void_p(out.data_ptr()), C.byref(lay)) == 0
        assert E.enc.encode(other, ch).to_bytes() == E.want(other, ch)[1]
        arena, cursor, entries = E.enc.encode_compact_batch_tensor(d_other.reshape(2, T, ch), planar=False)
        lengths = torch.full((2,), T, dtype=torch.int64, device="cuda")
        clips = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
        starts = torch.tensor([5, 100], dtype=torch.int64, device="cuda")
        crop = torch.empty((2, 700 * ch), dtype=torch.float32, device="cuda")
        lay_o = Lc.GlcClipLayout(2, ch, 0, 700 * ch, 0, 700, None)
        assert lib.glc_decode_crops_device_store(h, C.c_void_p(arena.data_ptr()), arena.numel(), C.c_void_p(entries.data_ptr()),
                                                 C.c_void_p(lengths.data_ptr()), 2, T, C.c_void_p(clips.data_ptr()),
                                                 C.c_void_p(starts.data_ptr()), 700, C.c_void_p(crop.data_ptr()), C.byref(lay_o)) == 0, \
            lib.glc_last_error(h)

    with Session(E, ch, 2) as SA, Session(E, ch, 1) as SB:
        gb = [[]]
        it_b = schedule(lb, ch)

        def both():
            between()
            nxt = next(it_b, None)
            if nxt is not None:
                assert SB.push(nxt[0], nxt[1]) == 0, SB.err()
                if nxt[1][0]:
                    gb[0].append(SB.take(0))

        ga = drive_device(E, SA, la, True, between=both)
        for chunks, fin in it_b:
            assert SB.push(chunks, fin) == 0, SB.err()
            if fin[0]:
                gb[0].append(SB.take(0))
    for i, x in enumerate(xa):
        assert E.assemble([b for _, _, b in ga[i][0]], x.size, ch) == E.want(x, ch)[0], i
    assert gb[0] == [E.want(xb[0], ch)[0]]


# ------------------------------------------------------------------------------------------ 5. refusals

def test_host_refusals_change_nothing(E):
    ch, L = 2, 4000
    x, y = chord(ch, L, 81), chord(ch, L, 82)
    with Session(E, ch, 2) as S:
        assert S.push([x[:1000 * ch], y[:700 * ch]], None) == 0
        held = [S.segments(0), S.segments(1)]
        assert S.push([x[:1001], None], None) == EINVAL and b"multiple of channels" in S.err()
        bad = (C.c_void_p * 2)(None, None)
        ns = (C.c_uint64 * 2)(2 * ch, 0)
        assert E.lib.glc_stream_enc_push(S.s, bad, PF32, 32, ns, None) == EINVAL                        # null samples
        odd = np.zeros(64, np.uint8)
        bad = (C.c_void_p * 2)(odd.ctypes.data + 1, None)
        assert E.lib.glc_stream_enc_push(S.s, bad, PF32, 32, ns, None) == EINVAL                        # misaligned samples
        assert E.lib.glc_stream_enc_push(S.s, None, PF32, 32, ns, None) == EINVAL
        assert S.push([x[:2 * ch], None], None, fmt=7) == EINVAL and S.push([x[:2 * ch], None], None, fmt=S16, bits=17) == EINVAL
        # a device push on a session that takes host pushes
        lay = SC.Layout(ch, [8, 8], False, PF32)
        lay.d = E.dev(lay.flat)
        arena = E.torch.zeros(1 << 16, dtype=E.torch.uint8, device="cuda")
        cursor = E.torch.zeros(1, dtype=E.torch.int64, device="cuda")
        entries = E.torch.zeros((2, 4), dtype=E.torch.int64, device="cuda")
        assert S.push_device(lay, None, arena, cursor, entries)[0] == EINVAL and b"host pushes" in S.err()
        assert [S.segments(0), S.segments(1)] == held
        # lane 0 finishes; until it is taken it refuses samples and a second finish, lane 1 goes on
        assert S.push([x[1000 * ch:], y[700 * ch:2000 * ch]], [True, False]) == 0, S.err()
        assert S.push([x[:10 * ch], y[2000 * ch:]], [False, True]) == EINVAL and b"lane 0" in S.err()
        assert S.push([None, None], [True, False]) == EINVAL
        out = C.c_void_p()
        assert E.lib.glc_stream_enc_frames(S.s, 1, C.byref(out)) == EINVAL                              # lane 1 is not finished
        assert S.push([None, y[2000 * ch:]], [False, True]) == 0, S.err()
        assert S.take(0) == E.want(x, ch)[0] and S.take(1) == E.want(y, ch)[0]
        # reset drops what a lane holds; the lane starts again from nothing
        assert S.push([y[:3000 * ch], None], None) == 0
        assert E.lib.glc_stream_enc_reset(S.s, 0) == 0 and E.lib.glc_stream_enc_reset(S.s, 2) == EINVAL
        assert S.segments(0) == []
        assert S.push([x, None], [True, False]) == 0
        assert S.take(0) == E.want(x, ch)[0]


def test_device_refusals_change_nothing(E):
    torch = E.torch
    ch, L = 2, 4000
    x = chord(ch, L, 83)
    arena = E.dev(pattern(1 << 18))
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    entries = torch.full((1, 4), -1, dtype=torch.int64, device="cuda")

    def layout(lo, hi):
        lay = SC.Layout(ch, [hi - lo], True, PF32, 1)
        lay.put(0, x[lo * ch:hi * ch])
        lay.d = E.dev(lay.flat)
        return lay

    with Session(E, ch, 1) as S:
        rc, segs = S.push_device(layout(0, 1900), None, arena, cursor, entries)
        assert rc == 0 and segs == [(0, 0, 1)]
        E.enc.synchronize()
        state = (arena.cpu().numpy().copy(), int(cursor.item()), entries.cpu().numpy().copy())
        lay = layout(1900, 2500)
        big = SC.Layout(ch, [8], True, PF32, 1)
        big.d = lay.d
        big.lens = [int(E.lib.glc_stream_enc_max_push(ch)) + 1]
        assert S.push_device(big, None, arena, cursor, entries)[0] == EINVAL and b"glc_stream_enc_max_push" in S.err()
        assert S.push([x[:2 * ch]], None) == EINVAL and b"device pushes" in S.err()                     # a host push after a device push
        assert S.push_device(lay, None, arena, cursor, entries, ptr=0)[0] == EINVAL                    # null input
        assert S.push_device(lay, None, arena, cursor, entries, ptr=lay.d.data_ptr() + 2)[0] == EINVAL  # misaligned input
        assert S.push_device(lay, None, arena[32:], cursor, entries)[0] == EINVAL                       # arena not 64-byte aligned
        assert S.push_device(lay, None, arena, cursor.view(torch.uint8)[4:].view(torch.int32), entries)[0] == EINVAL
        as_arena = lay.d.view(torch.uint8)
        assert S.push_device(lay, None, as_arena, cursor, entries, arena_bytes=256)[0] == EINVAL        # an arena that overlaps the input
        assert b"overlaps" in S.err()
        as_entries = lay.d.view(torch.uint8)[64:]
        assert S.push_device(lay, None, arena, cursor, as_entries)[0] == EINVAL                         # entries inside the input
        assert b"glc_stream_enc_push_device" in S.err() and b"entries overlap" in S.err()
        lay.fmt = 7
        assert S.push_device(lay, None, arena, cursor, entries)[0] == EINVAL and b"sample format" in S.err()
        lay.fmt = PF32
        assert S.push_device(lay, None, arena, cursor, entries, bits=0)[0] == 0                         # (bits is ignored for floats)
        E.enc.synchronize()
        assert int(cursor.item()) == state[1]                                                           # 2500 samples: still one frame
        narrow = SC.Layout(ch, [600], True, PF32, 1)
        narrow.d, narrow.channel_stride = lay.d, 10
        assert S.push_device(narrow, None, arena, cursor, entries)[0] == EINVAL and b"channel_stride" in S.err()
        assert S.push_device(lay, None, arena, cursor, entries, lay_ch=3)[0] == EINVAL                  # the layout is not the session's
        assert S.push_device(layout(2500, 2500), [True], arena, cursor, entries)[0] == 0                # an empty finishing push ... of 2500
        E.enc.synchronize()
        a = arena.cpu().numpy()
        ent = entries.cpu().numpy()[0]
        assert np.array_equal(a[:state[1]], state[0][:state[1]])
        blobs = [state[0][int(state[2][0][0]):state[1]].tobytes(), a[int(ent[0]):int(ent[0] + ent[1])].tobytes()]
        assert E.assemble(blobs, 2500 * ch, ch) == E.want(x[:2500 * ch], ch)[0]


def test_a_push_leaves_the_context_as_the_store_encode_does(E):
    """An accepted push - even one that completes no frame - clears the resident stream and closes an open decode
    session; a refused one changes nothing."""
    lib, ch = E.lib, 2
    h = E.enc._h
    x = chord(ch, 3 * HOP, 85)
    frames = E.ref.encode(x, ch)
    chunk = np.empty(8 * HOP * ch, F32)
    n, last = C.c_uint64(), C.c_int()

    def begin():
        assert lib.glc_decode_stream_begin(h, frames._h) == 0
        assert lib.glc_ctx_resident_stream(h) != 0

    def next_chunk():
        return lib.glc_decode_stream_next(h, chunk.ctypes.data_as(C.c_void_p), chunk.size, C.byref(n), C.byref(last))

    with Session(E, ch, 1) as S:
        begin()
        assert S.push([x[:100 * ch]], [True]) == EINVAL                  # refused: 100 samples end no stream
        assert S.push([x[:101]], None) == EINVAL
        assert lib.glc_ctx_resident_stream(h) != 0 and next_chunk() == 0  # the session is still open
        begin()
        assert S.push([x[:100 * ch]], None) == 0                          # accepted, completes nothing
        assert lib.glc_ctx_resident_stream(h) == 0 and next_chunk() == EINVAL
        begin()
        assert S.push([None], None) == 0                                  # accepted, queues nothing
        assert lib.glc_ctx_resident_stream(h) == 0 and next_chunk() == EINVAL
        begin()
        assert lib.glc_stream_enc_reset(S.s, 0) == 0 and S.segments(0) == []
        assert lib.glc_ctx_resident_stream(h) != 0                       # reset and the getters change nothing
        assert S.push([x], [True]) == 0
        assert lib.glc_ctx_resident_stream(h) == 0
        assert S.take(0) == E.want(x, ch)[0]


# ------------------------------------------------------------------------------------------ 6. wrappers

def test_python_stream_encoder_host(E):
    ch, L = 2, 7 * HOP + 3
    x, y = chord(ch, L, 91), SC.to_int(chord(ch, L, 92), S16, 16)
    se = E.g.StreamEncoder(SR, ch, n_streams=2)
    assert se.max_push == E.lib.glc_stream_enc_max_push(ch)
    rng = np.random.default_rng(91)
    at = 0
    for n in SC.random_chunking(rng, L, 2500):
        se.push([x[at * ch:(at + n) * ch], None])
        at += n
    se.push([None, None], finish=[True, False])
    segs = se.segments(0)
    assert sum(s[1] for s in segs) == O.num_frames(L, 1) and segs[0][0] == 0
    assert E.assemble([s[2] for s in segs], x.size, ch) == E.want(x, ch)[0]
    assert se.encoded(0).to_bytes() == E.want(x, ch)[0]
    se.push([None, y], finish=[False, True])                        # 16-bit integers
    assert se.encoded(1).to_bytes() == E.want(SC.widen(y, 16), ch)[0]
    with pytest.raises(E.g.GlcError):
        se.encoded(1)
    se.push([x[:1000], None])
    se.reset(0)
    one = E.g.StreamEncoder(SR, 1)
    one.push(x[:L], finish=True)                                    # a single lane takes a bare array
    assert one.encoded().to_bytes() == E.want(x[:L], 1)[0]


def test_python_stream_encoder_push_tensor(E):
    torch = E.torch
    ch, n, L = 2, 3, 4 * HOP + 9
    xs = [chord(ch, L, 93 + i) for i in range(n)]
    se = E.g.StreamEncoder(SR, ch, n_streams=n)
    arena = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    blobs = [[] for _ in range(n)]
    cuts = [0, 1500, 1500, 3800, L]
    for lo, hi in zip(cuts, cuts[1:]):
        t = torch.full((n, ch, hi - lo + 5), float("nan"), dtype=torch.float32, device="cuda")     # planar (B, C, T), padded
        for i, x in enumerate(xs):
            t[i, :, :hi - lo] = torch.from_numpy(x.reshape(L, ch)[lo:hi].T.copy()).cuda()
        lens = [hi - lo, hi - lo, 0 if hi < L else L]                # lane 2 sends everything in the last push
        if hi == L:
            t2 = torch.full((n, ch, L), float("nan"), dtype=torch.float32, device="cuda")
            t2[:, :, :hi - lo] = t[:, :, :hi - lo]
            t2[2] = torch.from_numpy(xs[2].reshape(L, ch).T.copy()).cuda()
            t = t2
        entries, segs = se.push_tensor(t, lens, [hi == L] * n, arena, cursor)
        torch.cuda.synchronize()
        a = arena.cpu().numpy()
        assert entries.shape[0] == len(segs)
        for (lane, f0, nf), e in zip(segs, entries.cpu().numpy()):
            assert e[3] >> 32 == 1
            blobs[lane].append(a[int(e[0]):int(e[0] + e[1])].tobytes())
    for i, x in enumerate(xs):
        assert E.assemble(blobs[i], x.size, ch) == E.want(x, ch)[0], i
    with pytest.raises(E.g.GlcError):
        se.push([None] * n)                                         # device pushes decided


def test_cpp_stream_encoder(E, tmp_path):
    exe = os.path.join(ROOT, "build", "glc_cpp_roundtrip")
    assert os.path.exists(exe), "build/glc_cpp_roundtrip missing: run __graft_entry__.build()"
    ch, L = 2, 9 * HOP + 41
    x = np.concatenate([chord(ch, L - 2100, 95), noise(ch, 2100, 10)])
    (tmp_path / "in.f32").write_bytes(x.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.f32"), str(SR), str(ch), str(tmp_path / "o.glc"), str(tmp_path / "o.f32"), "1000",
                        str(tmp_path / "s.glc")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "s.glc").read_bytes() == E.want(x, ch)[0]
