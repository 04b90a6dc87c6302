"""Integer PCM on the device batch and store paths: glc_encode_batch_device_compact_int, glc_roundtrip_batch_device_pcm,
glc_decode_batch_device_compact_i16, glc_decode_crops_device_compact_i16 and glc_decode_crops_device_store_i16.

Yardsticks are never the code under test.  For inputs it is the unchanged float call on the output of the unchanged
glc_pcm_widen_device (and, twice, the CPU oracle); for outputs it is the numpy `narrow` of the unchanged float call's
output (tests/store_int_cases.py).  Everything is compared bit for bit or byte for byte: whole arenas, entries, cursors,
every element of every output buffer, every status word.  Integer batches are flat arrays whose every element outside
the clips' true samples is a full-scale integer (the float twin gets NaN there), outputs are filled with the sentinel
0x5A5A.  Damaged blobs are those of compact_decode_cases (every count inside its buffer): the tests pin the defined
result, they provoke nothing."""
import ctypes as C

import numpy as np
import pytest

import compact_decode_cases as K
import store_draw_cases as SD
import store_int_cases as SI
from conftest import O

pytestmark = pytest.mark.gpu

F32 = np.float32
HOP = SI.HOP
SR = SI.SR
S16, S32, PF32 = SI.S16, SI.S32, SI.PF32
EINVAL = -1
NAN_BITS = 0x7FC05A5A


class Env:
    def __init__(self):
        import torch
        import glc_amd
        assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
        self.torch, self.g, self.lib, self.L = torch, glc_amd, glc_amd.lib, glc_amd._lib
        self._ctx = {}
        self.cache = {}

    def ctx(self, kind, ch=2):
        key = (kind, ch)
        if key not in self._ctx:
            g = self.g
            self._ctx[key] = g.Encoder(SR) if kind.startswith("enc") else g.RoundTrip(SR) if kind.startswith("rt") else g.Decoder(ch, SR)
        return self._ctx[key]

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    def err(self, ctx):
        return self.lib.glc_last_error(ctx._h)

    def layout(self, b):
        """glc_clip_layout of a store_int_cases.Batch (+ the array it points into)."""
        arr = (C.c_uint64 * max(b.n_clips, 1))(*b.lengths)
        lay = self.L.GlcClipLayout(b.n_clips, b.ch, 1 if b.planar else 0, b.clip_stride, b.channel_stride, max(b.lengths),
                                   C.cast(arr, C.POINTER(C.c_uint64)))
        return lay, arr

    def status(self, ctx, n):
        st = (self.L.GlcCompactStatus * n)()
        rc = self.lib.glc_decode_compact_last_status(ctx._h, st, n)
        return rc, [(s.flags, s.n_bad_rows, s.first_bad_row) for s in st]

    def batch_info(self, ctx, n):
        info = (self.L.GlcRoundtripInfo * n)()
        rc = self.lib.glc_roundtrip_batch_last_info(ctx._h, info, n)
        return rc, [(i.n_frames, i.n_raw_frames, i.total_nnz, i.serialized_bytes) for i in info]


def at(t, off):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


@pytest.fixture(scope="module")
def E():
    e = Env()
    yield e
    e.cache.clear()
    e._ctx.clear()           # contexts: released while the library is still loaded


def family(E, fmt, bits, ch):
    key = ("family", fmt, bits, ch)
    if key not in E.cache:
        E.cache[key] = SI.family_clips(fmt, bits, ch)
    return E.cache[key]


def pattern(n, seed=0):
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    return ((i * np.uint64(167) + (i >> np.uint64(8)) * np.uint64(13)) % np.uint64(251) + np.uint64(3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------ encode to store

def widened_twin(E, b, d_int, fmt, bits):
    """The float batch of the same layout: glc_pcm_widen_device over the whole flat array, NaN outside the clips."""
    torch = E.torch
    enc = E.ctx("enc-f32")
    d_f = torch.empty(b.flat.size, dtype=torch.float32, device="cuda")
    assert E.lib.glc_pcm_widen_device(enc._h, C.c_void_p(d_int.data_ptr()), fmt, bits, b.flat.size, C.c_void_p(d_f.data_ptr())) == 0
    enc.synchronize()
    d_f.view(torch.int32)[E.dev(~b.mask)] = NAN_BITS
    return d_f


def store_both(E, b, fmt, bits, cursor0=0, arena_bytes=None, calls=1, slack=4096):
    """The float call on the widened twin and the integer call on the integers, each `calls` times through one cursor
    into a pattern-filled arena of its own -> ((arena, entries, cursor) of the float side, ... of the integer side)."""
    torch, lib = E.torch, E.lib
    d_int = E.dev(b.flat)
    d_f = widened_twin(E, b, d_int, fmt, bits)
    lay, _keep = E.layout(b)
    bound = int(lib.glc_compact_store_bound(C.byref(lay)))
    size = cursor0 + 64 + calls * bound + slack
    offered = size if arena_bytes is None else arena_bytes
    image = pattern(size, seed=3)
    sides = []
    for which in ("f32", "int"):
        enc = E.ctx("enc-" + which)
        arena = E.dev(image)
        cursor = torch.tensor([cursor0], dtype=torch.int64, device="cuda")
        entries = torch.full((calls * b.n_clips, 4), -1, dtype=torch.int64, device="cuda")
        for k in range(calls):
            ent = C.c_void_p(entries.data_ptr() + 32 * k * b.n_clips)
            if which == "f32":
                rc = lib.glc_encode_batch_device_compact(enc._h, at(d_f, b.off), C.byref(lay), C.c_void_p(arena.data_ptr()), offered,
                                                         C.c_void_p(cursor.data_ptr()), ent)
            else:
                rc = lib.glc_encode_batch_device_compact_int(enc._h, at(d_int, b.off), fmt, bits, C.byref(lay),
                                                             C.c_void_p(arena.data_ptr()), offered, C.c_void_p(cursor.data_ptr()), ent)
            assert rc == 0, (which, E.err(enc))
        enc.synchronize()
        assert lib.glc_ctx_resident_stream(enc._h) == 0
        sides.append((arena, entries, cursor))
    assert torch.equal(d_int.cpu(), torch.from_numpy(b.flat))               # the input is unchanged
    return sides


def same_store(E, sides, what):
    (a0, e0, c0), (a1, e1, c1) = sides
    torch = E.torch
    print(f"{what}: cursor {int(c0.item())}, stored {e0[:, 3].cpu().tolist()}")
    assert torch.equal(e0, e1), (what, e0.cpu().tolist(), e1.cpu().tolist())
    assert int(c0.item()) == int(c1.item()), what
    if not torch.equal(a0, a1):
        bad = torch.nonzero(a0 != a1).reshape(-1)
        raise AssertionError(f"{what}: {bad.numel()} arena bytes differ, first at {int(bad[0])}")
    return e0.cpu().numpy()


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", SI.CHANNELS)
def test_encode_to_store_equals_the_float_call_on_widened_clips(E, ch, planar):
    """Every format at every slice offset: six clip lengths in one batch with odd strides, so the clips (and, planar,
    their planes) start at every residue of a vector of four samples."""
    for fmt, bits in SI.FORMATS:
        clips = family(E, fmt, bits, ch)
        for off in range(4):
            b = SI.input_batch(clips, ch, planar, off, SI.np_dtype(fmt))
            residues = {int(ix[0]) % 4 for ix in b.index}
            assert len(residues) == 4
            ent = same_store(E, store_both(E, b, fmt, bits, cursor0=(7, 0, 64, 130)[off]), f"ch{ch} fmt{fmt}/{bits} off{off}")
            assert ((ent[:, 3] >> 32) == 1).all() and (ent[:, 1] > 0).all()


def test_appending_twice_and_a_cut_arena(E):
    fmt, bits, ch = S16, 16, 2
    clips = SI.family_clips(fmt, bits, ch)
    b = SI.input_batch(clips, ch, True, 1, np.int16)
    ent = same_store(E, store_both(E, b, fmt, bits, cursor0=5, calls=2), "appended twice")
    n = b.n_clips
    assert (ent[n:, 0] > ent[:n, 0].max()).all() and np.array_equal(ent[:n, 1:], ent[n:, 1:])
    # an arena that ends inside clip 3: clips 3.. are not stored, the cursor counts on
    cut = int(ent[3, 0] + ent[3, 1] // 2)
    ent2 = same_store(E, store_both(E, b, fmt, bits, cursor0=5, arena_bytes=cut), "cut inside clip 3")
    assert ((ent2[:, 3] >> 32).tolist()) == [1, 1, 1, 0, 0, 0]
    assert np.array_equal(ent2[:, :2], ent[:n, :2])


def _long_clips(n_clips, frames, ch, seed):
    """Clips of about `frames` frames, cheap to make: two tones per channel, a hop of noise in front, the specials at
    both ends."""
    rng = np.random.default_rng(seed)
    n = frames * HOP
    t = np.arange(n, dtype=np.float64)
    base = np.stack([0.3 * np.sin(2 * np.pi * (440.0 + 97 * c) / SR * t) + 0.1 * np.sin(2 * np.pi * (1234.5 + 31 * c) / SR * t)
                     for c in range(ch)], 1)
    base = np.rint(base * 32768.0).astype(np.int16)
    clips = []
    for i in range(n_clips):
        x = np.roll(base, 977 * i, axis=0)[:n - 37 * i].copy()
        x[:HOP] = rng.integers(-20000, 20000, (HOP, ch))
        x[0, :2], x[-1, :2] = (-32768, 32767), (1, -1)
        clips.append(x)
    return clips


@pytest.mark.parametrize("case", ("two-rounds", "staged-whole"))
def test_encode_to_store_over_more_than_a_round(E, case):
    ch = 2
    clips = _long_clips(5, 1000, ch, 1) if case == "two-rounds" else _long_clips(1, 4097, ch, 2)
    if case == "staged-whole":
        assert -(-(512 + clips[0].shape[0]) // HOP) - 1 == 4097
    b = SI.input_batch(clips, ch, case == "two-rounds", 3, np.int16)
    ent = same_store(E, store_both(E, b, S16, 16), case)
    assert ((ent[:, 3] >> 32) == 1).all()


@pytest.mark.parametrize("fmt,bits,ch,planar", [(S16, 12, 2, True), (S32, 32, 3, False)])
def test_stored_blobs_are_the_oracle_streams_of_the_widened_integers(E, fmt, bits, ch, planar):
    g = E.g
    fam = family(E, fmt, bits, ch)
    clips = [fam[2], fam[5]]                        # 1024 samples (the oracle compresses it) and 2049 (raw frames)
    b = SI.input_batch(clips, ch, planar, 1, SI.np_dtype(fmt))
    enc = E.ctx("enc-int")
    d_int = E.dev(b.flat)
    lay, _keep = E.layout(b)
    arena = E.torch.zeros(int(E.lib.glc_compact_store_bound(C.byref(lay))), dtype=E.torch.uint8, device="cuda")
    cursor = E.torch.zeros(1, dtype=E.torch.int64, device="cuda")
    entries = E.torch.zeros((b.n_clips, 4), dtype=E.torch.int64, device="cuda")
    rc = E.lib.glc_encode_batch_device_compact_int(enc._h, at(d_int, b.off), fmt, bits, C.byref(lay), C.c_void_p(arena.data_ptr()),
                                                   arena.numel(), C.c_void_p(cursor.data_ptr()), C.c_void_p(entries.data_ptr()))
    assert rc == 0, E.err(enc)
    enc.synchronize()
    host, ent = arena.cpu().numpy(), entries.cpu().tolist()
    raw = comp = 0
    for i, clip in enumerate(clips):
        blob = host[ent[i][0]:ent[i][0] + ent[i][1]]
        data = g.EncodedAudio.from_compact(SR, clip.size, ch, [blob]).to_bytes()
        ref = O.encode(SI.widen(clip.reshape(-1), bits), SR, ch, taps=True)
        assert data == ref.glc, f"clip {i}"
        raw, comp = raw + int(ref.is_raw.sum()), comp + int((ref.is_raw == 0).sum())
    assert raw and comp


# ------------------------------------------------------------------------------------------ round trip

def roundtrip(E, which, d_in, in_off, fmt, bits, lin, d_out, out_off, out_fmt, lout):
    rt = E.ctx("rt-" + which)
    if which == "f32":
        rc = E.lib.glc_roundtrip_batch_device(rt._h, at(d_in, in_off), C.byref(lin), at(d_out, out_off), C.byref(lout))
    else:
        rc = E.lib.glc_roundtrip_batch_device_pcm(rt._h, at(d_in, in_off), fmt, bits, C.byref(lin), at(d_out, out_off), out_fmt, C.byref(lout))
    assert rc == 0, (which, E.err(rt))
    rt.synchronize()
    assert E.lib.glc_ctx_resident_stream(rt._h) == 0
    return rt


@pytest.mark.parametrize("in_planar", (True, False), ids=("planar-to-interleaved", "interleaved-to-planar"))
@pytest.mark.parametrize("ch", (1, 2, 3, 6))
@pytest.mark.parametrize("fmt,bits,out_fmt", [(S16, 16, PF32), (S16, 12, S16), (S32, 32, S16), (PF32, 32, S16)],
                         ids=("s16-f32", "s16-s16", "s32-s16", "f32-s16"))
def test_roundtrip_pcm(E, fmt, bits, out_fmt, ch, in_planar):
    torch = E.torch
    ifmt, ibits = (S16, 16) if fmt == PF32 else (fmt, bits)
    clips = family(E, ifmt, ibits, ch)
    in_off, out_off = (1 + ch) % 4, (2 + ch) % 4
    b = SI.input_batch(clips, ch, in_planar, in_off, SI.np_dtype(ifmt))
    d_int = E.dev(b.flat)
    d_f = widened_twin(E, b, d_int, ifmt, ibits)
    lin, _k1 = E.layout(b)
    of = SI.output_batch(b.lengths, ch, not in_planar, out_off, np.float32, pad=7)
    lout, _k2 = E.layout(of)
    # the yardstick: the float call on the widened twin
    ref = E.dev(of.flat)
    rt_f = roundtrip(E, "f32", d_f, in_off, PF32, 32, lin, ref, out_off, PF32, lout)
    rc_f, info_f = E.batch_info(rt_f, b.n_clips)
    ref = ref.cpu().numpy()
    assert (ref.view(np.uint32)[~of.mask] == NAN_BITS).all() and not (ref.view(np.uint32)[of.mask] == NAN_BITS).any()
    # the call under test
    src = d_f if fmt == PF32 else d_int
    if out_fmt == S16:
        oi = SI.output_batch(b.lengths, ch, not in_planar, out_off, np.int16, pad=7)
        assert np.array_equal(oi.mask, of.mask)
        got = E.dev(oi.flat)
        want = np.where(of.mask, SI.narrow(ref), oi.flat)
    else:
        got = E.dev(of.flat)
        want = ref
    rt_i = roundtrip(E, "pcm", src, in_off, fmt, bits, lin, got, out_off, out_fmt, lout)
    rc_i, info_i = E.batch_info(rt_i, b.n_clips)
    got = got.cpu().numpy()
    view = np.uint16 if out_fmt == S16 else np.uint32
    bad = np.flatnonzero(got.view(view) != want.view(view))
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[0]} (true sample: {bool(of.mask[bad[0]])})"
    assert rc_f == 0 and rc_i == 0 and info_i == info_f
    if out_fmt == S16:
        q = got[of.mask]
        assert (q != 0).any()


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_roundtrip_in_place_s16(E, planar):
    ch, fmt, bits = 2, S16, 16
    clips = SI.family_clips(fmt, bits, ch)
    b = SI.input_batch(clips, ch, planar, 3, np.int16)
    d_int = E.dev(b.flat)
    d_f = widened_twin(E, b, d_int, fmt, bits)
    lay, _k = E.layout(b)
    of = SI.output_batch(b.lengths, ch, planar, 3, np.float32)
    assert np.array_equal(of.mask, b.mask)
    ref = E.dev(of.flat)
    roundtrip(E, "f32", d_f, 3, PF32, 32, lay, ref, 3, PF32, lay)
    want = np.where(b.mask, SI.narrow(ref.cpu().numpy()), b.flat)              # the filler between the clips stays
    roundtrip(E, "pcm", d_int, 3, fmt, bits, lay, d_int, 3, S16, lay)
    assert np.array_equal(d_int.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------ decode, crops and draw as i16

STORE_LENGTHS = (2049, 1539)


def store_of(E, ch):
    """Two loud clips per channel count in a store the float encoder filled -> dict(arena, entries, lengths, blobs)."""
    key = ("store", ch)
    if key not in E.cache:
        torch = E.torch
        lens = list(STORE_LENGTHS)
        x = np.zeros((len(lens), ch, max(lens)), F32)
        for i, n in enumerate(lens):
            x[i, :, :n] = SI.loud_clip(ch, n, i).T
        arena, cursor, entries = E.ctx("enc-f32").encode_compact_batch_tensor(torch.from_numpy(x).cuda(), lengths=lens, planar=True)
        ent = entries.cpu().tolist()
        assert all(e[3] >> 32 == 1 for e in ent)
        E.cache[key] = dict(arena=arena, entries=entries, ent=ent, lens=lens,
                            lengths=torch.tensor(lens, dtype=torch.int64, device="cuda"))
    return E.cache[key]


def narrowed_pair(E, ch, lengths, planar, off, call_f32, call_i16, dec=None, n_status=None):
    """One float call and one _i16 call into buffers of the same element layout: every element of the int16 buffer is
    narrow(float output) on the crops and the sentinel elsewhere; the status words are the float call's."""
    dec = dec or E.ctx("dec", ch)
    of = SI.output_batch(lengths, ch, planar, off, np.float32)
    oi = SI.output_batch(lengths, ch, planar, off, np.int16)
    lay, _k = E.layout(of)
    d_f, d_i = E.dev(of.flat), E.dev(oi.flat)
    n = len(lengths) if n_status is None else n_status
    rc = call_f32(dec, at(d_f, off), lay)
    assert rc == 0, E.err(dec)
    rc_sf, st_f = E.status(dec, n)
    rc = call_i16(dec, at(d_i, off), lay)
    assert rc == 0, E.err(dec)
    assert E.lib.glc_ctx_resident_stream(dec._h) == 0
    rc_si, st_i = E.status(dec, n)
    ref, got = d_f.cpu().numpy(), d_i.cpu().numpy()
    assert (ref.view(np.uint32)[~of.mask] == NAN_BITS).all()
    want = np.where(of.mask, SI.narrow(ref), oi.flat)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[0]}: {got[bad[0]]} for {want[bad[0]]} (a crop's sample: {bool(of.mask[bad[0]])})"
    assert rc_sf == 0 and rc_si == 0 and st_i == st_f
    return ref[of.mask], got[of.mask], st_i


def blob_args(E, blobs, n_samples):
    b = len(blobs)
    ptrs = (C.c_void_p * b)(*[p for p, _ in blobs])
    sizes = (C.c_uint64 * b)(*[s for _, s in blobs])
    ns = (C.c_uint64 * b)(*n_samples)
    return ptrs, sizes, ns


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", (1, 2, 3, 6))
def test_whole_clips_and_crops_as_i16(E, ch, planar):
    lib = E.lib
    s = store_of(E, ch)
    base = s["arena"].data_ptr()
    blobs = [(base + e[0], e[1]) for e in s["ent"]]
    ptrs, sizes, ns = blob_args(E, blobs, [n * ch for n in s["lens"]])
    rails = set()
    for off in range(4):
        ref, got, st = narrowed_pair(
            E, ch, s["lens"], planar, off,
            lambda d, p, lay: lib.glc_decode_batch_device_compact(d._h, ptrs, sizes, ns, p, C.byref(lay)),
            lambda d, p, lay: lib.glc_decode_batch_device_compact_i16(d._h, ptrs, sizes, ns, p, C.byref(lay)))
        assert all(w == (0, 0, 0) for w in st)
        rails |= {int(got.max()), int(got.min())}
        assert ((got > -32768) & (got < 32767) & (got != 0)).any()
    assert rails >= {32767, -32768}                                           # the narrowing clamps at both rails here
    # crops: every length at every start of both clips, in one call per output offset
    sel = [(i, st_, L) for i, n in enumerate(s["lens"]) for st_, L in SI.crop_set(n)]
    cptrs, csizes, cns = blob_args(E, [blobs[i] for i, _, _ in sel], [s["lens"][i] * ch for i, _, _ in sel])
    crops = (E.L.GlcCrop * len(sel))(*[E.L.GlcCrop(a, L) for _, a, L in sel])
    for off in range(4):
        narrowed_pair(
            E, ch, [L for _, _, L in sel], planar, off,
            lambda d, p, lay: lib.glc_decode_crops_device_compact(d._h, cptrs, csizes, cns, crops, p, C.byref(lay)),
            lambda d, p, lay: lib.glc_decode_crops_device_compact_i16(d._h, cptrs, csizes, cns, crops, p, C.byref(lay)))


def draw_calls(E, arena, arena_bytes, entries, lengths, n_entries, max_length, clips_t, starts_t, L):
    lib = E.lib
    args = (C.c_void_p(arena.data_ptr()), arena_bytes, C.c_void_p(entries.data_ptr()), C.c_void_p(lengths.data_ptr()), n_entries, max_length,
            C.c_void_p(clips_t.data_ptr()), C.c_void_p(starts_t.data_ptr()), L)
    return (lambda d, p, lay: lib.glc_decode_crops_device_store(d._h, *args, p, C.byref(lay)),
            lambda d, p, lay: lib.glc_decode_crops_device_store_i16(d._h, *args, p, C.byref(lay)))


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", (1, 2, 3, 6))
def test_store_draw_as_i16(E, ch, planar):
    """Per crop length the five starts of both clips, with an unusable entry and an unusable selection among them; a
    crop that needs fewer hops than its slot leaves null descriptors behind it."""
    torch = E.torch
    s = store_of(E, ch)
    # entry 2: a copy of entry 0 marked not stored (64 | 1)
    ent = s["ent"] + [SD.entry(s["ent"][0][0], s["ent"][0][1], stored=0)]
    entries = torch.tensor(ent, dtype=torch.int64, device="cuda")
    lens = s["lens"] + [s["lens"][0]]
    lengths = torch.tensor(lens, dtype=torch.int64, device="cuda")
    fewer = 0
    for k, L in enumerate((1, 2, 3, 4, 5, 1023, 1024, 1025)):
        sel = [(i, st_) for i in (0, 1) for st_ in (0, 511, 512, 513, lens[i] - L)]
        sel.insert(3, (2, 0))                       # not stored
        sel.insert(7, (5, 0))                       # no such clip
        sel.insert(9, (1, lens[1] - L + 1))         # ends behind the clip
        clips_t = torch.tensor([c for c, _ in sel], dtype=torch.int64, device="cuda")
        starts_t = torch.tensor([a for _, a in sel], dtype=torch.int64, device="cuda")
        f32, i16 = draw_calls(E, s["arena"], s["arena"].numel(), entries, lengths, len(ent), max(lens), clips_t, starts_t, L)
        ref, got, st = narrowed_pair(E, ch, [L] * len(sel), planar, k % 4, f32, i16)
        flags = [w[0] for w in st]
        assert flags[3] == 64 | 1 and flags[7] == 128 | 1 and flags[9] == 128 | 1
        assert all(f == 0 for j, f in enumerate(flags) if j not in (3, 7, 9))
        per = L * ch
        got = got.reshape(len(sel), per)
        assert not got[3].any() and not got[7].any() and not got[9].any()     # 0 over an unusable crop's samples
        max_hops = SD.slots(L, ch)[0]
        plan = [E.g.plan_crop(lens[c] * ch, ch, a, L).n_hops for j, (c, a) in enumerate(sel) if j not in (3, 7, 9)]
        fewer += sum(h < max_hops for h in plan)
    assert fewer                                                              # null descriptors were among them


def test_more_than_one_round_of_crops(E):
    torch, lib = E.torch, E.lib
    ch, L = 1, 1025
    s = store_of(E, ch)
    n = 1100
    assert n > SD.per_round(L, ch)
    rng = np.random.default_rng(4)
    which = rng.integers(0, 2, n)
    starts = np.array([rng.integers(0, s["lens"][c] - L + 1) for c in which])
    base = s["arena"].data_ptr()
    ptrs, sizes, ns = blob_args(E, [(base + s["ent"][c][0], s["ent"][c][1]) for c in which], [s["lens"][c] * ch for c in which])
    crops = (E.L.GlcCrop * n)(*[E.L.GlcCrop(int(a), L) for a in starts])
    narrowed_pair(E, ch, [L] * n, True, 1,
                  lambda d, p, lay: lib.glc_decode_crops_device_compact(d._h, ptrs, sizes, ns, crops, p, C.byref(lay)),
                  lambda d, p, lay: lib.glc_decode_crops_device_compact_i16(d._h, ptrs, sizes, ns, crops, p, C.byref(lay)))
    clips_t = torch.from_numpy(which.astype(np.int64)).cuda()
    starts_t = torch.from_numpy(starts.astype(np.int64)).cuda()
    f32, i16 = draw_calls(E, s["arena"], s["arena"].numel(), s["entries"], s["lengths"], 2, max(s["lens"]), clips_t, starts_t, L)
    narrowed_pair(E, ch, [L] * n, True, 3, f32, i16)


def damaged_blobs():
    """(name, channels, buffer, bytes, the flag the device check must raise or 0) - compact_decode_cases' builders."""
    rng = np.random.RandomState(3)
    ext = K.Row(np.array([0, 1, 511, 1022, 1023], np.uint16), np.array([-32768, 32767, -32768, 32767, -1], np.int16))
    inf = K.Row(np.array([5, 700], np.uint16), np.array([100, -100], np.int16), 0x7F800000)
    zero_q = K.Row(np.array([9], np.uint16), np.array([0], np.int16), 0x7F800000)      # a stored zero times inf: NaN
    frames = [("c", [ext, inf]), ("c", [zero_q, ext]), ("c", [K.row(rng, 3), K.row(rng, 4)])]
    plain = [("c", [K.row(rng, 20), K.row(rng, 5)]), ("raw", K.raw_planes(rng, 2)), ("c", [K.row(rng, 7), K.row(rng, 0)])]
    out = [("inf-scale-over-a-stored-zero", 2, *K.pack(2, frames), 0),
           ("bad-magic", 2, *K.pack(2, plain, magic=0x12345678), K.BAD_HEADER),
           ("pair-sum", 2, *K.pack(2, plain, n_pairs=31), K.PAIR_SUM),
           ("row-longer-than-the-pairs", 2, *K.pack(2, plain, cnt_set={0: 1000}), K.ROW_BOUNDS)]
    return out


def test_damaged_blobs_narrow_as_the_float_call_decodes_them(E):
    torch, lib = E.torch, E.lib
    ch = 2
    cases = damaged_blobs()
    nf = 3
    n_samples = K.n_samples_of(ch, nf)
    length = n_samples // ch
    # a host-made store: the blobs back to back, 64-byte aligned
    parts, ent, off = [], [], 0
    for name, _, buf, nbytes, _ in cases:
        cap = K.align64(nbytes)
        parts.append(np.ascontiguousarray(buf[:cap]) if buf.size >= cap else np.concatenate([buf, np.zeros(cap - buf.size, np.uint8)]))
        ent.append(SD.entry(off, cap))
        off += cap
    arena = E.dev(np.concatenate(parts))
    assert arena.data_ptr() % 64 == 0
    base = arena.data_ptr()
    blobs = [(base + e[0], e[1]) for e in ent]
    ptrs, sizes, ns = blob_args(E, blobs, [n_samples] * len(cases))
    for planar in (True, False):
        ref, got, st = narrowed_pair(
            E, ch, [length] * len(cases), planar, 1,
            lambda d, p, lay: lib.glc_decode_batch_device_compact(d._h, ptrs, sizes, ns, p, C.byref(lay)),
            lambda d, p, lay: lib.glc_decode_batch_device_compact_i16(d._h, ptrs, sizes, ns, p, C.byref(lay)))
        for (name, _, _, _, flag), w in zip(cases, st):
            assert (w[0] != 0) == (flag != 0) and (flag or w == (0, 0, 0)), (name, w)
        first = ref[:n_samples]                                               # the inf-scale clip
        print(f"inf-scale clip: {int(np.isnan(first).sum())} NaN, {int(np.isposinf(first).sum())} +inf, {int(np.isneginf(first).sum())} -inf")
        assert np.isnan(first).any() and np.isposinf(first).any() and np.isneginf(first).any()
        q = got[:n_samples]
        assert (q[np.isnan(first)] == 0).all() and (q[np.isposinf(first)] == 32767).all() and (q[np.isneginf(first)] == -32768).all()
    L = 1500
    crops = (E.L.GlcCrop * len(cases))(*[E.L.GlcCrop(700, L) for _ in cases])
    narrowed_pair(E, ch, [L] * len(cases), True, 2,
                  lambda d, p, lay: lib.glc_decode_crops_device_compact(d._h, ptrs, sizes, ns, crops, p, C.byref(lay)),
                  lambda d, p, lay: lib.glc_decode_crops_device_compact_i16(d._h, ptrs, sizes, ns, crops, p, C.byref(lay)))
    entries = torch.tensor(ent, dtype=torch.int64, device="cuda")
    lengths = torch.tensor([length] * len(cases), dtype=torch.int64, device="cuda")
    clips_t = torch.arange(len(cases), dtype=torch.int64, device="cuda")
    starts_t = torch.full((len(cases),), 700, dtype=torch.int64, device="cuda")
    f32, i16 = draw_calls(E, arena, arena.numel(), entries, lengths, len(cases), length, clips_t, starts_t, L)
    narrowed_pair(E, ch, [L] * len(cases), False, 3, f32, i16)


# ------------------------------------------------------------------------------------------ refusals

def test_refusals_leave_everything_untouched(E):
    torch, lib = E.torch, E.lib
    ch = 2
    clips = SI.family_clips(S16, 16, ch, (1025, 513))
    b = SI.input_batch(clips, ch, True, 0, np.int16)
    lay, _k = E.layout(b)
    d_int = E.dev(b.flat)
    d_i32 = E.dev(b.flat.astype(np.int32))
    image = pattern(1 << 16)
    arena = E.dev(image)
    cursor = torch.tensor([64], dtype=torch.int64, device="cuda")
    entries = torch.full((b.n_clips, 4), -1, dtype=torch.int64, device="cuda")
    oi = SI.output_batch(b.lengths, ch, True, 0, np.int16)
    d_out = E.dev(np.concatenate([oi.flat, oi.flat]))                      # room for a float output too
    enc, rt, dec = E.ctx("enc-int"), E.ctx("rt-pcm"), E.ctx("dec", ch)

    def encode(p, fmt, bits, arena_p=None):
        return lib.glc_encode_batch_device_compact_int(enc._h, p, fmt, bits, C.byref(lay), arena_p or C.c_void_p(arena.data_ptr()), arena.numel(),
                                                       C.c_void_p(cursor.data_ptr()), C.c_void_p(entries.data_ptr()))

    def trip(p, fmt, bits, out_p, out_fmt):
        return lib.glc_roundtrip_batch_device_pcm(rt._h, p, fmt, bits, C.byref(lay), out_p, out_fmt, C.byref(lay))

    p16, p32 = at(d_int, 0), at(d_i32, 0)
    assert encode(p16, 0, 16) == EINVAL and encode(p16, 4, 16) == EINVAL                         # bad fmt
    assert encode(p16, S16, 0) == EINVAL and encode(p16, S16, 17) == EINVAL                      # bad bits
    assert encode(p32, S32, 33) == EINVAL and encode(p32, S32, 0) == EINVAL
    assert b"bits" in E.err(enc)
    assert encode(C.c_void_p(d_int.data_ptr() + 1), S16, 16) == EINVAL                           # misaligned for its sample size
    assert encode(C.c_void_p(d_i32.data_ptr() + 2), S32, 32) == EINVAL
    assert b"aligned" in E.err(enc)
    out = at(d_out, 0)
    assert trip(p16, 0, 16, out, S16) == EINVAL and trip(p16, S16, 17, out, S16) == EINVAL and trip(p32, S32, 33, out, S16) == EINVAL
    assert trip(p16, S16, 0, out, PF32) == EINVAL
    assert trip(p16, S16, 16, out, S32) == EINVAL and trip(p16, S16, 16, out, 0) == EINVAL        # out_fmt
    assert b"GLC_PCM_F32 or GLC_PCM_S16" in E.err(rt)
    assert trip(C.c_void_p(d_int.data_ptr() + 1), S16, 16, out, S16) == EINVAL
    assert trip(p16, S16, 16, C.c_void_p(d_out.data_ptr() + 1), S16) == EINVAL                   # odd d_out
    assert trip(p16, S16, 16, C.c_void_p(d_out.data_ptr() + 2), PF32) == EINVAL                  # a float output on a 2-byte address
    # different widths on overlapping bytes: the same pointer and layout, S32 in and S16 out; S16 in and F32 out
    assert trip(p32, S32, 32, p32, S16) == EINVAL
    assert b"overlap" in E.err(rt)
    assert trip(p16, S16, 16, p16, PF32) == EINVAL
    # ... and a byte extent the element count would not have shown: the S32 input's second half under an S16 output
    ext16 = 2 * ((b.n_clips - 1) * b.clip_stride + (ch - 1) * b.channel_stride + max(b.lengths))
    assert trip(p32, S32, 32, C.c_void_p(d_i32.data_ptr() + ext16 + 2), S16) == EINVAL
    assert trip(p16, S16, 16, C.c_void_p(d_int.data_ptr() + 2), S16) == EINVAL                   # the same format, shifted: not in place
    # the _i16 decodes: odd d_out, and an output extent that overlaps the arena by its last byte only
    s = store_of(E, ch)
    base = s["arena"].data_ptr()
    ptrs, sizes, ns = blob_args(E, [(base + e[0], e[1]) for e in s["ent"]], [n * ch for n in s["lens"]])
    ob = SI.output_batch(s["lens"], ch, True, 0, np.int16)
    olay, _k2 = E.layout(ob)
    d_o = E.dev(ob.flat)
    odd = C.c_void_p(d_o.data_ptr() + 1)
    crops = (E.L.GlcCrop * 2)(E.L.GlcCrop(0, s["lens"][0]), E.L.GlcCrop(0, s["lens"][1]))
    assert lib.glc_decode_batch_device_compact_i16(dec._h, ptrs, sizes, ns, odd, C.byref(olay)) == EINVAL
    assert lib.glc_decode_crops_device_compact_i16(dec._h, ptrs, sizes, ns, crops, odd, C.byref(olay)) == EINVAL
    extent = 2 * ((ob.n_clips - 1) * ob.clip_stride + (ch - 1) * ob.channel_stride + max(ob.lengths))   # bytes of the int16 extent
    # the last element of the extent is the first of blob 0 (nothing is queued, the address is only compared)
    blob0 = base + s["ent"][0][0]
    assert lib.glc_decode_batch_device_compact_i16(dec._h, ptrs, sizes, ns, C.c_void_p(blob0 - extent + 2), C.byref(olay)) == EINVAL
    assert b"overlaps the blob" in E.err(dec)
    # the draw: an arena of an odd number of bytes whose LAST byte is the first byte of the output extent, and an
    # extent whose last element is the arena's first two bytes
    L = 1025
    dl = SI.output_batch([L, L], ch, True, 0, np.int16)
    dlay, _k3 = E.layout(dl)
    dext = 2 * (dl.clip_stride + (ch - 1) * dl.channel_stride + L)
    clips_t = torch.zeros(2, dtype=torch.int64, device="cuda")
    starts_t = torch.zeros(2, dtype=torch.int64, device="cuda")
    big = torch.from_numpy(np.full(1 << 20, SI.SENTINEL, np.uint16).view(np.int16).copy()).cuda()
    a0 = (big.data_ptr() + (1 << 19) + 63) & ~63

    def draw(arena_bytes, out_addr):
        return lib.glc_decode_crops_device_store_i16(dec._h, C.c_void_p(a0), arena_bytes, C.c_void_p(s["entries"].data_ptr()),
                                                     C.c_void_p(s["lengths"].data_ptr()), 2, max(s["lens"]), C.c_void_p(clips_t.data_ptr()),
                                                     C.c_void_p(starts_t.data_ptr()), L, C.c_void_p(out_addr), C.byref(dlay))

    assert draw(4095, a0 + 4094) == EINVAL
    assert b"overlaps the arena" in E.err(dec)
    assert draw(4096, a0 - dext + 2) == EINVAL
    assert b"overlaps the arena" in E.err(dec)
    assert draw(4096, a0 + 4097) == EINVAL                                                     # odd d_out
    assert b"aligned" in E.err(dec)
    for c in (enc, rt, dec):
        c.synchronize()
    # nothing was queued: every buffer is as it was
    assert np.array_equal(arena.cpu().numpy(), image) and int(cursor.item()) == 64 and (entries.cpu().numpy() == -1).all()
    assert np.array_equal(d_int.cpu().numpy(), b.flat) and np.array_equal(d_i32.cpu().numpy(), b.flat.astype(np.int32))
    assert (d_out.cpu().numpy().view(np.uint16) == SI.SENTINEL).all() and (d_o.cpu().numpy().view(np.uint16) == SI.SENTINEL).all()
    assert (big.cpu().numpy().view(np.uint16) == SI.SENTINEL).all()
    # bytes, not elements: an int16 extent that ends where the arena begins is accepted and drawn; the float extent
    # of the same element count from the same address runs into the arena and is refused
    room = (dext + 4 + 63) // 64 * 64
    both = torch.zeros(room + s["arena"].numel(), dtype=torch.uint8, device="cuda")
    both[room:] = s["arena"]
    a1 = both.data_ptr() + room
    assert a1 % 64 == 0
    out_addr = a1 - dext - dext % 4
    args = (C.c_void_p(a1), s["arena"].numel(), C.c_void_p(s["entries"].data_ptr()), C.c_void_p(s["lengths"].data_ptr()), 2, max(s["lens"]),
            C.c_void_p(clips_t.data_ptr()), C.c_void_p(starts_t.data_ptr()), L)
    assert lib.glc_decode_crops_device_store(dec._h, *args, C.c_void_p(out_addr), C.byref(dlay)) == EINVAL
    assert b"overlaps the arena" in E.err(dec)
    assert lib.glc_decode_crops_device_store_i16(dec._h, *args, C.c_void_p(out_addr), C.byref(dlay)) == 0, E.err(dec)
    dec.synchronize()
    assert torch.equal(both[room:], s["arena"])
    got = both[out_addr - both.data_ptr():room].cpu().numpy().view(np.int16)
    f32, i16 = draw_calls(E, s["arena"], s["arena"].numel(), s["entries"], s["lengths"], 2, max(s["lens"]), clips_t, starts_t, L)
    ref, _, _ = narrowed_pair(E, ch, [L, L], True, 0, f32, i16)
    assert np.array_equal(got[:dext // 2][dl.mask[:dext // 2]], SI.narrow(ref))


# ------------------------------------------------------------------------------------------ context

def test_the_new_calls_leave_the_context_as_their_float_twins_do(E):
    """The same sequence on two contexts, float calls on one and the integer twins on the other, interleaved with
    glc_decode of a stream that becomes resident: after every step both report the same."""
    torch, lib, g = E.torch, E.lib, E.g
    ch = 2
    s = store_of(E, ch)
    x = SI.loud_clip(ch, 3000, 5).reshape(-1) * F32(0.3)
    stream = g.Encoder(SR).encode(x, ch)
    base = s["arena"].data_ptr()
    ptrs, sizes, ns = blob_args(E, [(base + e[0], e[1]) for e in s["ent"]], [n * ch for n in s["lens"]])
    clips = SI.family_clips(S16, 16, ch, (1025, 513))
    b = SI.input_batch(clips, ch, False, 1, np.int16)
    d_int = E.dev(b.flat)
    d_f = widened_twin(E, b, d_int, S16, 16)
    blay, _k = E.layout(b)
    A, B = g.Decoder(ch, SR), g.Decoder(ch, SR)                               # float twins on A, the new calls on B
    of, oi = SI.output_batch(s["lens"], ch, True, 0, np.float32), SI.output_batch(s["lens"], ch, True, 0, np.int16)
    olay, _k2 = E.layout(of)
    out_f, out_i = E.dev(of.flat), E.dev(oi.flat)
    rf, ri = SI.output_batch(b.lengths, ch, True, 0, np.float32), SI.output_batch(b.lengths, ch, True, 0, np.int16)
    rlay, _k3 = E.layout(rf)
    rt_f, rt_i = E.dev(rf.flat), E.dev(ri.flat)
    arena_a, arena_b = (torch.zeros(1 << 18, dtype=torch.uint8, device="cuda") for _ in range(2))
    cur_a, cur_b = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    ent_a, ent_b = (torch.zeros((2, 4), dtype=torch.int64, device="cuda") for _ in range(2))
    clips_t = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    starts_t = torch.tensor([3, 500], dtype=torch.int64, device="cuda")
    dl_f, dl_i = SI.output_batch([700, 700], ch, False, 0, np.float32), SI.output_batch([700, 700], ch, False, 0, np.int16)
    dlay, _k4 = E.layout(dl_f)
    dr_f, dr_i = E.dev(dl_f.flat), E.dev(dl_i.flat)
    f32_draw, i16_draw = draw_calls(E, s["arena"], s["arena"].numel(), s["entries"], s["lengths"], 2, max(s["lens"]), clips_t, starts_t, 700)

    def state(d):
        d.synchronize()
        return (lib.glc_ctx_resident_stream(d._h) != 0, E.status(d, 2), E.batch_info(d, 2))

    def resident(d):
        y = d.decode(stream)
        assert lib.glc_ctx_resident_stream(d._h) == stream.stream_id != 0
        return y

    steps = [
        ("decode",) * 2,
        (lambda: lib.glc_decode_batch_device_compact(A._h, ptrs, sizes, ns, at(out_f, 0), C.byref(olay)),
         lambda: lib.glc_decode_batch_device_compact_i16(B._h, ptrs, sizes, ns, at(out_i, 0), C.byref(olay))),
        ("decode",) * 2,
        (lambda: lib.glc_roundtrip_batch_device(A._h, at(d_f, 1), C.byref(blay), at(rt_f, 0), C.byref(rlay)),
         lambda: lib.glc_roundtrip_batch_device_pcm(B._h, at(d_int, 1), S16, 16, C.byref(blay), at(rt_i, 0), S16, C.byref(rlay))),
        ("decode",) * 2,
        (lambda: lib.glc_encode_batch_device_compact(A._h, at(d_f, 1), C.byref(blay), C.c_void_p(arena_a.data_ptr()), arena_a.numel(),
                                                     C.c_void_p(cur_a.data_ptr()), C.c_void_p(ent_a.data_ptr())),
         lambda: lib.glc_encode_batch_device_compact_int(B._h, at(d_int, 1), S16, 16, C.byref(blay), C.c_void_p(arena_b.data_ptr()),
                                                         arena_b.numel(), C.c_void_p(cur_b.data_ptr()), C.c_void_p(ent_b.data_ptr()))),
        ("decode",) * 2,
        (lambda: f32_draw(A, at(dr_f, 0), dlay), lambda: i16_draw(B, at(dr_i, 0), dlay)),
    ]
    first = None
    for k, (fa, fb) in enumerate(steps):
        if fa == "decode":
            ya, yb = resident(A), resident(B)
            assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
            first = ya if first is None else first
            assert np.array_equal(ya.view(np.uint32), first.view(np.uint32))   # the decode between them is not disturbed
            continue
        assert fa() == 0, (k, E.err(A))
        assert fb() == 0, (k, E.err(B))
        sa, sb = state(A), state(B)
        assert sa == sb, (k, sa, sb)
        assert sb[0] is False                                                 # no stream is resident after a call of the family
    assert torch.equal(arena_a, arena_b) and torch.equal(ent_a, ent_b) and int(cur_a.item()) == int(cur_b.item())
    for f, i, m in ((out_f, out_i, of.mask), (rt_f, rt_i, rf.mask), (dr_f, dr_i, dl_f.mask)):
        f, i = f.cpu().numpy(), i.cpu().numpy()
        assert np.array_equal(i[m], SI.narrow(f[m])) and (i[~m].view(np.uint16) == SI.SENTINEL).all()


# ------------------------------------------------------------------------------------------ the Python arguments

def test_tensor_methods_take_integer_tensors_and_int16_outputs(E):
    torch, g = E.torch, E.g
    ch = 2
    clips = SI.family_clips(S16, 12, ch, (1025, 2049))
    lens = [c.shape[0] for c in clips]
    x = np.zeros((2, ch, 2049), np.int16)
    for i, c in enumerate(clips):
        x[i, :, :lens[i]] = c.T
    xi = torch.from_numpy(x).cuda()
    xf = torch.from_numpy(SI.widen(x, 12)).cuda()
    enc, rt, dec = E.ctx("enc-int"), E.ctx("rt-pcm"), E.ctx("dec", ch)
    a0, c0, e0 = enc.encode_compact_batch_tensor(xf, lengths=lens)
    a1, c1, e1 = enc.encode_compact_batch_tensor(xi, lengths=lens, bits=12)
    assert torch.equal(e0, e1) and torch.equal(c0, c1) and torch.equal(a0[:int(c0.item())], a1[:int(c1.item())])
    with pytest.raises(g.GlcError):
        enc.encode_compact_batch_tensor(xi, lengths=lens, bits=17)
    with pytest.raises(TypeError):
        enc.encode_compact_batch_tensor(xf, lengths=lens, bits=12)
    yf = rt.apply_batch_tensor(xf, lengths=lens)
    yi = rt.apply_batch_tensor(xi, lengths=lens, bits=12, out_dtype=torch.int16)
    assert yi.dtype == torch.int16 and np.array_equal(yi.cpu().numpy(), SI.narrow(yf.cpu().numpy()))
    y2 = rt.apply_batch_tensor(xi, lengths=lens, bits=12)
    assert y2.dtype == torch.float32 and torch.equal(y2.view(torch.int32), yf.view(torch.int32))
    blobs = g.store_blobs(a1, e1)
    ns = [n * ch for n in lens]
    wf = dec.decode_compact_batch_tensor(blobs, ns)
    wi = dec.decode_compact_batch_tensor(blobs, ns, dtype=torch.int16)
    assert wi.dtype == torch.int16 and np.array_equal(wi.cpu().numpy(), SI.narrow(wf.cpu().numpy()))
    out = torch.full((2, ch, 700), SI.SENTINEL, dtype=torch.int16, device="cuda")
    cf = dec.decode_compact_crops_tensor(blobs, ns, [3, 300], 700)
    ci = dec.decode_compact_crops_tensor(blobs, ns, [3, 300], 700, out=out)          # an int16 out selects the format
    assert ci is out and np.array_equal(ci.cpu().numpy(), SI.narrow(cf.cpu().numpy()))
    lengths = torch.tensor(lens, dtype=torch.int64, device="cuda")
    sel = torch.tensor([1, 0, 1], dtype=torch.int64, device="cuda")
    st = torch.tensor([0, 325, 1349], dtype=torch.int64, device="cuda")
    df = dec.decode_store_crops_tensor(a1, e1, lengths, sel, st, 700, 2049, planar=False)
    di = dec.decode_store_crops_tensor(a1, e1, lengths, sel, st, 700, 2049, planar=False, dtype=np.int16)
    assert di.dtype == torch.int16 and np.array_equal(di.cpu().numpy(), SI.narrow(df.cpu().numpy()))
