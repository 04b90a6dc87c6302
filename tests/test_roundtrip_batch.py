"""The batch device round trip: glc_roundtrip_batch_device / RoundTrip.apply_batch_tensor degrade every clip of a
padded, strided batch - interleaved (B, T, C) or planar (B, C, T) - in one call, where the audio sits.

Every comparison is bit for bit - float32 viewed as uint32, tolerance 0.  The CPU oracle per clip
(O.decode(O.encode(x).glc)) is the truth for the small cases; the library's own two-step path (Encoder.encode +
Decoder.decode per clip, which the other suites hold to the oracle) is the expectation for the large ones."""
import ctypes as C

import numpy as np
import pytest

import conftest as cf
import roundtrip_cases as RC
from conftest import O

pytestmark = pytest.mark.gpu

HOP = RC.HOP
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
    if (kind, sr) not in _ctx:
        _ctx[(kind, sr)] = {"rt": lambda: g.RoundTrip(sr), "enc": lambda: g.Encoder(sr), "dec": lambda: g.Decoder(2, sr)}[kind]()
    return _ctx[(kind, sr)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


_oracle = {}


def oracle(key, x, sr, ch):
    """(stream, decoded samples) of the CPU oracle for clip `x`, computed once per key."""
    if key not in _oracle:
        glc = O.encode(x, sr, ch).glc
        _oracle[key] = (glc, O.decode(glc)[0])
    return _oracle[key]


def two_step(g, sr, x, ch):
    enc = ctx(g, "enc", sr).encode(x, ch)
    return enc, ctx(g, "dec", sr).decode(enc).copy()


# ------------------------------------------------------------------------------------------ strided batches

class Batch:
    """Clips (interleaved float32 arrays of `ch` channels) laid out in one NaN-filled buffer: clip i starts `lead`
    + i * clip_stride elements in; planar clips have a plane every channel_stride elements.  Strides default to
    the dense padded tensor of the longest clip."""

    def __init__(self, clips, ch, planar, lead=0, clip_stride=None, channel_stride=None, tail=0):
        self.clips, self.ch, self.planar, self.lead = clips, ch, planar, lead
        self.lens = [c.size // ch for c in clips]
        self.T = max(self.lens)
        self.channel_stride = (channel_stride or self.T) if planar else ch
        dense = (ch - 1) * self.channel_stride + self.T if planar else self.T * ch
        self.clip_stride = clip_stride or dense
        assert self.clip_stride >= dense and self.channel_stride >= (self.T if planar else ch)
        self.size = lead + (len(clips) - 1) * self.clip_stride + dense + tail

    def fill(self, arrays):
        """The buffer's words with `arrays[i]` (interleaved) in clip i's samples and the NaN pattern everywhere else."""
        buf = np.full(self.size, NAN_BITS, np.uint32)
        for i, a in enumerate(arrays):
            a = bits(a).reshape(-1, self.ch)
            assert a.shape[0] == self.lens[i]
            at = self.lead + i * self.clip_stride
            if self.planar:
                for c in range(self.ch):
                    buf[at + c * self.channel_stride: at + c * self.channel_stride + self.lens[i]] = a[:, c]
            else:
                buf[at: at + a.size] = a.reshape(-1)
        return buf

    def tensor(self, torch, words):
        """(storage, strided view of shape (B, C, T) / (B, T, C)) on the device."""
        store = torch.from_numpy(words.view(F32).copy()).cuda()
        shape = (len(self.clips), self.ch, self.T) if self.planar else (len(self.clips), self.T, self.ch)
        return store, store.as_strided(shape, (self.clip_stride, self.channel_stride, 1), self.lead)

    def like(self, planar, **kw):
        return Batch(self.clips, self.ch, planar, **kw)


def run(torch, rt, src, dst, refs, in_place=False):
    """One call from layout `src` to layout `dst`; the WHOLE output buffer must be the references in the clips'
    samples and the untouched NaN pattern in every other word; the input must be unchanged."""
    in_words = src.fill(src.clips)
    if in_place:
        store, x = src.tensor(torch, in_words)
        out_store, out = store, x
    else:
        store, x = src.tensor(torch, in_words)
        out_store, out = dst.tensor(torch, np.full(dst.size, NAN_BITS, np.uint32))
    torch.cuda.synchronize()
    import glc_amd                 # `rt` may be any context class: the call is the C entry point's
    y = glc_amd.RoundTrip.apply_batch_tensor(rt, x, lengths=src.lens, planar=src.planar, out=out, out_planar=dst.planar)
    assert y is out and rt.resident_stream() == 0
    rt.synchronize()
    got = out_store.cpu().numpy().view(np.uint32)
    want = dst.fill(refs)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[0]} of {got.size}"
    if not in_place:
        assert np.array_equal(store.cpu().numpy().view(np.uint32), in_words)


# ------------------------------------------------------------------------------------------ 1 + 8: the oracle, ragged

CASES = RC.oracle_cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault((_c[1], _c[2]), []).append(_c)
GROUPS = {k: v for k, v in GROUPS.items() if len(v) >= 2}
GROUP_IDS = [f"{sr // 1000}k-{ch}ch" for sr, ch in GROUPS]


def test_the_groups_hold_the_edges():
    names = {c[0] for v in GROUPS.values() for c in v}
    for d in ("-1", "+0", "+1"):
        assert f"chord-48k-mono-hop{d}" in names and f"chord-44k-stereo-hop{d}" in names and f"chord-96k-mono-frame-edge{d}" in names
    assert {"shortest-44k-mono", "shortest-96k-6ch", "mixed-48k-stereo", "mixed-44k-mono", "noise-48k-stereo"} <= names
    assert any(len({c[3].size for c in v}) > 1 for v in GROUPS.values())


def check_want(glc, want):
    raw = [f["raw"] is not None for f in cf.parse_glc(glc)["frames"]]
    if want == "tonal":
        assert not any(raw)
    elif want == "noise":
        assert any(raw)
    elif want == "mixed":
        assert any(raw) and not all(raw)
        assert any(raw[i] != raw[i + 1] for i in range(len(raw) - 1))


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_ragged_batch_equals_oracle_per_clip(glc_amd, torch, key, planar):
    sr, ch = key
    group = GROUPS[key]
    refs, streams = [], []
    for name, _, _, x, want in group:
        glc, ref = oracle(name, x, sr, ch)
        check_want(glc, want)
        assert ref.size == x.size
        refs.append(ref), streams.append(glc)
    rt = ctx(glc_amd, "rt", sr)
    b = Batch([c[3] for c in group], ch, planar)
    _, x = b.tensor(torch, b.fill(b.clips))       # the padding behind short clips holds NaNs: it is not read
    torch.cuda.synchronize()
    y = rt.apply_batch_tensor(x, lengths=b.lens, planar=planar)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.device == x.device and y.is_contiguous()
    got = y.cpu().numpy()
    for i, ref in enumerate(refs):
        n = b.lens[i]
        clip = got[i, :, :n].T if planar else got[i, :n, :]
        assert np.array_equal(bits(clip).reshape(-1), bits(ref)), group[i][0]
        pad = got[i, :, n:] if planar else got[i, n:, :]
        assert not bits(pad).any(), "the padding of a new output tensor is zero"
    # 8: per-clip info = the counts of Encoder.encode, the size of the oracle's stream
    infos = rt.last_batch_info()
    assert len(infos) == len(group)
    for (name, _, _, xc, _), glc, got_i in zip(group, streams, infos):
        enc = ctx(glc_amd, "enc", sr).encode(xc, ch)
        i = enc.info()
        assert (got_i.n_frames, got_i.n_raw_frames, got_i.total_nnz) == (i.n_frames, i.n_raw_frames, i.total_nnz), name
        assert got_i.serialized_bytes == glc_amd.lib.glc_serialized_size(enc._h) == len(glc), name


# ------------------------------------------------------------------------------------------ 2: nothing else is written

def small_clips(sr, ch):
    """Three clips of a few frames and differing lengths: tonal, LCG noise (raw frames), one frame."""
    return [RC.chord(sr, ch, 3 * HOP + 17, seed=5), RC.lcg_noise((2 * HOP + 600) * ch, seed=77), RC.chord(sr, ch, 513, seed=6)]


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("ch", [1, 2, 3, 4, 8])
def test_only_the_clips_samples_are_written(glc_amd, torch, ch, planar):
    sr = 48000
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    rt = ctx(glc_amd, "rt", sr)
    T = max(c.size // ch for c in clips)
    # dense; then strides larger than needed and odd, the buffer entered 4 bytes off a 16-byte boundary, so that
    # planes and clips start at every offset from one
    for lead, plane_gap, clip_gap in [(0, 0, 0), (1, 37, 101), (3, 2, 64), (2, 1, 1)]:
        kw = dict(lead=lead, tail=9)
        if planar:
            kw["channel_stride"] = T + plane_gap
            kw["clip_stride"] = (ch - 1) * (T + plane_gap) + T + clip_gap
        else:
            kw["clip_stride"] = T * ch + clip_gap
        src = Batch(clips, ch, planar, **kw)
        run(torch, rt, src, src, refs)


# ------------------------------------------------------------------------------------------ 3: isolation

@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
def test_neighbours_do_not_leak(glc_amd, torch, planar):
    sr, ch = 44100, 2
    n = 4 * HOP + 200
    loud = [RC.lcg_noise(n * ch, seed=s, amp=1.0) for s in (1, 2)]
    silent = np.zeros(n * ch, F32)
    r_loud = [oracle(("loud", s), x, sr, ch)[1] for s, x in zip((1, 2), loud)]
    r_silent = oracle("silent", silent, sr, ch)[1]
    assert not bits(r_silent).any()
    rt = ctx(glc_amd, "rt", sr)
    b = Batch([loud[0], silent, loud[1]], ch, planar)
    run(torch, rt, b, b, [r_loud[0], r_silent, r_loud[1]])
    same = Batch([loud[0]] * 3, ch, planar)
    run(torch, rt, same, same, [r_loud[0]] * 3)


# ------------------------------------------------------------------------------------------ 4: counts

def test_one_and_two_clips(glc_amd, torch):
    sr, ch = 48000, 2
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    rt = ctx(glc_amd, "rt", sr)
    for planar in (True, False):
        for k in (1, 2):
            b = Batch(clips[:k], ch, planar, lead=1, tail=5)
            run(torch, rt, b, b, refs[:k])
            assert [i.n_frames for i in rt.last_batch_info()] == [RC.frames_of(n) for n in b.lens]


def test_seven_hundred_one_frame_clips_in_one_round(glc_amd, torch):
    sr, ch = 48000, 1
    kinds = [RC.chord(sr, 1, 513, seed=s) for s in (1, 2, 3)] + [RC.lcg_noise(513, seed=9), np.zeros(513, F32)]
    k_refs = [oracle(("one-frame", i), x, sr, ch)[1] for i, x in enumerate(kinds)]
    order = [(7 * i) % len(kinds) for i in range(700)]
    rt = ctx(glc_amd, "rt", sr)
    b = Batch([kinds[k] for k in order], ch, True, clip_stride=517, lead=1)
    run(torch, rt, b, b, [k_refs[k] for k in order])
    infos = rt.last_batch_info()
    per_kind = [ctx(glc_amd, "enc", sr).encode(x, ch).info() for x in kinds]
    assert all((i.n_frames, i.n_raw_frames, i.total_nnz) == (1, per_kind[k].n_raw_frames, per_kind[k].total_nnz)
               for i, k in zip(infos, order))


def long_clip(sr, ch, n_frames, seed):
    """`n_frames` frames of chord and noise segments: compressed and raw frames, cheap to make."""
    per_channel = n_frames * HOP - 100
    assert RC.frames_of(per_channel) == n_frames
    seg = np.concatenate([cf.gen_chord(sr, ch, 3 * HOP, seed=seed), RC.lcg_noise(2 * HOP * ch, seed=seed)])
    return np.resize(seg, per_channel * ch).astype(F32)


def check_infos(g, rt, encs):
    infos = rt.last_batch_info()
    assert len(infos) == len(encs)
    for got, enc in zip(infos, encs):
        i = enc.info()
        assert (got.n_frames, got.n_raw_frames, got.total_nnz) == (i.n_frames, i.n_raw_frames, i.total_nnz)
        assert got.serialized_bytes == g.lib.glc_serialized_size(enc._h)


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
def test_a_batch_that_spills_into_a_second_round(glc_amd, torch, planar):
    sr, ch = 44100, 2
    kinds = [long_clip(sr, ch, 110, seed=s) for s in (1, 2, 3)]
    two = [two_step(glc_amd, sr, x, ch) for x in kinds]
    order = [i % 3 for i in range(40)]
    assert 40 * 111 > 4096                                   # virtual frames: more than a round holds
    rt = ctx(glc_amd, "rt", sr)
    b = Batch([kinds[k] for k in order], ch, planar, lead=1)
    run(torch, rt, b, b, [two[k][1] for k in order])
    check_infos(glc_amd, rt, [two[k][0] for k in order])


@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in-place"])
def test_a_clip_longer_than_a_round_between_two_short_ones(glc_amd, torch, in_place):
    sr, ch = 44100, 2
    clips = [long_clip(sr, ch, 7, seed=1), long_clip(sr, ch, 4100, seed=2), long_clip(sr, ch, 5, seed=3)]
    two = [two_step(glc_amd, sr, x, ch) for x in clips]
    rt = ctx(glc_amd, "rt", sr)
    b = Batch(clips, ch, True, lead=1, channel_stride=4100 * HOP + 3)
    run(torch, rt, b, b, [t[1] for t in two], in_place=in_place)
    check_infos(glc_amd, rt, [t[0] for t in two])


# ------------------------------------------------------------------------------------------ 5: layout conversion

@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("planar_in", [True, False], ids=["planar-to-interleaved", "interleaved-to-planar"])
def test_layout_conversion(glc_amd, torch, ch, planar_in):
    sr = 48000
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    src = Batch(clips, ch, planar_in, lead=1)
    T = src.T
    dst = src.like(not planar_in, lead=3, tail=4,
                   **(dict(clip_stride=T * ch + 5) if planar_in else dict(channel_stride=T + 1, clip_stride=ch * (T + 1) + 2)))
    run(torch, ctx(glc_amd, "rt", sr), src, dst, refs)


# ------------------------------------------------------------------------------------------ 6: in place

@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
def test_in_place(glc_amd, torch, planar):
    sr, ch = 48000, 2
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    b = Batch(clips, ch, planar, lead=2, tail=3)
    run(torch, ctx(glc_amd, "rt", sr), b, b, refs, in_place=True)      # the padding stays the NaN pattern it was


# ------------------------------------------------------------------------------------------ 7: torch's stream

@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
def test_apply_batch_tensor_on_torchs_current_stream(glc_amd, torch, planar):
    sr, ch = 48000, 2
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    rt = ctx(glc_amd, "rt", sr)
    b = Batch([c * F32(0.5) for c in clips], ch, planar)
    words = b.fill(b.clips)
    words[words == NAN_BITS] = 0
    _, half = b.tensor(torch, words)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xt = half + half            # filled by a kernel on this stream: x * 0.5 * 2 is x exactly
        yt = rt.apply_batch_tensor(xt, lengths=b.lens, planar=planar)
        zt = yt.clone()             # ... and read by one, with no synchronisation in between
    assert glc_amd.lib.glc_ctx_stream(rt._h) != side.cuda_stream      # the private stream is back
    side.synchronize()
    got = zt.cpu().numpy()
    for i, ref in enumerate(refs):
        n = b.lens[i]
        clip = got[i, :, :n].T if planar else got[i, :n, :]
        assert np.array_equal(bits(clip).reshape(-1), bits(ref))


# ------------------------------------------------------------------------------------------ 9: errors

def test_errors_write_nothing(glc_amd, torch):
    sr, ch = 48000, 2
    g, L = glc_amd, glc_amd.lib
    Lay = g._lib.GlcClipLayout
    rt = ctx(g, "rt", sr)
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    b = Batch(clips, ch, True)
    _, x = b.tensor(torch, b.fill(b.clips))
    out = torch.from_numpy(np.full(b.size + 8, NAN_BITS, np.uint32).view(F32)).cuda()
    torch.cuda.synchronize()
    T, n = b.T, len(clips)
    lens = (C.c_uint64 * n)(*b.lens)
    short = (C.c_uint64 * n)(b.lens[0], 512, b.lens[2])
    other = (C.c_uint64 * n)(b.lens[0], b.lens[1] - 1, b.lens[2])
    lp = lambda a: C.cast(a, C.POINTER(C.c_uint64))

    def lay(n_clips=n, channels=ch, planar=1, clip_stride=ch * T, channel_stride=T, length=T, lengths=lens):
        return Lay(n_clips, channels, planar, clip_stride, channel_stride, length, lp(lengths) if lengths is not None else None)

    def call(d_pcm, lin, d_out, lout):
        return L.glc_roundtrip_batch_device(rt._h, C.c_void_p(d_pcm), C.byref(lin) if lin else None, C.c_void_p(d_out),
                                            C.byref(lout) if lout else None)

    X, Y, ok = x.data_ptr(), out.data_ptr(), lay()
    refusals = [
        (None, ok, Y, ok), (X, ok, None, ok), (X, None, Y, ok), (X, ok, Y, None),             # null pointers
        (X, lay(channels=0), Y, lay(channels=0)),                                             # channels == 0
        (X, lay(lengths=short), Y, lay(lengths=short)),                                       # a clip the encoder refuses
        (X, lay(lengths=None, length=512), Y, lay(lengths=None, length=512)),
        (X, lay(channel_stride=T - 1), Y, ok), (X, ok, Y, lay(channel_stride=T - 1)),         # a plane does not fit its stride
        (X, lay(clip_stride=ch * T - 1), Y, ok), (X, ok, Y, lay(clip_stride=ch * T - 1)),     # a clip does not fit its stride
        (X, lay(planar=0, clip_stride=ch * T - 1), Y, ok),
        (X, ok, Y, lay(n_clips=n - 1)), (X, ok, Y, lay(channels=1)), (X, ok, Y, lay(lengths=other)),   # mismatching layouts
        (X, ok, Y, lay(lengths=None)),
        (X, ok, X + 4, ok), (X, ok, X, lay(planar=0)), (X, ok, X, lay(channel_stride=T + 1, clip_stride=ch * (T + 1))),   # overlap
        (X, ok, X + 4 * (b.size - 1), ok),
    ]
    for k, args in enumerate(refusals):
        assert call(*args) == EINVAL, k
        assert L.glc_last_error(rt._h), k
    assert call(X, lay(lengths=short), Y, lay(lengths=short)) == EINVAL and b"clip 1" in L.glc_last_error(rt._h)
    assert call(X, lay(n_clips=0), Y, lay(n_clips=0)) == 0                                    # an empty batch is no error
    cpu = torch.zeros(2, ch, 2048)
    for bad, kw in [(cpu, {}), (x.double(), {}), (x.transpose(1, 2), {}), (x[:, :, ::2], {}), (x, dict(out=cpu)),
                    (x, dict(out=out[:x.numel()].view(x.shape).double())), (x[0], {})]:
        with pytest.raises(TypeError):
            rt.apply_batch_tensor(bad, **kw)
    with pytest.raises(g.GlcError):
        rt.apply_batch_tensor(x, lengths=b.lens[:2])
    with pytest.raises(g.GlcError):
        rt.apply_batch_tensor(x, lengths=[b.lens[0], 512, b.lens[2]])
    with pytest.raises(g.GlcError):
        rt.apply_batch_tensor(x, lengths=b.lens, out=out[:n * ch * (T + 1)].view(n, ch, T + 1))
    if torch.cuda.device_count() > 1:
        with pytest.raises(g.GlcError):
            rt.apply_batch_tensor(x.to("cuda:1"))
    rt.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)
    # the context works afterwards
    run(torch, rt, b, b, refs)


def test_last_batch_info_needs_a_batch(glc_amd, torch):
    rt = glc_amd.RoundTrip(44100)
    info = (glc_amd._lib.GlcRoundtripInfo * 2)()
    assert glc_amd.lib.glc_roundtrip_batch_last_info(rt._h, info, 2) == EINVAL
    x = torch.from_numpy(np.stack([RC.chord(44100, 1, 600, seed=s) for s in (1, 2)])[:, None, :].copy()).cuda()
    torch.cuda.synchronize()
    rt.apply_batch_tensor(x)
    assert glc_amd.lib.glc_roundtrip_batch_last_info(rt._h, info, 3) == EINVAL
    assert glc_amd.lib.glc_roundtrip_batch_last_info(rt._h, info, 2) == 0 and info[0].n_frames == info[1].n_frames == 1
    rt.close()


# ------------------------------------------------------------------------------------------ 10: context state

def test_context_state_around_batch_calls(glc_amd, torch):
    sr, ch = 48000, 2
    clips = small_clips(sr, ch)
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    a = RC.mixed_clip(sr, ch)
    enc_a, ref_a = two_step(glc_amd, sr, a, ch)
    glc_a = enc_a.to_bytes()
    one = glc_amd.Decoder(ch, sr)                    # ONE context does everything below
    RT, ENC = glc_amd.RoundTrip, glc_amd.Encoder
    assert np.array_equal(bits(one.decode(enc_a)), bits(ref_a))
    assert one.resident_stream() == enc_a.stream_id != 0
    small = Batch(clips[:2], ch, True, lead=1)
    large = Batch([clips[i % 3] for i in range(9)] + [a], ch, False, lead=3, tail=2)
    large_refs = [refs[i % 3] for i in range(9)] + [ref_a]
    # two batch calls of different sizes back to back (workspaces grow, the staged tables are reused), then the
    # smaller one again: the same bits as each alone
    in_s, in_l = small.tensor(torch, small.fill(small.clips)), large.tensor(torch, large.fill(large.clips))
    out_s, out_l, out_s2 = (bt.tensor(torch, np.full(bt.size, NAN_BITS, np.uint32)) for bt in (small, large, small))
    torch.cuda.synchronize()
    RT.apply_batch_tensor(one, in_s[1], lengths=small.lens, planar=True, out=out_s[1])
    RT.apply_batch_tensor(one, in_l[1], lengths=large.lens, planar=False, out=out_l[1])
    RT.apply_batch_tensor(one, in_s[1], lengths=small.lens, planar=True, out=out_s2[1])
    assert one.resident_stream() == 0
    one.synchronize()
    assert np.array_equal(out_s[0].cpu().numpy().view(np.uint32), small.fill(refs[:2]))
    assert np.array_equal(out_l[0].cpu().numpy().view(np.uint32), large.fill(large_refs))
    assert np.array_equal(out_s2[0].cpu().numpy().view(np.uint32), small.fill(refs[:2]))
    # the stream that was resident is uploaded again; a single-clip round trip, an encode and a decode give what they gave
    assert np.array_equal(bits(one.decode(enc_a)), bits(ref_a))
    assert one.resident_stream() == enc_a.stream_id
    assert np.array_equal(bits(RT.apply(one, a, ch)), bits(ref_a))
    run(torch, one, small, small, refs[:2])
    assert ENC.encode(one, a, ch).to_bytes() == glc_a
    assert np.array_equal(bits(one.decode(enc_a)), bits(ref_a))
    # an open streaming session is closed by the call
    glc_amd.lib.glc_decode_stream_begin(one._h, enc_a._h)
    run(torch, one, small, small, refs[:2])
    n, last = C.c_uint64(), C.c_int()
    buf = np.empty(501 * HOP * ch, F32)
    assert glc_amd.lib.glc_decode_stream_next(one._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n), C.byref(last)) == EINVAL
    one.close()


# ------------------------------------------------------------------------------------------ offsets past 2^32

def test_a_layout_that_spans_more_than_2_to_the_32_elements(glc_amd, torch):
    """Two stereo clips 2^32 + 5 elements apart, planes 2^31 + 3 apart in the input: every offset needs 64 bits."""
    sr, ch = 48000, 2
    clips = small_clips(sr, ch)[:2]
    refs = [oracle(("small", ch, i), x, sr, ch)[1] for i, x in enumerate(clips)]
    T = max(c.size // ch for c in clips)
    cstride, pstride = 2 ** 32 + 5, 2 ** 31 + 3
    store = torch.empty(cstride + pstride + T + 8, dtype=torch.float32, device="cuda")       # 24 GiB, never filled
    x = store.as_strided((2, ch, T), (cstride, pstride, 1), 1)
    for i, c in enumerate(clips):
        n = c.size // ch
        x[i, :, :n] = torch.from_numpy(np.ascontiguousarray(c.reshape(-1, ch).T)).cuda()
    guard = torch.from_numpy(np.full(64, NAN_BITS, np.uint32).view(F32)).cuda()
    spots = [1 + i * cstride + c * pstride + off for i in range(2) for c in range(ch) for off in (-1, clips[i].size // ch)]
    for s in spots:                      # the word in front of every plane and the one behind its samples
        store[s] = guard[0]
    torch.cuda.synchronize()
    rt = ctx(glc_amd, "rt", sr)
    rt.apply_batch_tensor(x, lengths=[c.size // ch for c in clips], planar=True, out=x)
    rt.synchronize()
    for i, ref in enumerate(refs):
        n = clips[i].size // ch
        assert np.array_equal(bits(x[i, :, :n].cpu().numpy().T).reshape(-1), bits(ref))
    assert all(int(store[s].view(torch.int32).item()) == NAN_BITS for s in spots)
    # ... and from a small dense batch into an interleaved one whose second clip lies behind 2^32 elements
    dense = Batch(clips, ch, True)
    _, xd = dense.tensor(torch, dense.fill(clips))
    y = store.as_strided((2, T, ch), (cstride, ch, 1), 3)
    torch.cuda.synchronize()
    rt.apply_batch_tensor(xd, lengths=dense.lens, planar=True, out=y, out_planar=False)
    rt.synchronize()
    for i, ref in enumerate(refs):
        n = clips[i].size // ch
        assert np.array_equal(bits(y[i, :n, :].cpu().numpy()).reshape(-1), bits(ref))
    del store, x, y
    torch.cuda.empty_cache()
