"""What the eleven torch-tensor methods of codec.py refuse before the C call, and with which exception: TypeError for a
tensor of the wrong kind (no CUDA tensor, dtype, rank, shape, contiguity, strides), GlcError(GLC_EINVAL) for a wrong
value or a wrong device.  One table row per refusal, one accepted call per method; the table was recorded on the
commit before the checks became shared helpers and holds for them unchanged.  A refusal never reaches the device.

The second half needs no GPU: the clip-layout rule reads shapes and strides only, and the stream scope is held to a
stub context."""
import numpy as np
import pytest

import roundtrip_cases as RC

EINVAL = -1
SR, CH, B, T = 48000, 2, 2, 520      # two clips of two channels, just over the 512 samples the encoder refuses


class _State:
    pass


@pytest.fixture(scope="module")
def S():
    """Contexts of every class and one good argument of every kind, built by the accepted calls themselves."""
    import torch

    import glc_amd as g
    s = _State()
    s.torch, s.g = torch, g
    clips = [RC.chord(SR, CH, T, seed=11 + i).reshape(T, CH) for i in range(B)]
    s.xi = torch.from_numpy(np.stack(clips)).cuda()                        # (B, T, C)
    s.x = s.xi.transpose(1, 2).contiguous()                                # (B, C, T)
    s.x1 = s.xi[0].contiguous().reshape(-1)                                # one clip, interleaved
    s.enc, s.dec, s.rt = g.Encoder(SR), g.Decoder(CH, SR), g.RoundTrip(SR)
    s.se, s.sd = g.StreamEncoder(SR, CH, n_streams=B), g.StreamDecoder(SR, CH, n_streams=B)
    s.arena, s.cursor, s.entries = s.enc.encode_compact_batch_tensor(s.x)
    s.blobs = g.store_blobs(s.arena, s.entries)
    assert all(b is not None for b in s.blobs)
    s.ns = [T * CH] * B
    s.lengths_t = torch.full((B,), T, dtype=torch.int64, device="cuda")
    s.keep = torch.ones(B, dtype=torch.uint8, device="cuda")
    s.clips_t = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    s.starts_t = torch.tensor([0, 3], dtype=torch.int64, device="cuda")
    s.blob1, _ = s.enc.encode_compact_tensor(s.x1, CH)
    s.seg_arena = torch.zeros(1 << 18, dtype=torch.uint8, device="cuda")
    s.seg_entries, s.segs = g.StreamEncoder(SR, CH, n_streams=B).push_tensor(
        s.x, None, [True] * B, s.seg_arena, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert len(s.segs) == B
    torch.cuda.synchronize()
    yield s
    for k in ("enc", "dec", "rt", "se", "sd"):      # contexts: released while the library is still loaded
        getattr(s, k).close()


def good(S, name):
    """(bound method, its accepted keyword arguments) of one of the eleven."""
    t = S.torch
    zeros = lambda *shape, dtype=t.float32: t.zeros(shape, dtype=dtype, device="cuda")
    return {
        "compact_store": (S.dec.compact_store_tensor, dict(arena=S.arena.clone(), entries=S.entries, lengths=S.lengths_t, keep=S.keep,
                                                           out_arena=None, used_bytes=None)),
        "encode_compact": (S.enc.encode_compact_tensor, dict(x=S.x1, channels=CH)),
        "encode_batch": (S.enc.encode_compact_batch_tensor, dict(x=S.x, lengths=[T, T - 1], planar=True, arena=t.zeros_like(S.arena),
                                                                 cursor=zeros(1, dtype=t.int64), bits=None)),
        "decode_compact": (S.dec.decode_compact_tensor, dict(blob=S.blob1, n_samples=T * CH, out=zeros(T * CH))),
        "decode_batch": (S.dec.decode_compact_batch_tensor, dict(blobs=S.blobs, n_samples=S.ns, lengths=None, planar=True,
                                                                 out=zeros(B, CH, T), dtype=None)),
        "decode_crops": (S.dec.decode_compact_crops_tensor, dict(blobs=S.blobs, n_samples=S.ns, starts=[0, 5], lengths=100, planar=True,
                                                                 out=zeros(B, CH, 100), dtype=None)),
        "store_crops": (S.dec.decode_store_crops_tensor, dict(arena=S.arena, entries=S.entries, lengths=S.lengths_t, clips=S.clips_t,
                                                              starts=S.starts_t, length=100, max_length=T, planar=True,
                                                              out=zeros(B, CH, 100), dtype=None)),
        "apply": (S.rt.apply_tensor, dict(x=S.x1, channels=CH)),
        "apply_batch": (S.rt.apply_batch_tensor, dict(x=S.x, lengths=[T, T - 1], planar=True, out=zeros(B, CH, T), out_planar=None,
                                                      bits=None, out_dtype=None)),
        "stream_enc": (S.se.push_tensor, dict(x=S.x, lengths=[T, T - 1], finish=[True] * B, arena=t.zeros_like(S.seg_arena),
                                              cursor=zeros(1, dtype=t.int64), planar=True, bits=None)),
        "stream_dec": (S.sd.push_tensor, dict(arena=S.seg_arena, entries=S.seg_entries, segs=S.segs, finish=[True] * B,
                                              total_len=[T] * B, planar=True, out=zeros(B, CH, T), dtype=None)),
    }[name]


# Ways a tensor is of the wrong kind, by the kind that is asked for; each gives a TypeError.
def _bad_u8(arg):
    """A contiguous 1-D uint8 CUDA tensor is asked for (arena, out_arena, blob)."""
    return [(f"{arg} on the host", lambda S, v: v.cpu()), (f"{arg} int8", lambda S, v: v.view(S.torch.int8)),
            (f"{arg} strided", lambda S, v: v[::2]), (f"{arg} 2-D", lambda S, v: v[:v.numel() // 2 * 2].view(2, -1))]


def _bad_i64(arg):
    """A contiguous int64 CUDA tensor of a given shape is asked for (entries, lengths, clips, starts)."""
    return [(f"{arg} on the host", lambda S, v: v.cpu()), (f"{arg} int32", lambda S, v: v.int()),
            (f"{arg} strided", lambda S, v: S.torch.stack([v, v], -1)[..., 0]), (f"{arg} of another rank", lambda S, v: v.unsqueeze(-1))]


def _bad_clips(arg, dtype="float64"):
    """A 3-D CUDA tensor of samples with innermost stride 1 is asked for (x, out)."""
    return [(f"{arg} on the host", lambda S, v: v.cpu()), (f"{arg} {dtype}", lambda S, v: v.to(getattr(S.torch, dtype))),
            (f"{arg} 2-D", lambda S, v: v[0]), (f"{arg} innermost stride 2", lambda S, v: S.torch.cat([v, v], 2)[:, :, ::2])]


def _rows():
    """(method, what is wrong, {argument: f(S, good value) -> bad value}, exception, a word of its message)."""
    TE, GE = TypeError, "GlcError"
    rows = []

    def add(method, arg, cases, exc=TE, word=None, **also):
        for label, f in cases:
            rows.append((method, label, {arg: f, **{k: c if callable(c) else (lambda S, v, c=c: c) for k, c in also.items()}}, exc, word))

    # ---- _Ctx.compact_store_tensor
    add("compact_store", "arena", _bad_u8("arena"), word="arena")
    add("compact_store", "entries", _bad_i64("entries") + [("entries (n, 3)", lambda S, v: v[:, :3].contiguous())], word="entries")
    add("compact_store", "lengths", _bad_i64("lengths") + [("lengths of another count", lambda S, v: S.torch.cat([v, v]))], word="lengths")
    add("compact_store", "keep", [("keep on the host", lambda S, v: v.cpu()), ("keep int64", lambda S, v: v.long()),
                                  ("keep strided", lambda S, v: S.torch.cat([v, v])[::2]),
                                  ("keep of another count", lambda S, v: S.torch.cat([v, v]))], word="keep")
    add("compact_store", "out_arena", [(label, lambda S, v, f=f: f(S, S.torch.zeros_like(S.arena))) for label, f in _bad_u8("out_arena")], word="out_arena")
    add("compact_store", "used_bytes", [("used_bytes above the arena", lambda S, v: S.arena.numel() + 1), ("used_bytes negative", lambda S, v: -1)],
        GE, "used_bytes")
    # ---- the two single-clip methods: a contiguous float32 CUDA tensor of any rank
    for m in ("encode_compact", "apply"):
        add(m, "x", [("x on the host", lambda S, v: v.cpu()), ("x float64", lambda S, v: v.double()), ("x int16", lambda S, v: v.short()),
                     ("x strided", lambda S, v: v[::2])], word="float32")
    add("apply", "x", [("x 3-D", lambda S, v: v.reshape(1, T, CH)), ("x (frames, 3) for 2 channels", lambda S, v: v[:T // 3 * 3].reshape(-1, 3))], GE)
    add("decode_compact", "blob", _bad_u8("blob"), word="blob")
    add("decode_compact", "out", [("out on the host", lambda S, v: v.cpu()), ("out float64", lambda S, v: v.double()),
                                  ("out strided", lambda S, v: S.torch.cat([v, v])[::2]), ("out 2-D", lambda S, v: v.reshape(T, CH))], word="out")
    # ---- the clip tensors: x of the three that take samples, out of the four that give them
    dense = lambda S, v: S.torch.cat([v.transpose(1, 2)] * 2, 2)[:, :, :v.shape[1]]      # (B, T, C) with 2 C between samples
    for m in ("encode_batch", "apply_batch", "stream_enc"):
        add(m, "x", _bad_clips("x"), word="x")
        add(m, "x", [("x interleaved and not dense", dense)], word="dense", planar=False)
        add(m, "lengths", [("lengths of another count", lambda S, v: [T]), ("a length above T", lambda S, v: [T, T + 1]),
                           ("a negative length", lambda S, v: [-1, T]), ("lengths a tensor above T", lambda S, v: S.torch.tensor([T + 1, T]))], GE, "lengths")
        add(m, "bits", [("bits for float32 samples", lambda S, v: 12)], word="bits")
        add(m, "bits", [("17 bits in int16 samples", lambda S, v: 17)], GE, "bits", x=lambda S, v: v.mul(32767).short())
    for m in ("encode_batch", "apply_batch"):
        add(m, "x", [("x of no channels", lambda S, v: v[:, :0])], GE, "channels")
    add("stream_enc", "x", [("x of three lanes", lambda S, v: S.torch.cat([v, v[:1]])), ("x of three channels", lambda S, v: S.torch.cat([v, v[:, :1]], 1))],
        GE, "lanes")
    add("stream_enc", "finish", [("finish of another count", lambda S, v: [True])], GE, "finish")
    for m in ("encode_batch", "stream_enc"):
        add(m, "arena", _bad_u8("arena"), word="arena")
        add(m, "cursor", [("cursor on the host", lambda S, v: v.cpu()), ("cursor int32", lambda S, v: v.int()),
                          ("cursor of two elements", lambda S, v: S.torch.cat([v, v])),
                          ("cursor strided, two elements", lambda S, v: S.torch.cat([v] * 4)[::2])], word="cursor")
    for m in ("decode_batch", "decode_crops", "store_crops", "apply_batch"):
        add(m, "out", _bad_clips("out"), word="out")
        add(m, "out_dtype" if m == "apply_batch" else "dtype", [("dtype float64", lambda S, v: "float64")], word="dtype")
        add(m, "out_dtype" if m == "apply_batch" else "dtype", [("dtype int16 for a float32 out", lambda S, v: "int16")], word="out")
        add(m, "out", [("out interleaved and not dense", dense)], word="dense", **{"out_planar" if m == "apply_batch" else "planar": False})
        add(m, "out", [("out of three clips", lambda S, v: S.torch.cat([v, v[:1]])), ("out of three channels", lambda S, v: S.torch.cat([v, v[:, :1]], 1)),
                       ("out shorter than the clips", lambda S, v: v[:, :, :-1].contiguous())], GE)
    add("store_crops", "out", [("out longer than the crops", lambda S, v: S.torch.cat([v, v], 2))], GE, "out")
    add("apply_batch", "out", [("out longer than x", lambda S, v: S.torch.cat([v, v], 2))], GE, "out")
    # ---- blobs and the per-clip sequences of the compact decodes
    for m in ("decode_batch", "decode_crops"):
        add(m, "blobs", [(label.replace("blob", "blobs[1]"), lambda S, v, f=f: [v[0], f(S, v[1])]) for label, f in _bad_u8("blob")], word=r"blobs\[1\]")
        add(m, "n_samples", [("n_samples of another count", lambda S, v: v[:1])], GE, "n_samples")
        add(m, "lengths", [("lengths of another count", lambda S, v: [100])], GE, "lengths")
    add("decode_crops", "starts", [("starts of another count", lambda S, v: [0]), ("a negative start", lambda S, v: [0, -1])], GE, "starts")
    # ---- the store draw
    add("store_crops", "arena", _bad_u8("arena"), word="arena")
    add("store_crops", "entries", _bad_i64("entries") + [("entries (n, 3)", lambda S, v: v[:, :3].contiguous())], word="entries")
    for a in ("lengths", "clips", "starts"):
        add("store_crops", a, _bad_i64(a), word=a)
    add("store_crops", "lengths", [("lengths of another count than entries", lambda S, v: v[:1])], GE)
    add("store_crops", "starts", [("starts of another count than clips", lambda S, v: v[:1])], GE)
    add("store_crops", "length", [("a negative length", lambda S, v: -1)], GE, "length")
    # ---- the streaming decode push: its `out` is contiguous, and every fault of its shape is a TypeError
    add("stream_dec", "arena", _bad_u8("arena"), word="arena")
    add("stream_dec", "entries", _bad_i64("entries") + [("entries of another count than segs", lambda S, v: S.torch.cat([v, v]))], word="entries")
    add("stream_dec", "segs", [("a segment of lane 2 of 2", lambda S, v: [v[0], (2,) + tuple(v[1][1:])])], GE, "lane")
    add("stream_dec", "finish", [("finish of another count", lambda S, v: [True])], GE, "finish")
    add("stream_dec", "out", _bad_clips("out")[:1] + _bad_clips("out")[2:] + [
        ("out of three lanes", lambda S, v: S.torch.cat([v, v[:1]])), ("out of three channels", lambda S, v: S.torch.cat([v, v[:, :1]], 1)),
        ("out shorter than the spans", lambda S, v: v[:, :, :-1].contiguous()), ("out a slice", lambda S, v: S.torch.cat([v, v], 2)[:, :, :T])], word="out")
    return rows


ROWS = _rows()
METHODS = ["compact_store", "encode_compact", "encode_batch", "decode_compact", "decode_batch", "decode_crops", "store_crops", "apply",
           "apply_batch", "stream_enc", "stream_dec"]


def test_the_table_covers_the_eleven_methods():
    assert {r[0] for r in ROWS} == set(METHODS) and len(METHODS) == 11
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS), "two rows of one name"
    for m in METHODS:
        kinds = {r[3] for r in ROWS if r[0] == m}
        assert TypeError in kinds, m
        assert "GlcError" in kinds or m in ("encode_compact", "decode_compact"), m    # these two refuse values in the C call only


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[f"{r[0]}-{r[1]}".replace(" ", "_") for r in ROWS])
def test_refused_before_the_c_call(S, row):
    method, _, changes, exc, word = row
    fn, kw = good(S, method)
    for arg, f in changes.items():
        kw[arg] = f(S, kw[arg])
    with pytest.raises(S.g.GlcError if exc == "GlcError" else exc, match=word) as e:
        fn(**kw)
    if exc == "GlcError":
        assert e.value.code == EINVAL


@pytest.mark.gpu
def test_every_method_takes_its_good_arguments(S):
    """The accepted call of each table: the arguments the rows above spoil one at a time."""
    t, g = S.torch, S.g
    S.se, S.sd = g.StreamEncoder(SR, CH, n_streams=B), g.StreamDecoder(SR, CH, n_streams=B)     # fresh lanes
    got = {}
    for m in METHODS:
        fn, kw = good(S, m)
        got[m] = (fn(**kw), kw)
    t.cuda.synchronize()
    ents, lens_out, new_index, n_out, cur = got["compact_store"][0]
    assert int(n_out.item()) == B and new_index.tolist() == [0, 1] and lens_out.tolist() == [T, T] and ents.shape == (B, 4) and cur.shape == (1,)
    blob, info = got["encode_compact"][0]
    assert t.equal(blob, S.blob1) and info.bytes == blob.numel()
    arena, cursor, entries = got["encode_batch"][0]
    assert arena is got["encode_batch"][1]["arena"] and entries.shape == (B, 4) and 0 < int(cursor.item()) <= arena.numel()
    one = got["decode_compact"][0]
    whole = got["decode_batch"][0]
    assert one.shape == (T * CH,) and whole is got["decode_batch"][1]["out"]
    assert t.equal(one.view(T, CH).t(), whole[0]), "one blob decodes alone as it does in a batch"
    crops = got["decode_crops"][0]
    assert t.equal(crops[0], whole[0, :, 0:100]) and t.equal(crops[1], whole[1, :, 5:105])
    draws = got["store_crops"][0]
    assert t.equal(draws[0], whole[0, :, 0:100]) and t.equal(draws[1], whole[1, :, 3:103])
    assert [s.flags for s in S.dec.last_compact_status()] == [0] * B
    y1, yb = got["apply"][0], got["apply_batch"][0]
    assert y1.shape == S.x1.shape and t.equal(y1.view(T, CH).t(), yb[0]) and t.equal(yb[0], whole[0])
    assert not yb[1, :, T - 1:].any(), "nothing is written behind a clip's length"
    seg_entries, segs = got["stream_enc"][0]
    assert seg_entries.shape == (len(segs), 4) and sorted(s[0] for s in segs) == [0, 1]
    out, emitted = got["stream_dec"][0]
    assert emitted == [T] * B and t.equal(out, whole)
    assert [s.flags for s in S.sd.last_compact_status()] == [0] * len(S.segs)


@pytest.mark.gpu
def test_every_method_waits_for_the_legacy_default_stream(S, monkeypatch):
    """On torch's legacy default stream (handle 0, which means the private stream to the library) each of the eleven
    waits for what torch has queued there before it queues anything, and leaves the private stream set."""
    t, g = S.torch, S.g
    real = t.cuda.current_stream
    log = []

    class Proxy:
        def __init__(self, s):
            self.s, self.cuda_stream = s, s.cuda_stream

        def synchronize(self):
            log.append("synchronised")
            self.s.synchronize()
    S.se, S.sd = g.StreamEncoder(SR, CH, n_streams=B), g.StreamDecoder(SR, CH, n_streams=B)
    streams = []
    monkeypatch.setattr(g.codec._Ctx, "set_stream", lambda self, raw, f=g.codec._Ctx.set_stream: (streams.append(raw), f(self, raw))[1])
    with t.cuda.stream(t.cuda.default_stream()):
        assert real().cuda_stream == 0
        monkeypatch.setattr(t.cuda, "current_stream", lambda device=None: Proxy(real(device)))
        for m in METHODS:
            fn, kw = good(S, m)
            del log[:], streams[:]
            fn(**kw)
            assert log == ["synchronised"] and streams == [0, 0], m
        monkeypatch.undo()


@pytest.mark.gpu
def test_the_streaming_decode_holds_its_out_to_the_dtype(S):
    """Not a row of the table: before the output rule was shared this method took an `out` of any dtype and wrote
    float32 or int16 into it."""
    fn, kw = good(S, "stream_dec")
    for out, dtype in ((kw["out"].double(), None), (kw["out"], "int16"), (kw["out"].int(), None)):
        with pytest.raises(TypeError, match="out must be a contiguous (float32|int16) CUDA tensor"):
            fn(**{**kw, "out": out, "dtype": dtype})


@pytest.mark.gpu
def test_a_tensor_of_another_device_is_a_glc_error(S):
    """Only where there is a second device: the wrong device is a wrong value, not a wrong kind."""
    t = S.torch
    if t.cuda.device_count() < 2:
        return
    for m, arg in [("compact_store", "arena"), ("encode_compact", "x"), ("encode_batch", "x"), ("decode_compact", "blob"), ("store_crops", "arena"),
                   ("store_crops", "entries"), ("apply", "x"), ("apply_batch", "x"), ("apply_batch", "out"), ("stream_enc", "x"), ("stream_dec", "arena")]:
        fn, kw = good(S, m)
        kw[arg] = kw[arg].to("cuda:1")
        with pytest.raises(S.g.GlcError) as e:
            fn(**kw)
        assert e.value.code == EINVAL, (m, arg)


# ------------------------------------------------------------------------------------------ no GPU: the shared rules

def fields(lay):
    return (lay.n_clips, lay.channels, lay.planar, lay.clip_stride, lay.channel_stride, lay.length)


def test_clip_layout_reads_shape_and_strides():
    import torch

    from glc_amd import codec
    x = torch.zeros(3, 2, 7)                                      # planar (B, C, T)
    lay, b, c, n = codec._clip_layout(x, True, "x")
    assert (b, c, n) == (3, 2, 7) and fields(lay) == (3, 2, 1, 14, 7, 7) and not lay.lengths
    y = torch.zeros(3, 7, 2)                                      # interleaved (B, T, C): no plane stride
    lay, b, c, n = codec._clip_layout(y, False, "y")
    assert (b, c, n) == (3, 2, 7) and fields(lay) == (3, 2, 0, 14, 0, 7) and not lay.lengths
    big = torch.zeros(5, 4, 20)                                   # a slice keeps the strides of what it is cut from
    lay, b, c, n = codec._clip_layout(big[1:4, 1:3, 2:9], True, "x")
    assert (b, c, n) == (3, 2, 7) and fields(lay) == (3, 2, 1, 80, 20, 7)
    lay, b, c, n = codec._clip_layout(torch.zeros(5, 20, 2)[1:4, 2:9], False, "y")     # whole samples of a longer clip
    assert (b, c, n) == (3, 2, 7) and fields(lay) == (3, 2, 0, 40, 0, 7)
    lay = codec._clip_layout(big.as_strided((3, 2, 7), (3, 40, 1)), True, "x")[0]      # any strides: the C side judges overlap
    assert fields(lay) == (3, 2, 1, 3, 40, 7)


def test_clip_layout_refusals_and_their_edges():
    import torch

    from glc_amd import codec
    L = codec._clip_layout
    for t in (torch.zeros(4), torch.zeros(2, 4), torch.zeros(1, 2, 3, 4)):
        with pytest.raises(TypeError, match=r"x must have shape \(B, C, T\) or \(B, T, C\)"):
            L(t, True, "x")
    with pytest.raises(TypeError, match="out: the innermost stride must be 1"):
        L(torch.zeros(2, 2, 8)[:, :, ::2], True, "out")
    with pytest.raises(TypeError, match="innermost"):
        L(torch.zeros(2, 7, 2).transpose(1, 2), True, "x")        # interleaved storage read as planar
    with pytest.raises(TypeError, match=r"x: an interleaved clip must be dense \(stride 2 between samples\)"):
        L(torch.zeros(2, 7, 4)[:, :, :2], False, "x")
    # the innermost stride of a dimension of one element is never used
    assert fields(L(torch.zeros(2, 2, 8)[:, :, ::8], True, "x")[0]) == (2, 2, 1, 16, 8, 1)
    with pytest.raises(TypeError, match=r"dense \(stride 1 between samples\)"):
        L(torch.zeros(2, 7, 4)[:, :, ::4], False, "x")            # mono, but 4 elements from sample to sample
    # a clip of one sample (T == 1) and a batch of no clips (B == 0) have no two samples whose distance could be wrong
    assert fields(L(torch.zeros(2, 1, 4)[:, :, :2], False, "x")[0]) == (2, 2, 0, 4, 0, 1)
    assert fields(L(torch.zeros(2, 7, 4)[:0, :, :2], False, "x")[0]) == (0, 2, 0, 28, 0, 7)
    assert fields(L(torch.zeros(0, 2, 7), True, "x")[0]) == (0, 2, 1, 14, 7, 7)
    # no channels: the layout is built, the call site refuses the count
    assert L(torch.zeros(2, 0, 7), True, "x")[1:] == (2, 0, 7) and L(torch.zeros(2, 7, 0), False, "x")[1:] == (2, 0, 7)


def test_lengths_are_held_by_the_layout():
    import ctypes as C
    import gc

    import torch

    from glc_amd import codec
    lay = codec._clip_layout(torch.zeros(3, 2, 7), True, "x")[0]
    assert codec._set_lengths(lay, torch.tensor([7, 0, 3]), 3, 7) == [7, 0, 3]
    gc.collect()
    assert lay.lengths[:3] == [7, 0, 3] and C.addressof(lay.lengths_array) == C.addressof(lay.lengths.contents)
    for bad in ([7, 3], [7, 8, 3], [7, -1, 3]):
        with pytest.raises(codec.GlcError, match=r"lengths must hold 3 values in \[0, 7\]") as e:
            codec._set_lengths(lay, bad, 3, 7)
        assert e.value.code == EINVAL
    assert lay.lengths[:3] == [7, 0, 3], "a refused list leaves the layout as it was"
    empty = codec._clip_layout(torch.zeros(0, 2, 7), True, "x")[0]
    assert codec._set_lengths(empty, [], 0, 7) == [] and empty.lengths      # an empty batch still has a pointer to hand over
    assert len(codec._c_array(C.c_uint64, [])) == 1 and list(codec._c_array(C.c_uint64, [4, 5])) == [4, 5]


class _StubStream:
    def __init__(self, handle, log):
        self.cuda_stream, self._log = handle, log

    def synchronize(self):
        self._log.append("torch stream synchronised")


def _stub_ctx(log):
    from glc_amd import codec

    class Stub(codec._Ctx):
        def set_stream(self, raw_stream):
            log.append(("set_stream", raw_stream))

        def __del__(self):
            pass
    return Stub.__new__(Stub)


@pytest.mark.parametrize("handle", [0, 0x7F001234])
def test_the_stream_scope(monkeypatch, handle):
    import torch

    from glc_amd import codec
    log = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: log.append(("current_stream", device)) or _StubStream(handle, log))
    ctx = _stub_ctx(log)
    with codec._on_torch_stream(ctx, "cuda:0"):
        log.append("body")
    # the legacy default stream has no handle to pass on: what torch queued there is waited for, then the private stream serves
    entry = [("current_stream", "cuda:0")] + (["torch stream synchronised"] if handle == 0 else []) + [("set_stream", handle)]
    assert log == entry + ["body", ("set_stream", 0)]
    del log[:]
    with pytest.raises(KeyError):
        with codec._on_torch_stream(ctx, "cuda:0"):
            raise KeyError("the body fails")
    assert log == entry + [("set_stream", 0)], "the private stream is restored when the body raises"


def test_the_tensor_rule_names_what_it_wants():
    """The kind of object is judged before the device, so a host tensor is a TypeError on any context."""
    import torch

    from glc_amd import codec
    ctx = _stub_ctx([])
    ctx.device = 0
    for t, dtypes, shape, contiguous, text in [
            (torch.zeros(4, dtype=torch.uint8), torch.uint8, (None,), True, "arena must be a contiguous uint8 CUDA tensor of shape (n)"),
            (torch.zeros(2, 4, dtype=torch.int64), torch.int64, (None, 4), True, "arena must be a contiguous int64 CUDA tensor of shape (n, 4)"),
            (None, (torch.bool, torch.uint8), (3,), True, "arena must be a contiguous bool or uint8 CUDA tensor of shape (3)"),
            ([1.0], torch.float32, None, False, "arena must be a float32 CUDA tensor")]:
        with pytest.raises(TypeError) as e:
            ctx._tensor(t, "arena", dtypes, shape, contiguous)
        assert str(e.value) == text
