"""The screened encode path under the store, stream and PCM drivers (tests/encode_driver_cases.py builds the inputs;
tests/test_encode_screen_edges.py holds the path under glc_encode, glc_encode_batch and the float round trips, and its
helpers - the row model, the record model with its mutations, the stats hooks - are the ones used here).

CPU: every input's virtual stream, built in numpy exactly as its driver stages it, goes through the oracle and the
row model: noise fails, silence passes, a clicked frame fails, and only rows of frames that touch a clip's or a
lane's zero padding, or of a junk frame, may be too close to call - at most 2 % of an input's rows, the exact count
recorded in UNDECIDED.  For every input of 256 rows or more one mutation of the record model changes a byte of a
frame some clip or lane owns: the per-clip byte comparison can see a wrong screen on that input.
GPU: each driver with the screen forced on under both forms of the transform and both repairs, with all kinds
automatic, with the edge kind forced, and with the screen off - blobs and output words against oracle.encode /
oracle.decode per clip or lane, the rows screened exactly the rows the driver launched, the rows repaired inside the
model's window, the forced repair kind on every screened launch, no launch on the edge side stream, no byte written
outside the stored blobs or the clips' own words.  One store encode of a clip longer than a round in the automatic
mode: its first chunk of 8192 rows takes the path in the matrix form, its second of 600 does not."""
import ctypes as C
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_driver_cases as D  # noqa: E402
import encode_screen_edges as E  # noqa: E402
import store_int_cases as SI  # noqa: E402
import stream_encode_cases as SC  # noqa: E402
from encode_screen_edges import SR  # noqa: E402
from oracle import oracle as O  # noqa: E402

F32 = np.float32
HOP = E.HOP
NAMES = list(D.inputs())
STORE = [n for n in NAMES if D.inputs()[n].driver == "store"]
BUILT = (1, 2, 4, 8)          # channel counts the matrix form is built for (at 44.1 / 48 kHz)

# rows the model leaves undecided per input: what opens the GPU tests' lo..hi window of repaired rows, and no more.
# The condition is the cap - 2 % of an input's rows; the counts are what the reference gives for these inputs.
UNDECIDED = {
    "store-f32": 4, "store-s16": 4, "store-ch8": 5, "store-ch3": 5, "rtpcm-s16": 4,
    "push-first": 4, "push-middle": 0, "push-gap": 0, "push-finish": 0,
    "push-first-s32": 4, "push-middle-s32": 0, "push-gap-s32": 0, "push-finish-s32": 0,
    "push-ragged": 0, "push-ch4": 0, "push-small": 0,
}

_model = {}


def modelled(name):
    """name -> (Input, oracle records, taps, model verdict per row), once."""
    if name not in _model:
        inp = D.inputs()[name]
        rec, taps = E.expected(inp.case)
        _model[name] = (inp, rec, taps, E.model(inp.case, taps))
    return _model[name]


def window(name):
    """(lo, hi) of the rows a screened launch of the input repairs: the rows the model fails, the rows it does not pass."""
    v = modelled(name)[3]
    return int((v == -1).sum()), int((v != 1).sum())


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_the_inputs_are_the_shapes_the_drivers_launch():
    rows = {n: D.inputs()[n].rows for n in NAMES}
    assert rows["store-f32"] == rows["store-s16"] == 320 and rows["store-ch8"] >= 256 and rows["store-ch3"] >= 256
    assert rows["rtpcm-s16"] == 278
    for sfx in ("", "-s32"):
        assert [rows[f"push-{p}{sfx}"] for p in ("first", "middle", "gap", "finish")] == [334, 334, 158, 350]
    assert rows["push-ragged"] >= 256 and rows["push-ch4"] >= 256 and rows["push-small"] == 42
    assert set(NAMES) == set(UNDECIDED)
    # the pushes complete the frames they are named for, on every lane
    main = D.sessions()["main-f32"]
    for inp, (f0, n) in zip(main.inputs(), ((0, 20), (20, 20), (40, 9), (49, 21))):
        assert [(s[2], s[1]) for s in inp.segs] == [(f0, n)] * 8 and [s[5] for s in inp.segs] == list(range(8))
        assert inp.case.f0 == 1 and inp.case.f1 * HOP * 2 == inp.case.n_samples - HOP * 2
    # the ragged push: lanes 1, 6 get nothing, 3, 7 too little, 4 finishes, the rest complete 30 frames
    rag = D.inputs()["push-ragged"]
    assert [(s[5], s[2], s[1]) for s in rag.segs] == [(0, 0, 30), (2, 0, 30), (4, 0, 5), (5, 0, 30), (8, 0, 30)]
    rec, new, fin = rag.session.pushes()[0]
    assert [new[i] for i in (1, 6, 3, 7)] == [0, 0, 700, 1535] and fin == [i == 4 for i in range(9)]
    # integers: what the oracle sees is what the device widens them to
    s16 = D.inputs()["store-s16"]
    assert s16.clips[0].dtype == np.int16 and np.array_equal(s16.wide[0], s16.clips[0].astype(F32) / F32(32768.0))
    s32 = D.inputs()["push-first-s32"]
    assert s32.clips[0].dtype == np.int32 and np.abs(s32.clips[1]).max() >= 2 ** 22 and np.abs(s32.clips[1]).max() < 2 ** 23
    assert np.array_equal(s32.wide[1], s32.clips[1].astype(F32) / F32(2.0 ** 23))


@pytest.mark.parametrize("name", NAMES)
def test_driver_rows_are_decided_where_the_inputs_rely_on_them(name):
    """Per slot of the virtual stream: its frames by the stream frame they are (a push's segment starts at first_frame,
    a clip's at 0), the junk frame behind it.  Undecided: only rows of frames that touch the zero padding - the
    stream's first, its last two - and of junk frames; at most 2 % of the rows, and exactly UNDECIDED[name]."""
    inp, _, taps, v = modelled(name)
    c = inp.case
    fv = v.reshape(-1, c.ch)
    n_frames = fv.shape[0]
    may = set()
    seen = set()
    for at, n, f0, total, kind, who in inp.segs:
        if at + n < n_frames:
            may.add(at + n)                                               # the junk frame
        for j in range(n):
            sf, what = f0 + j, (name, who, kind, f0 + j)
            if sf in (0, total - 2, total - 1):
                may.add(at + j)
            inner = 1 <= sf < total - 2
            if kind == "noise":
                if inner:
                    assert (fv[at + j] == -1).all(), what
                    seen.add("noise")
            elif kind == "silence":
                assert (fv[at + j] == 1).all(), what                      # silence passes, padding or not
                seen.add("silence")
            else:
                if (2 if kind == "click-first" else 1) <= sf < total - 2:
                    assert (fv[at + j] == 1).all(), what
                    seen.add("quiet")
                if (kind == "click-first" and sf == 0) or (kind == "click-last" and sf == total - 1):
                    assert (fv[at + j] == -1).all(), what
                    seen.add("click")
    und = set(np.flatnonzero((fv == 0).any(1)).tolist())
    count = int((v == 0).sum())
    assert und <= may, (name, sorted(und - may))
    assert count * 50 <= c.M, f"{name}: {count} of {c.M} rows undecided: over 2 %"
    assert count == UNDECIDED[name], (name, count, sorted(und))
    assert {"noise", "silence", "quiet"} <= seen | ({"silence"} if name == "push-small" else set()), (name, seen)   # (two lanes: tonal, noise)
    assert "click" in seen or name in ("push-middle", "push-gap", "push-middle-s32", "push-gap-s32", "push-small"), (name, seen)
    lo, hi = window(name)
    assert 0 < lo <= hi < c.M


def test_a_wrong_screen_changes_a_byte_of_a_real_frame_on_every_input_of_256_rows():
    """The record model (encode_screen_edges.screen_records) on the drivers' rows.  Unmutated it gives the oracle's bytes
    in every frame whose rows the row model decides.  Then, for every input of 256 rows or more, at least one of
    MUTATIONS changes a record byte of a frame some clip or lane owns - not only of junk frames, which no blob holds."""
    report = {}
    for name in NAMES:
        inp, rec, taps, v = modelled(name)
        c = inp.case
        if c.M < 256:
            continue
        rows = E.Rows(c, taps)
        rb = O.record_bytes(c.ch)
        exp = rec.reshape(-1, rb)
        got, _, stray = E.screen_records(c, rows, rec, E.flags(c, taps))
        decided = (v.reshape(-1, c.ch) != 0).all(1)
        assert not stray and np.array_equal(got.reshape(-1, rb)[decided], exp[decided]), f"{name}: the unmutated model differs from the oracle"
        real = inp.real_frames()
        hit = []
        for mut in sorted(E.MUTATIONS):
            if mut == 10:                 # a sequence of two launches on one workspace: not a property of one input
                continue
            got, _, _ = E.screen_records(c, rows, rec, E.flags(c, taps, mut), mut)
            bad = (got.reshape(-1, rb) != exp).any(1) & decided & real
            if bad.any():
                hit.append((mut, int(bad.sum())))
        report[name] = hit
        assert hit, f"{name}: no mutation changes a byte of a real frame"
    print("; ".join(f"{n}: " + ", ".join(f"{m} ({k} frames)" for m, k in h) for n, h in report.items()))
    assert set(report) == {n for n in NAMES if D.inputs()[n].rows >= 256}


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

# (label, screen mode, bound kind, repair kind, edge kind)
COMBOS = [("fma-tiles", 2, 1, 1, 0), ("fma-latency", 2, 1, 2, 0), ("mx-tiles", 2, 2, 1, 0), ("mx-latency", 2, 2, 2, 0),
          ("automatic-kinds", 2, 0, 0, 0), ("edge-forced", 2, 0, 0, 2), ("off", 1, 0, 0, 0)]


class Gpu:
    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
        import glc_amd
        import test_stream_encode as TS
        E.S.bind(glc_amd)
        self.torch, self.g, self.lib, self.L, self.TS = torch, glc_amd, glc_amd.lib, glc_amd._lib, TS
        self.stream_env = TS.Env()                      # its .enc is the ONE context every push session here lives on
        self._ctx = {"push": self.stream_env.enc}
        self.oracle = {}

    def ctx(self, kind):
        if kind not in self._ctx:
            self._ctx[kind] = self.g.RoundTrip(SR) if kind == "rtpcm" else self.g.Encoder(SR)
        return self._ctx[kind]

    def fresh(self):
        return self.g.Encoder(SR)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    def close(self):
        for k, c in self._ctx.items():
            if k != "push":
                c.close()
        self._ctx.clear()
        self.stream_env.cache.clear()
        self.stream_env.enc = self.stream_env.ref = None

    def want(self, name, i, wide, ch):
        """(oracle .glc bytes, oracle decode of them) of clip or lane i of an input, once."""
        if (name, i) not in self.oracle:
            glc = O.encode(wide, SR, ch).glc
            self.oracle[(name, i)] = (glc, O.decode(glc)[0])
        return self.oracle[(name, i)]

    def counters(self, ctx):
        """(rows screened, rows repaired, repairs by tiles, by latency, edge launches, edge rows) of a context so far."""
        out = list(E.S.stats(self.g, ctx))
        for f in (self.lib.glc_debug_encode_repair_stats, self.lib.glc_debug_encode_edge_stats):
            a, b = C.c_uint64(), C.c_uint64()
            assert f(ctx._h, C.byref(a), C.byref(b)) == 0
            out += [a.value, b.value]
        return np.array(out, np.int64)

    def tap(self, ctx, rows):
        """(H, A) per row of the context's last screened launch, which must have had `rows` rows; None where it had not."""
        h, a = np.zeros(rows, F32), np.zeros(rows, F32)
        pf = C.POINTER(C.c_float)
        rc = self.lib.glc_debug_encode_bound_tap(ctx._h, rows, h.ctypes.data_as(pf), a.ctypes.data_as(pf))
        return (h, a) if rc == 0 else None

    @contextmanager
    def settings(self, ctx, mode, bound, repair, edge):
        lib, h = self.lib, ctx._h
        try:
            assert lib.glc_debug_set_encode_bound(h, bound) == 0 and lib.glc_debug_set_encode_repair(h, repair) == 0
            assert lib.glc_debug_set_encode_edge(h, edge) == 0 and lib.glc_debug_set_encode_screen(h, mode) == 0
            yield
        finally:
            assert lib.glc_debug_set_encode_screen(h, 0) == 0 and lib.glc_debug_set_encode_bound(h, 0) == 0
            assert lib.glc_debug_set_encode_repair(h, 0) == 0 and lib.glc_debug_set_encode_edge(h, 0) == 0


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.close()


def takes(inp, mode, bound):
    """Whether the forced mode screens a launch of the input's rows: 256 rows, 128 where the matrix kind is forced and
    the form is built for the channel count."""
    return mode == 2 and inp.rows >= (128 if bound == 2 and inp.ch in BUILT else 256)


def check_counts(gpu, ctx, inp, combo, delta, taps):
    """One launch of the input under one combination: the counters' deltas, and the tap where it was screened."""
    label, mode, bound, repair, edge = combo
    screened, repaired, tiles, latency, edge_launches, edge_rows = (int(x) for x in delta)
    lo, hi = window(inp.name)
    print(f"{inp.name} [{label}]: screened {screened} of {inp.rows}, repaired {repaired}, model {lo}..{hi}, "
          f"repairs by tiles / latency {tiles} / {latency}")
    assert (edge_launches, edge_rows) == (0, 0), f"{inp.name} [{label}]: a driver's launch took the edge side stream"
    if not takes(inp, mode, bound):
        assert (screened, repaired, tiles, latency) == (0, 0, 0, 0), f"{inp.name} [{label}]: a launch of {inp.rows} rows was screened"
        return
    assert screened == inp.rows, f"{inp.name} [{label}]: {screened} of {inp.rows} rows went through the screened path"
    assert lo <= repaired <= hi, f"{inp.name} [{label}]: {repaired} rows repaired, the model has {lo}..{hi}"
    assert tiles + latency == 1 and (repair == 0 or (tiles, latency) == ((1, 0) if repair == 1 else (0, 1))), (inp.name, label, tiles, latency)
    t = gpu.tap(ctx, inp.rows)
    assert t is not None, f"{inp.name} [{label}]: the last screened launch on slot 0 was not one of {inp.rows} rows"
    assert gpu.tap(ctx, inp.rows + 1) is None
    taps[(inp.name, label)] = t


def check_forms(inp, taps):
    """Which form took the launches, from H: the FMA form's fused sums are the same numbers whenever they are formed, the
    matrix pipe's sums of bf16 pieces are others.  Built channel counts: H under the forced matrix kind differs from H
    under the forced FMA kind.  3 channels: the form is not built, the forced matrix kind keeps the FMA form - the same
    H bit for bit, and the 256-row threshold."""
    fma, mx = taps.get((inp.name, "fma-tiles")), taps.get((inp.name, "mx-tiles"))
    if fma is None or mx is None:
        assert inp.rows < 256
        return
    assert np.array_equal(fma[1].view(np.uint32), taps[(inp.name, "fma-latency")][1].view(np.uint32))
    same = np.array_equal(fma[0].view(np.uint32), mx[0].view(np.uint32))
    if inp.ch in BUILT:
        assert not same, f"{inp.name}: H under the forced matrix kind is the FMA form's: the matrix form did not take the launch"
    else:
        assert same, f"{inp.name}: {inp.ch} channels under the forced matrix kind did not keep the FMA form"


# -------------------------------------------------------------------------------------- the store encode

def layout_of(gpu, inp):
    """The input's clips in a flat array as a glc_clip_layout says (stream_encode_cases.Layout: odd strides, `off`
    elements in front, NaN or full-scale integers everywhere else) -> (Layout with .d uploaded, glc_clip_layout, keep)."""
    lens = [w.size // inp.ch for w in inp.wide]
    lay = SC.Layout(inp.ch, lens, inp.planar, inp.fmt, inp.off)
    for i, x in enumerate(inp.clips):
        lay.put(i, x)
    lay.d = gpu.dev(lay.flat)
    arr = (C.c_uint64 * len(lens))(*lens)
    cl = gpu.L.GlcClipLayout(len(lens), inp.ch, 1 if lay.planar else 0, lay.clip_stride, lay.channel_stride, 0, C.cast(arr, C.POINTER(C.c_uint64)))
    return lay, cl, arr


def store_once(gpu, ctx, inp, staged):
    """One glc_encode_batch_device_compact(_int) of the input into a pattern-filled arena whose cursor stands at 130 ->
    the clips' blobs.  Entries, cursor, every arena byte outside the blobs and the input itself are checked."""
    torch, lib = gpu.torch, gpu.lib
    lay, cl, _keep = staged
    n = len(inp.clips)
    cursor0, first = 130, 192
    size = first + gpu.g.compact_store_bound(inp.ch, lay.lens) + 4096
    image = gpu.TS.pattern(size, seed=7)
    arena = gpu.dev(image)
    cursor = torch.tensor([cursor0], dtype=torch.int64, device="cuda")
    entries = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
    p = C.c_void_p(lay.d.data_ptr() + lay.off * lay.d.element_size())
    if inp.fmt == D.PF32:
        rc = lib.glc_encode_batch_device_compact(ctx._h, p, C.byref(cl), C.c_void_p(arena.data_ptr()), size, C.c_void_p(cursor.data_ptr()),
                                                 C.c_void_p(entries.data_ptr()))
    else:
        rc = lib.glc_encode_batch_device_compact_int(ctx._h, p, inp.fmt, inp.bits, C.byref(cl), C.c_void_p(arena.data_ptr()), size,
                                                     C.c_void_p(cursor.data_ptr()), C.c_void_p(entries.data_ptr()))
    assert rc == 0, lib.glc_last_error(ctx._h)
    ctx.synchronize()
    assert lib.glc_ctx_resident_stream(ctx._h) == 0
    assert np.array_equal(lay.d.cpu().numpy().view(np.uint8), lay.flat.view(np.uint8)), "the input was written"
    a, ent = arena.cpu().numpy(), entries.cpu().numpy()
    at, blobs = first, []
    for i in range(n):
        o, nb, _, rs = (int(x) for x in ent[i])
        assert rs >> 32 == 1 and o == at and nb > 0 and nb % 64 == 0, (inp.name, i, ent[i].tolist())
        blobs.append(a[o:o + nb].tobytes())
        at += nb
    assert int(cursor.item()) == at
    assert np.array_equal(a[:first], image[:first]) and np.array_equal(a[at:], image[at:]), "arena bytes outside the blobs were written"
    return blobs


@pytest.mark.gpu
@pytest.mark.parametrize("name", STORE)
def test_gpu_store_encode_screens_its_packed_round(gpu, name):
    """glc_encode_batch_device_compact / _int: one packed round {vs, 0, T} over frames 0 .. V, junk frames included."""
    inp = modelled(name)[0]
    ctx = gpu.ctx("store")
    staged = layout_of(gpu, inp)
    refs = [gpu.want(name, i, w, inp.ch)[0] for i, w in enumerate(inp.wide)]
    taps, out = {}, {}
    for combo in COMBOS:
        with gpu.settings(ctx, *combo[1:]):
            c0 = gpu.counters(ctx)
            blobs = store_once(gpu, ctx, inp, staged)
            check_counts(gpu, ctx, inp, combo, gpu.counters(ctx) - c0, taps)
        for i, (blob, w) in enumerate(zip(blobs, inp.wide)):
            got = gpu.g.EncodedAudio.from_compact(SR, w.size, inp.ch, [blob]).to_bytes()
            assert got == refs[i], f"{name} [{combo[0]}]: clip {i} differs from the oracle's encode of it alone"
        out[combo[0]] = blobs
    assert all(b == out["off"] for b in out.values())
    check_forms(inp, taps)
    if name == "store-ch3":                         # not built: the forced matrix kind screened it, from 256 rows, in the FMA form
        assert ("store-ch3", "mx-tiles") in taps and inp.rows >= 256


# -------------------------------------------------------------------------------------- the PCM round trip

def _clip_layout(gpu, b):
    arr = (C.c_uint64 * b.n_clips)(*b.lengths)
    return gpu.L.GlcClipLayout(b.n_clips, b.ch, 1 if b.planar else 0, b.clip_stride, b.channel_stride, max(b.lengths),
                               C.cast(arr, C.POINTER(C.c_uint64))), arr


@pytest.mark.gpu
def test_gpu_roundtrip_pcm_decodes_the_records_the_screen_and_the_repair_left(gpu):
    """glc_roundtrip_batch_device_pcm, S16 planar in and S16 interleaved out: the words of every clip are the S16
    narrowing (store_int_cases.narrow) of the oracle's decode of its own encode of the widened clip; every other word of
    the output keeps its sentinel and the input is unchanged."""
    name = "rtpcm-s16"
    inp = modelled(name)[0]
    ch = inp.ch
    ctx = gpu.ctx("rtpcm")
    b = SI.input_batch([x.reshape(-1, ch) for x in inp.clips], ch, True, inp.off, np.int16)
    ob = SI.output_batch(b.lengths, ch, False, 2, np.int16, pad=7)
    lin, _k1 = _clip_layout(gpu, b)
    lout, _k2 = _clip_layout(gpu, ob)
    want = ob.flat.copy()
    for i, w in enumerate(inp.wide):
        dec = gpu.want(name, i, w, ch)[1]
        assert dec.size == w.size
        want[ob.index[i]] = SI.narrow(dec)
    d_in = gpu.dev(b.flat)
    taps = {}
    for combo in COMBOS:
        d_out = gpu.dev(ob.flat)
        with gpu.settings(ctx, *combo[1:]):
            c0 = gpu.counters(ctx)
            rc = gpu.lib.glc_roundtrip_batch_device_pcm(ctx._h, C.c_void_p(d_in.data_ptr() + 2 * b.off), D.S16, 16, C.byref(lin),
                                                        C.c_void_p(d_out.data_ptr() + 2 * ob.off), D.S16, C.byref(lout))
            assert rc == 0, gpu.lib.glc_last_error(ctx._h)
            ctx.synchronize()
            check_counts(gpu, ctx, inp, combo, gpu.counters(ctx) - c0, taps)
        got = d_out.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name} [{combo[0]}]: {bad.size} words differ, first at {bad[0]} (a clip's own: {bool(ob.mask[bad[0]])})"
        assert np.array_equal(d_in.cpu().numpy(), b.flat)
    assert (want[ob.mask] != 0).any()
    check_forms(inp, taps)


# -------------------------------------------------------------------------------------- the stream push

def push_session(gpu, session, combo, taps, host=False):
    """The session's pushes on a new session of the push context under one combination.  Device pushes go through
    test_stream_encode.drive_device - one pattern-filled arena and cursor, the segments against the plan, entries of
    lanes that complete nothing untouched, no arena byte outside the blobs written - with the counters read after every
    push; host pushes through drive_host, the counters read over the whole session.  Every lane's stream, assembled
    from its blobs, is the oracle's encode of the whole lane."""
    TS, env = gpu.TS, gpu.stream_env
    ctx = gpu.ctx("push")
    inputs = {i.push: i for i in session.inputs()}
    lanes = session.lanes()
    ch, n = session.ch, len(lanes)
    seen = [gpu.counters(ctx)]
    at_push = [0]

    def probe():
        k = at_push[0]
        at_push[0] += 1
        seen.append(gpu.counters(ctx))
        if k in inputs:
            check_counts(gpu, ctx, inputs[k], combo, seen[-1] - seen[-2], taps)
        else:                                       # a push that only ends streams: a few rows, under every threshold
            assert (seen[-1] == seen[-2]).all(), (session.tag, combo[0], k)

    with gpu.settings(ctx, *combo[1:]):
        with TS.Session(env, ch, n) as S:
            if host:
                got = TS.drive_host(S, lanes, session.fmt, session.bits)
                total = gpu.counters(ctx) - seen[0]
            else:
                lens = [w.size // ch for w in session.wide]
                size = gpu.g.compact_store_bound(ch, lens) + 8192 * n * len(session.pushes()) + 4096
                dev = TS.drive_device(env, S, lanes, session.planar, session.fmt, session.bits, session.off, arena_size=size, between=probe)
                assert at_push[0] == len(session.pushes())
                got = [[env.assemble([b for _, _, b in stream], w.size, ch) for stream in lane] for lane, w in zip(dev, session.wide)]
    for i, w in enumerate(session.wide):
        assert len(got[i]) == 1 and got[i][0] == gpu.want(session.tag, i, w, ch)[0], \
            f"{session.tag} [{combo[0]}{', host' if host else ''}]: lane {i} differs from the oracle's encode of its whole stream"
    if host:
        label, mode, bound = combo[0], combo[1], combo[2]
        on = [i for i in inputs.values() if takes(i, mode, bound)]
        lo, hi = sum(window(i.name)[0] for i in on), sum(window(i.name)[1] for i in on)
        print(f"{session.tag} [{label}, host]: screened {int(total[0])} of {sum(i.rows for i in on)}, repaired {int(total[1])}, model {lo}..{hi}")
        assert int(total[0]) == sum(i.rows for i in on) and lo <= int(total[1]) <= hi
        assert int(total[2] + total[3]) == len(on) and (int(total[4]), int(total[5])) == (0, 0)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["main-f32", "main-s32"])
def test_gpu_stream_push_screens_frames_1_to_v_minus_1_of_every_push(gpu, tag):
    """8 stereo lanes, four pushes of one session in order, so that what a screened push holds back feeds the next:
    frames 0..19, 20..39, 40..48 (158 rows: screened only where the forced matrix kind lowers the threshold to 128) and
    49..69 with the finish.  Planar float32, and 24-bit integers interleaved in 32-bit words."""
    session = D.sessions()[tag]
    taps, out = {}, {}
    for combo in COMBOS:
        out[combo[0]] = push_session(gpu, session, combo, taps)
    assert all(o == out["off"] for o in out.values())
    for inp in session.inputs():
        check_forms(inp, taps)
    gap = next(i for i in session.inputs() if i.name.startswith("push-gap"))
    assert (gap.name, "mx-tiles") in taps and (gap.name, "fma-tiles") not in taps


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["fma-tiles", "mx-latency", "off"])
def test_gpu_host_push_screens_the_same_rows(gpu, label):
    """glc_stream_enc_push stages the same virtual streams from a pinned copy of the chunks: StreamEncoder.encoded's
    bytes (glc_stream_enc_frames) per lane against the oracle, the counters over the whole session."""
    combo = next(c for c in COMBOS if c[0] == label)
    push_session(gpu, D.sessions()["main-f32"], combo, {}, host=True)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["ragged", "ch4", "small"])
def test_gpu_stream_push_ragged_four_channels_and_under_the_threshold(gpu, tag):
    """ragged: lanes that get nothing, lanes that are held back only, one that finishes and four that complete 30 frames
    in ONE push (258 rows; the second push only ends the streams and is never screened).  ch4: the fused raw decision.
    small: 42 rows - never screened, whatever is forced."""
    session = D.sessions()[tag]
    taps, out = {}, {}
    for combo in COMBOS:
        out[combo[0]] = push_session(gpu, session, combo, taps)
    assert all(o == out["off"] for o in out.values())
    for inp in session.inputs():
        check_forms(inp, taps)
    if tag == "small":
        assert not taps


# -------------------------------------------------------------------------------------- automatic mode, a lng round

_lng = {}


def lng_model():
    """(clip, oracle bytes, (lo, hi) of the first chunk's rows), once per session: about 15 s of CPU."""
    if not _lng:
        x = D.lng_clip()
        c = E.whole_case("lng", SR, 2, x)
        _, taps = E.expected(c)
        v = E.model(c, taps)[:D.LNG_CHUNK * 2]
        _lng["x"] = (x, O.encode(x, SR, 2).glc, (int((v == -1).sum()), int((v != 1).sum())))
    return _lng["x"]


@pytest.mark.gpu
def test_gpu_automatic_mode_screens_the_full_chunk_of_a_long_clip_in_the_matrix_form(gpu):
    """A store encode, in mode 0 with every kind 0 on a fresh context, of ONE stereo clip of 4396 frames at 48 kHz.
    The round rule (glc_rounds.hpp pack_rounds) makes it a round of its own: 4396 + 1 slots pass the budget of 4096.
    The driver encodes it as a real stream of its own length in chunks of 4096 frames on slot 0, without
    kEncodeAlternate and without kEncodeEdge.  From ScreenPolicy:
      chunk 0, 4096 frames = 8192 rows: may() is mdct_forward_is_st16 - 8192 >= 3584 and its 32 row tiles fill the last
        round of 32 - so the launch is eligible; no slot has a count pending and backoff is 0, so admit() lets it
        through: a fresh context's first screened launch is its probe.  matrix_bound(): built for stereo at 48 kHz and
        8192 >= 3584 - the matrix form.  latency_repair(): no count has been read - the tile repair.
      chunk 1, 300 frames = 600 rows: under 3584, not eligible.
    So rows_screened moves by exactly 8192, one repair by tiles is counted, nothing on the edge side stream, and the
    bound tap answers for 8192 rows and refuses 600.  rows_repaired lies in the model's window of the first chunk's rows,
    whose lower end is at least the clicked frame's two."""
    x, ref, (lo, hi) = lng_model()
    assert lo > 0
    inp = D.batch_input("lng", "store", 2, D.PF32, 32, True, 1, [x])
    ctx = gpu.fresh()
    try:
        staged = layout_of(gpu, inp)
        c0 = gpu.counters(ctx)
        blob = store_once(gpu, ctx, inp, staged)[0]
        screened, repaired, tiles, latency, el, er = (int(v) for v in gpu.counters(ctx) - c0)
        print(f"lng, automatic: screened {screened} of {D.LNG_FRAMES * 2}, repaired {repaired}, model {lo}..{hi}, "
              f"repairs by tiles / latency {tiles} / {latency}")
        assert gpu.g.EncodedAudio.from_compact(SR, x.size, 2, [blob]).to_bytes() == ref, "mode 0: the blob differs from the oracle's stream"
        assert screened == D.LNG_CHUNK * 2 == 8192
        assert lo <= repaired <= hi
        assert (tiles, latency, el, er) == (1, 0, 0, 0)
        assert gpu.tap(ctx, 8192) is not None and gpu.tap(ctx, 600) is None
        with gpu.settings(ctx, 1, 0, 0, 0):
            c0 = gpu.counters(ctx)
            off = store_once(gpu, ctx, inp, staged)[0]
            assert (gpu.counters(ctx) == c0).all()
        assert off == blob
    finally:
        ctx.close()
